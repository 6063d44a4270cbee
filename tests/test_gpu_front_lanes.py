"""GPU parity of the front mode of fq_pwconv_i8_stat at every lane filling and both workgroup sizes: row widths whose quarter
(the lanes of a row segment) divides 64 and widths where it does not, 16 to 128 channels, bands of 1, 5, 7 and 8 rows on planes of
9 and 13 rows (a short last band each time), four wavefronts per workgroup and - where the launch has them, 64 and 128 channels -
eight (FQ_PWSTAT_FRONT_WAVES).  The reference is the plain statistic pass on the tensor the storing depthwise launch wrote: both
statistics, both `current_input_max` and every byte of `x_codes_out` are compared bit for bit; the codes the depthwise statistic
pass keeps are compared with the host oracle's quantiser.  Every launch works from poisoned, guard-banded memory
(tests/poison.py).  That the knob is obeyed is seen from the outside: the profiler's record of the launches names the
instantiation that ran, and its last template argument is the wavefront count (that no shape here falls back to four for want
of LDS is tests/test_front_waves.py's, on the plan the launch calls)."""
import re

import numpy as np
import pytest
import torch

import poison
from test_gpu_front_dw import _compare, _input_codes, _make, _operands, _two_launches
from test_gpu_pwdw import N, _eq

pytestmark = pytest.mark.gpu

# Q = W / 4 = 3, 7, 9, 14, 15, 28 leave 1, 1, 1, 8, 4 and 8 of a wavefront's 64 lanes without a whole row segment; 16 and 64
# (Q = 4, 16) fill it, as does 256 (Q = 64: one row segment per wavefront, the widest plane the kernel takes; its bands have at
# most four rows, so the forced 5, 7 and 8 are clamped to that)
WIDTHS = (12, 28, 36, 56, 60, 112, 16, 64, 256)
CINS = (16, 32, 64, 128)
HEIGHTS = (9, 13)
ROWS = (1, 5, 7, 8)
COUT = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


def _waves(cin):
    return (4, 8) if cin >= 64 else (4,)


def _run(k, o, dev, ops, proxy):
    """The depthwise statistic pass and the 1x1 statistic pass that recomputes the layer (handed an x of NaN), on operands
    that are already in place; every output comes from the proxy."""
    n, cin, cout, h, w = k["case"]
    empty = lambda shape, dtype: proxy.empty(shape, dtype=dtype, device=dev)      # noqa: E731
    curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    s0 = ops.absmax_per_sample(o["y0"])
    ycodes = empty(ops.front_codes_shape(o["y0"].shape), torch.int8)
    none, zstat = ops.dwconv3x3(o["y0"], o["dww"], o["biasA"], stride=1, in_stat=s0, width=8, flags=o["fA"], cur_out=curA,
                                bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"], store=False, x_codes_out=ycodes)
    assert none is None
    buf = empty(ops.pair_codes_shape((n, cin, h, w)), torch.int8)
    front = dict(x_codes=ycodes, w=o["dww"], bias=o["biasA"], bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"],
                 in_stat=s0, width=8, flags=o["fA"])
    pstat = ops.pwconv_i8_stat(o["nan"], o["wc"], o["scales"], o["rowsum"], None, in_stat=zstat, in_thr=o["thrB"], width=8,
                               flags=o["fB"], cur_out=curB, bn_scale=o["bnB"][0], bn_shift=o["bnB"][1], act=k["actB"],
                               x_codes_out=buf, front=front)
    return dict(zstat=N(zstat), curA=N(curA), pstat=N(pstat), curB=N(curB), buf=N(buf), ycodes=N(ycodes))


def _sweep(case, mode, rows, pattern, dev, ops, monkeypatch):
    n, cin, cout, h, w = case
    assert ops.pwconv_front_supported((n, cin, h, w), cout), "shape refused: %s" % (case,)
    k = _make(case, mode)
    want = _two_launches(k, dev, ops)                          # the reference: once per shape, never changed
    host = _input_codes(k)
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        o = _operands(k, dev, ops, lambda a: proxy.guarded(a, dev))
        o["nan"] = torch.full((n, cin, h, w), float("nan"), device=dev)
        for r in rows:
            for waves in _waves(cin):
                monkeypatch.setenv("FQ_PWSTAT_FRONT_ROWS", str(r))
                monkeypatch.setenv("FQ_PWSTAT_FRONT_WAVES", str(waves))
                got = _run(k, o, dev, ops, proxy)
                try:
                    _compare(got, want, k)
                    _eq(got["ycodes"], host, "codes of the depthwise input vs the host oracle's quantiser")
                except AssertionError as e:
                    raise AssertionError("%d rows per band, %d wavefronts: %s" % (r, waves, e))
        torch.cuda.synchronize()
        proxy.guards_intact()
        _eq(N(o["y0"]), k["y0"], "the depthwise input after all launches")
    finally:
        proxy.release()
        ops._WS.clear()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("cin", CINS)
def test_every_lane_filling_and_both_workgroup_sizes(dev, ops, monkeypatch, cin, w):
    for h, pattern in zip(HEIGHTS, poison.PATTERNS):
        _sweep((3, cin, COUT, h, w), "u8_bn_relu", ROWS, pattern, dev, ops, monkeypatch)


@pytest.mark.parametrize("case", [(3, 128, COUT, 13, 36), (3, 32, COUT, 9, 60)], ids=["128@13x36", "32@9x60"])
def test_signed_input_codes(dev, ops, monkeypatch, case):
    """Two's complement bytes in the code buffer of the depthwise input (FQ_ACT_SIGNED on the layer in front)."""
    _sweep(case, "s8_front", (5, 8), 0xFF, dev, ops, monkeypatch)
    assert (_input_codes(_make(case, "s8_front")) < 0).any()


@pytest.mark.parametrize("cin", (64, 128))
def test_the_knob_launches_the_workgroup_size_it_names(dev, ops, monkeypatch, cin):
    """FQ_PWSTAT_FRONT_WAVES = 4 and 8: the kernel the profiler saw is pw_stat_kernel<slabs, epilogue, signed, WAVES>."""
    from torch.profiler import ProfilerActivity, profile
    k = _make((3, cin, COUT, 9, 36), "u8_bn_relu")
    o = _operands(k, dev, ops, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    o["nan"] = torch.full((3, cin, 9, 36), float("nan"), device=dev)
    monkeypatch.setenv("FQ_PWSTAT_FRONT_ROWS", "5")
    seen = {}
    for waves in (4, 8):
        monkeypatch.setenv("FQ_PWSTAT_FRONT_WAVES", str(waves))
        _run(k, o, dev, ops, torch)                                # (first call of an instantiation: its set-up stays outside)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _run(k, o, dev, ops, torch)
            torch.cuda.synchronize()
        names = sorted(set(e.name for e in prof.events() if "pw_stat_kernel" in e.name))
        seen[waves] = [int(m.group(1)) for m in (re.search(r"pw_stat_kernel<[^>]*,\s*(\d+)\s*>", nm) for nm in names) if m]
        assert names and len(seen[waves]) == len(names), names
    assert seen == {4: [4], 8: [8]}, seen
