"""GPU parity of the STORING 1x1 with a front layer (fq_pwconv_i8_front, `ops.pwconv_i8(front=)`): fq_dwconv3x3 without y (the statistic pass that keeps
its input's codes) followed by fq_pwconv_i8_front (which recomputes the depthwise values from those codes and stores the 1x1's
output) against the two launches they replace - fq_dwconv3x3 storing z, fq_pwconv_i8 reading it.  No value may change: every
comparison is bit for bit (y, both statistics, both `current_input_max`), also from poisoned, guard-banded memory
(tests/poison.py).  The depthwise statistic pass is checked on the same shapes: its codes against the host oracle's, its maxima
against the storing launch."""
import numpy as np
import pytest
import torch

import poison
import regimes as R
from test_gpu_front_dw import _input_codes, _make
from test_gpu_pwdw import N, _eq, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


# (n, C, H, W, Cout) -> forced rows per band (None: the rule's).  The real plane; bands of 4, 4 and 1 rows; nine and three lanes
# per row with a short last pixel tile (5 x 36 = 180 = 5 tiles + 20, 6 x 12 = 72 = 2 tiles + 8); planes of one and of two rows -
# no row above or below.
SHAPES = {
    (2, 256, 28, 28, 256): None,
    (3, 256, 9, 28, 256): 4,
    (2, 256, 5, 36, 256): None,
    (2, 256, 6, 12, 256): None,
    (1, 256, 1, 28, 256): None,
    (1, 256, 2, 28, 256): None,
    (2, 256, 2, 28, 256): None,                             # (the same with an all-zero sample beside it)
}
IDS = ["%dx%dx%dx%d->%d" % s for s in SHAPES]
SMALL = (3, 256, 9, 28, 256)
# the quantisers of tests/test_gpu_front_dw.py (unsigned fast path, ReLU6, depthwise bias with the run-time epilogue, signed codes
# on either side, a stored threshold make_fast_quot declines) and the 1x1's own epilogues: ReLU6, and the run-time one with a bias
MODES = ["u8_bn_relu", "u8_bn_relu6", "u8_bias_none", "s8_front", "s8_pw", "s8_both", "u8_no_fast_quot", "u8_pw_relu6", "u8_pw_bias"]


def _k(shape, mode, **kw):
    n, c, h, w, cout = shape
    k = _make((n, c, cout, h, w), mode, **kw)
    k["biasB"] = None
    if "pw_relu6" in mode:
        k["actB"] = "relu6"
    if "pw_bias" in mode:                                   # bias, BatchNorm, no activation: the 1x1's run-time epilogue
        k["biasB"] = (np.random.default_rng(c + w).standard_normal(cout) * 0.5).astype(np.float32)
        k["actB"] = None
    return k


def _operands(k, dev, ops, put):
    n, cin, cout, h, w = k["case"]
    o = dict(y0=put(k["y0"]), dww=put(k["dww"]), biasA=None if k["biasA"] is None else put(k["biasA"]),
             bnA=tuple(None if a is None else put(a) for a in k["bnA"]), bnB=tuple(put(a) for a in k["bnB"]),
             biasB=None if k["biasB"] is None else put(k["biasB"]))
    o["wc"], o["scales"], o["rowsum"] = ops.weight_codes(_t(k["w1"], dev), cout, 8)
    o["fA"], o["fB"] = ops.act_flags(signed=k["s_front"]), ops.act_flags(signed=k["s_pw"])
    o["thrB"] = None if k["thrB"] is None else put(np.float32([k["thrB"]]))
    return o


def _two_launches(k, dev, ops):
    """The reference: the storing depthwise launch, then the storing 1x1 reading what it stored."""
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    s0 = ops.absmax_per_sample(o["y0"])
    z, zstat = ops.dwconv3x3(o["y0"], o["dww"], o["biasA"], stride=1, in_stat=s0, width=k["front_width"], flags=o["fA"], cur_out=curA,
                             bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"])
    y, ystat = ops.pwconv_i8(z, o["wc"], o["scales"], o["rowsum"], o["biasB"], in_stat=zstat, in_thr=o["thrB"], width=k["width"],
                             flags=o["fB"], cur_out=curB, bn_scale=o["bnB"][0], bn_shift=o["bnB"][1], act=k["actB"])
    return dict(zstat=N(zstat), curA=N(curA), ystat=N(ystat), curB=N(curB), y=N(y), z=N(z))


def _fold(k, dev, ops, put=None, empty=None, x="nan"):
    """The statistic pass of the depthwise layer, then the storing 1x1 that recomputes it - handed an x of NaN, or none."""
    put = put or (lambda a: _t(a, dev))
    empty = empty or (lambda shape, dtype: torch.full(shape, 0x55, dtype=dtype, device=dev))
    o = _operands(k, dev, ops, put)
    n, cin, cout, h, w = k["case"]
    curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    s0 = ops.absmax_per_sample(o["y0"])
    ycodes = empty(ops.front_codes_shape(o["y0"].shape), torch.int8)
    none, zstat = ops.dwconv3x3(o["y0"], o["dww"], o["biasA"], stride=1, in_stat=s0, width=k["front_width"], flags=o["fA"], cur_out=curA,
                                bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"], store=False, x_codes_out=ycodes)
    assert none is None
    front = dict(x_codes=ycodes, w=o["dww"], bias=o["biasA"], bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"],
                 in_stat=s0, width=k["front_width"], flags=o["fA"])
    xarg = torch.full((n, cin, h, w), float("nan"), device=dev) if x == "nan" else (n, cin, h, w)      # (a shape: x == NULL)
    y, ystat = ops.pwconv_i8(xarg, o["wc"], o["scales"], o["rowsum"], o["biasB"], front=front, in_stat=zstat,
                             in_thr=o["thrB"], width=k["width"], flags=o["fB"], cur_out=curB, bn_scale=o["bnB"][0],
                             bn_shift=o["bnB"][1], act=k["actB"])
    return dict(zstat=N(zstat), curA=N(curA), ystat=N(ystat), curB=N(curB), y=N(y), ycodes=N(ycodes), y0=N(o["y0"]))


_REFERENCE = {}


def _reference(shape, mode, dev, ops, **kw):
    """(inputs, results of the two storing launches): computed once per case, shared, never changed."""
    key = (shape, mode, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        k = _k(shape, mode, **kw)
        _REFERENCE[key] = (k, _two_launches(k, dev, ops))
    return _REFERENCE[key]


def _compare(got, want):
    _eq(got["zstat"], want["zstat"], "per-sample statistic of the depthwise output (statistic pass vs storing launch)")
    _eq(got["curA"], want["curA"], "current_input_max of the depthwise block")
    _eq(got["curB"], want["curB"], "current_input_max of the 1x1 block")
    _eq(got["ystat"], want["ystat"], "per-sample statistic of the 1x1 output")
    _eq(got["y"], want["y"], "the 1x1 output, every byte")


def _forced(monkeypatch, rows, waves):
    for name, v in (("FQ_PWSTAT_FRONT_ROWS", rows), ("FQ_PWSTAT_FRONT_WAVES", waves)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_every_shape_with_four_and_with_eight_wavefronts(dev, ops, monkeypatch, shape, waves):
    n, c, h, w, cout = shape
    assert ops.pwconv_front_store_supported((n, c, h, w), cout), "shape refused: %s" % (shape,)
    k, want = _reference(shape, "u8_bn_relu", dev, ops)
    _forced(monkeypatch, SHAPES[shape], waves)
    got = _fold(k, dev, ops)
    _compare(got, want)
    _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input vs the host oracle's quantiser")
    # what the data holds: an all-zero sample among others (n > 1), a value the online threshold clips, negative sums under ReLU
    assert n == 1 or (not k["y0"][-1].any() and (k["y0"] > want["curA"][0]).any())
    assert (want["y"] == 0).any() and want["ystat"].max() > 0


@pytest.mark.parametrize("mode", MODES[1:])
def test_every_quantiser_and_epilogue(dev, ops, monkeypatch, mode):
    k, want = _reference(SMALL, mode, dev, ops)
    _forced(monkeypatch, 4, 0)
    got = _fold(k, dev, ops, x=None)
    _compare(got, want)
    _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input vs the host oracle's quantiser")
    if "no_fast_quot" in mode:
        den = np.float32(np.float32(np.float32(k["thrB"]) / np.float32(255)) + np.float32(1e-10))
        assert (den.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF
    if "relu6" in mode and "pw" in mode:
        assert want["y"].max() == 6.0


@pytest.mark.parametrize("side", ["front", "pw"])
@pytest.mark.parametrize("width", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("mode", ["u8_bn_relu", "s8_both"])
def test_activation_widths_on_either_quantiser(dev, ops, monkeypatch, mode, width, side):
    kw = dict(front_width=width) if side == "front" else dict(width=width)
    k, want = _reference((2, 256, 6, 12, 256), mode, dev, ops, **kw)
    _forced(monkeypatch, 0, 0)
    _compare(_fold(k, dev, ops), want)


@pytest.mark.parametrize("regime", ["boundaries", "allones_divisor", "eps_scale", "zero"])
def test_value_regimes_on_the_depthwise_input(dev, ops, monkeypatch, regime):
    k, want = _reference((2, 256, 5, 36, 256), "u8_bn_relu", dev, ops, regime=regime)
    _forced(monkeypatch, 0, 0)
    _compare(_fold(k, dev, ops), want)
    if regime == "allones_divisor":
        assert R.has_allones_significand(R.divisor(k["thrB"], False, 8))


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("prezeroed", [False, True])
@pytest.mark.parametrize("shape,mode", [((2, 256, 28, 28, 256), "u8_bn_relu"), (SMALL, "s8_both"), ((2, 256, 5, 36, 256), "u8_pw_bias"),
                                        ((2, 256, 6, 12, 256), "u8_bn_relu6"), ((1, 256, 1, 28, 256), "u8_bias_none")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%dx%d->%d" % v)
def test_from_poisoned_guarded_memory(dev, ops, monkeypatch, shape, mode, prezeroed, pattern):
    """Inputs between guard bands, y and every statistic target poisoned: every byte of y is written, no guard is touched, no
    result carries poison.  `prezeroed`: the statistic rows come from the forward's arena (FQ_STAT_PREZEROED) instead of a fresh
    tensor the launch zeroes itself."""
    k, want = _reference(shape, mode, dev, ops)
    _forced(monkeypatch, SHAPES[shape], 0)
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    arena = ops.StatArena(8, dev) if prezeroed else None
    try:
        if arena is not None:
            arena.begin(shape[0])
        got = _fold(k, dev, ops, put=lambda a: proxy.guarded(a, dev),
                    empty=lambda shape_, dtype: proxy.empty(shape_, dtype=dtype, device=dev))
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert len(proxy.records) >= 8
        _compare(got, want)
        _eq(got["y0"], k["y0"], "the depthwise input after both passes")
        _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input")
    finally:
        if arena is not None:
            arena.end()
        proxy.release()
        ops._WS.clear()


def test_refused_shapes_and_quantisers_launch_nothing(dev, ops, monkeypatch):
    from quantization.mxnet_amd._lib import FakeQuantError
    sup = ops.pwconv_front_store_supported
    assert sup((2, 256, 28, 28), 256)
    assert not sup((2, 256, 7, 30), 256) and not sup((2, 256, 7, 61), 256)          # W % 4 != 0
    assert not sup((2, 512, 14, 28), 256) and not sup((2, 128, 28, 28), 256)        # Cin
    assert not sup((2, 256, 28, 28), 512) and not sup((2, 256, 28, 28), 128)        # Cout
    _forced(monkeypatch, 0, 0)
    k = _k((2, 256, 6, 12, 256), "u8_bn_relu")
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    n, cin, cout, h, w = k["case"]
    s0 = ops.absmax_per_sample(o["y0"])
    with pytest.raises(Exception):                          # a depthwise layer of stride 2 has no statistic pass to stand in front
        ops.dwconv3x3(o["y0"], o["dww"], stride=2, in_stat=s0, store=False)
    ycodes = torch.zeros(ops.front_codes_shape(o["y0"].shape), dtype=torch.int8, device=dev)
    zstat = torch.ones(n, device=dev)
    front = dict(x_codes=ycodes, w=o["dww"], bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act="relu", in_stat=s0, width=8, flags=0)
    proxy = poison.Proxy(0xFF)
    monkeypatch.setattr(ops, "torch", proxy)
    try:
        def refused(**kw):
            args = dict(in_stat=zstat, width=8, flags=0, bn_scale=o["bnB"][0], bn_shift=o["bnB"][1], act="relu")
            f = dict(front, **kw.pop("front", {}))
            args.update(kw)
            with pytest.raises(FakeQuantError):
                ops.pwconv_i8((n, cin, h, w), o["wc"], o["scales"], o["rowsum"], front=f, **args)
        refused(width=9)                                    # widths above 8 on either quantiser
        refused(front=dict(width=9))
        refused(flags=4)                                    # FQ_ACT_NO_ABS / FQ_ACT_NO_EPS: not this launch's quantiser
        refused(front=dict(flags=8))
        refused(front=dict(flags=0x100))                    # (the library's own range-mode bit is no flag of the entry point)
        torch.cuda.synchronize()
        outs = [r for r in proxy.records if r[5] == "empty"]
        assert len(outs) >= 5
        for raw, g, body, dtype, shape_, what in outs:      # nothing was launched: every output is still poison
            assert bool((raw == 0xFF).all()), (shape_, dtype)
    finally:
        proxy.release()
    # a shape the launch does not take: the entry point says so
    w512 = ops.weight_codes(torch.zeros(512, 256, device=dev), 512, 8)
    with pytest.raises(FakeQuantError, match="shape not taken"):
        ops.pwconv_i8((n, cin, h, w), w512[0], w512[1], w512[2], front=front, in_stat=zstat,
                      bn_scale=torch.ones(512, device=dev), bn_shift=torch.zeros(512, device=dev), act="relu")
