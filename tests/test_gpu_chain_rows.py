"""GPU parity of the code buffer the fused launch keeps in statistic mode (fq_pwdw_fused with `mid_codes_out`: the codes of the
1x1 output it has just quantised for its stencil, handed to the statistic pass of the next pair), row by row:
  * every width among 28, 36, 56 and 112 that `fq_pwdw_fused_supported(..., stat_mode)` admits - 28 is the narrow plane whose
    single strip carries the stencil's left zero column inside it (`lz` of pwdw_plan), 36 two strips with the second anchored
    over the first, 56 MobileNet's, 112 four strips - with 64 and with 128 channels (one and two wavefronts per strip);
  * bands of two and of three rows on a plane of seven (2 + 2 + 2 + 1 and 3 + 3 + 1: the halo rows that two bands both quantise
    are written by both, and the last band is short).
Every byte of the buffer equals the code the host oracle's quantiser (oracle/fq_host.cpp) makes of the host twin's 1x1 output -
the buffer is planar, (N, C, H * W), so a byte of the stencil's zero columns written anywhere would land on a neighbouring
pixel's code and show here; the buffer and every other allocation lie between guard bands of poison, which stay untouched; the
per-sample maxima and `current_input_max` equal those of the storing launch; the launch reads no fp32 input (it is handed
NaN).  Both poison patterns."""
import numpy as np
import pytest
import torch

import poison
from test_gpu_pair_chain import _first_half, _fused, _host_mid_codes, _make, _operands
from test_gpu_pwdw import N, _eq, _t

pytestmark = pytest.mark.gpu

WIDTHS = (28, 36, 56, 112)
CHANNELS = ((32, 64), (64, 128))            # (cin, cmid): the depthwise layer has cmid channels
H = 7
BANDS = (2, 3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


_REFERENCE = {}


def _reference(case, dev, ops, monkeypatch):
    """(inputs, maxima of the storing launch, the host's codes and statistic): once per case, shared, never changed."""
    if case not in _REFERENCE:
        n, cin, cmid, cout, h, w = case
        k = _make(case, False)
        monkeypatch.delenv("FQ_PWDW_RB", raising=False)
        o = _operands(k, dev, ops, lambda a: _t(a, dev))
        xstat, xcodes, ystat = _first_half(k, o, dev, ops, lambda s, d: torch.full(s, 0x55, dtype=d, device=dev))
        cur2 = torch.zeros(1, device=dev)
        z, zstat = _fused(k, o, dev, ops, xstat, xcodes, ystat, cur2)
        assert np.isfinite(N(z)).all() and np.abs(N(z)).max() > 0
        _REFERENCE[case] = (k, dict(ystat=N(ystat), zstat=N(zstat), cur2=N(cur2)), _host_mid_codes(k, ops, dev))
    return _REFERENCE[case]


def _stat_mode(k, rb, pattern, dev, ops, monkeypatch):
    n, cin, cmid, cout, h, w = k["case"]
    monkeypatch.setenv("FQ_PWDW_RB", str(rb))
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        empty = lambda shape, dtype: proxy.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        o = _operands(k, dev, ops, lambda a: proxy.guarded(a, dev))
        xstat, xcodes, ystat = _first_half(k, o, dev, ops, empty)
        cur2 = torch.zeros(1, device=dev)
        ycodes = empty(ops.front_codes_shape((n, cmid, h, w)), torch.int8)
        nan_x = torch.full((n, cin, h, w), float("nan"), device=dev)
        none, zstat = _fused(k, o, dev, ops, xstat, xcodes, ystat, cur2, x=nan_x, store=False, mid_codes_out=ycodes)
        assert none is None
        torch.cuda.synchronize()
        proxy.guards_intact()
        _eq(N(o["x"]), k["x"], "the input after the launches")
        return dict(ystat=N(ystat), zstat=N(zstat), cur2=N(cur2), ycodes=N(ycodes))
    finally:
        proxy.release()
        ops._WS.clear()


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "%d->%d" % c)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_byte_of_the_code_buffer_in_bands_of_two_and_three_rows(dev, ops, monkeypatch, w, channels, pattern):
    cin, cmid = channels
    case = (3, cin, cmid, cmid, H, w)
    if not ops.pwdw_chain_supported((3, cin, H, w), cmid):
        # a width the launch does not admit with these channels is refused with a message, nothing is launched
        k = _make(case, False)
        o = _operands(k, dev, ops, lambda a: _t(a, dev))
        xstat, xcodes, ystat = _first_half(k, o, dev, ops, lambda s, d: torch.zeros(s, dtype=d, device=dev))
        ycodes = torch.full((3, cmid, H * w), 0x55, dtype=torch.int8, device=dev)
        with pytest.raises(ValueError, match="does not take"):
            _fused(k, o, dev, ops, xstat, xcodes, ystat, torch.zeros(1, device=dev), store=False, mid_codes_out=ycodes)
        torch.cuda.synchronize()
        assert (ycodes == 0x55).all()
        return
    k, want, host = _reference(case, dev, ops, monkeypatch)
    assert (host[0].view(np.uint8) > 127).any() and (host[0] == 0).any()
    for rb in BANDS:
        got = _stat_mode(k, rb, pattern, dev, ops, monkeypatch)
        what = ", %d rows per band" % rb
        _eq(got["ystat"], host[1], "statistic of the 1x1 output vs the host twin" + what)
        _eq(got["ycodes"], host[0], "mid_codes_out vs the host oracle's quantiser (every byte of the buffer)" + what)
        _eq(got["zstat"], want["zstat"], "per-sample maxima of the depthwise output: statistic mode vs the storing launch" + what)
        _eq(got["cur2"], want["cur2"], "current_input_max of the depthwise block" + what)


def test_every_width_is_admitted(dev, ops):
    """The four widths are taken with 64 channels, so that none of the cases above is the refusal alone."""
    assert [w for w in WIDTHS if ops.pwdw_chain_supported((3, 32, H, w), 64)] == list(WIDTHS)
