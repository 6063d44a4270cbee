"""The quantiser of the depthwise statistic pass (fq_dwconv3x3 without y, `x_codes_out`) on every rounding tie: under a stored
threshold t the pass divides by d = fp32(fp32(t / 255) + 1e-10), and its input here is (k + 0.5) d for every k of 0 .. 255,
each nudged by -2 .. +2 ulp - the values at which a quotient that is one ulp off, or a rounding that is not half-away, gives
another code.  Thresholds: three ordinary ones, one whose divisor has an all-ones significand (the divisor make_fast_quot of the
recompute kernels declines) and one at the scale of tests/regimes.py's `eps_scale` (the divisor is mostly epsilon).  The pass
divides through the fp64 reciprocal at every one of them - the fp32 quotient with its correction step was measured in this pass
and bought nothing - and the test holds whichever form computes the codes: the codes the pass keeps and the
per-sample maxima of its output are bit-equal to the host twin's (oracle/fq_host.cpp).

Before anything is compared the ORACLE's codes are checked to contain every code there is: 0 .. 255 - except under the
`eps_scale` threshold, where the clip bound itself divides to about 180 (that is what the regime is: regimes.check wants the
largest code between a quarter and three quarters of the levels), so there every code from 0 to the bound's own is wanted."""
import numpy as np
import pytest
import torch

import poison
import regimes as R
from test_gpu_pwdw import N, _eq, _t

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(2, 16, 8, 16), (2, 32, 12, 28)]
THRESHOLDS = {"2.5": F32(2.5), "6": F32(6.0), "0.731": F32(0.731), "allones_divisor": None, "eps_scale": None}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


def _threshold(name):
    if name == "allones_divisor":
        t = R.allones_threshold(False)
        assert R.has_allones_significand(R.divisor(t, False))
        return F32(t)
    if name == "eps_scale":
        return F32(F32(8.0) * R.eps_factor(False))
    t = THRESHOLDS[name]
    assert not R.has_allones_significand(R.divisor(t, False))
    return t


def _ties(thr):
    """(k + 0.5) d, k = 0 .. 255, each with its neighbours two ulp down to two ulp up: 1280 fp32 values."""
    d = np.float64(R.divisor(thr, False))
    base = ((np.arange(256, dtype=np.float64) + 0.5) * d).astype(F32)
    assert (base > 0).all() and np.isfinite(base).all()
    bits = base.view(np.uint32).astype(np.int64)[:, None] + np.arange(-2, 3, dtype=np.int64)[None, :]
    return bits.astype(np.uint32).view(F32).reshape(-1)


def _case(shape, name):
    n, c, h, w = shape
    thr = _threshold(name)
    ties = _ties(thr)
    rng = np.random.default_rng(c + w)
    numel = n * c * h * w
    assert numel >= 2 * ties.size
    x = np.tile(ties, numel // ties.size + 1)[:numel]
    rng.shuffle(x)
    k = dict(x=x.reshape(shape).astype(F32), thr=thr)
    k["w"] = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(F32)
    k["bn"] = ((0.5 + rng.random(c)).astype(F32), (rng.standard_normal(c) * 0.1).astype(F32) * thr)
    return k


def _host(k):
    from oracle import host as H
    codes = H.fake_quant_offline(k["x"], k["thr"], 8, H.act_flags(signed=False), want_codes=True)[2]
    _, stat = H.dwconv3x3(k["x"], k["w"], None, stride=1, in_max=k["thr"], signed=False, width=8, bn_scale=k["bn"][0],
                          bn_shift=k["bn"][1], act="relu", want_stat=True)
    return codes, stat


@pytest.mark.parametrize("name", list(THRESHOLDS))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%dx%d" % s for s in SHAPES])
def test_codes_and_maximum_on_every_tie(dev, ops, monkeypatch, shape, name):
    n, c, h, w = shape
    k = _case(shape, name)
    codes, stat = _host(k)
    # from the oracle's codes, on the CPU: every code occurs
    from oracle import host as H
    top = int(H.fake_quant_offline(np.full((1, 1), k["thr"], F32), k["thr"], 8, H.act_flags(signed=False), want_codes=True)[2][0, 0])
    if name == "eps_scale":
        assert 0.25 * 255 <= top <= 0.75 * 255, top
    else:
        assert top == 255
    assert sorted(set(codes.reshape(-1).tolist())) == list(range(top + 1))
    want_codes = (codes.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(n, c, h * w)

    proxy = poison.Proxy(0xFF)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        x = proxy.guarded(k["x"], dev)
        ycodes = proxy.empty(ops.front_codes_shape(shape), dtype=torch.int8, device=dev)
        cur = torch.zeros(1, device=dev)
        none, gstat = ops.dwconv3x3(x, _t(k["w"], dev), None, stride=1, in_thr=_t(np.asarray([k["thr"]], F32), dev), width=8,
                                    flags=ops.act_flags(signed=False), cur_out=cur, bn_scale=_t(k["bn"][0], dev),
                                    bn_shift=_t(k["bn"][1], dev), act="relu", store=False, x_codes_out=ycodes)
        assert none is None
        torch.cuda.synchronize()
        proxy.guards_intact()
        _eq(N(ycodes), want_codes, "codes of the depthwise input vs the host twin")
        _eq(N(gstat), stat, "per-sample maxima of the depthwise output vs the host twin")
        assert stat.max() > 0
    finally:
        proxy.release()
        ops._WS.clear()
