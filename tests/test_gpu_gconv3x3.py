"""fq_gconv3x3_i8: the grouped 3x3 convolution (stride 1, padding 1, 4 .. 32 channels per group) on int8 codes, against an fp64
convolution of the two fake-quantised tensors and, bit for bit, against the dense oracle on the zero-expanded filter."""
import numpy as np
import pytest
import torch

import poison
import regimes as R
from oracle import fq_oracle as O

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


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


CASES = [  # (n, C, groups, h, w)
    (2, 32, 8, 5, 6),        # cg 4, one slab
    (3, 64, 8, 7, 7),        # cg 8, blocks that span samples
    (2, 96, 6, 9, 11),       # cg 16, slab count not a multiple of the slabs per workgroup
    (1, 128, 4, 14, 14),     # cg 32
    (9, 32, 8, 3, 3),        # many samples per block
    (1, 64, 16, 1, 50),      # a one-row plane wider than a pixel tile
    (2, 32, 8, 28, 28)]      # a workgroup walks several blocks, both panels in use
MODES = ["online_u8_bn_relu", "offline_s8_channel_w4", "online_s8_bias", "offline_s8_group"]


def _dense(wt, groups):
    """(C, C / groups, 3, 3) -> the block-diagonal dense filter (C, C, 3, 3)"""
    c, cg = wt.shape[:2]
    wd = np.zeros((c, c, 3, 3), np.float32)
    for co in range(c):
        g = co // cg
        wd[co, g * cg:(g + 1) * cg] = wt[co]
    return wd


def _input_side(regime, rthr, x, stored, both=False):
    """(launch keywords as host arrays, the threshold the launch quantises with).  `rthr` is what `R.apply` returned: the driver's
    stored threshold, the regime's own in its place, the batch mean a regime without one leaves stored - or None, the launch works
    online.  Routed as `_regime_threshold` of tests/test_gpu_parity.py routes it: a regime's own threshold turns an online launch
    into a stored one - but for `boundaries`, which plants its threshold as every sample's maximum: that launch stays online and
    divides by the same d.  `both`: a stored launch that is handed the statistic too (it only feeds cur_out)."""
    stat = O.absmax_per_sample(x)
    if rthr is not None and (stored or regime != "boundaries"):
        kw = dict(in_thr=np.float32([rthr]))
        if both:
            kw["in_stat"] = stat
        return kw, np.float32(rthr)
    in_max = O.batch_mean(stat)
    assert rthr is None or in_max == rthr
    return dict(in_stat=stat), in_max


def _up(kw, dev, T):
    return {k: (T(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def _fp64(xq, wq, groups, stride, bias=None):
    """plain and high-precision: the fp64 grouped convolution of the two fake-quantised tensors"""
    ref = torch.nn.functional.conv2d(torch.from_numpy(xq.astype(np.float64)), torch.from_numpy(wq.astype(np.float64)),
                                     stride=stride, padding=1, groups=groups).numpy()
    return ref if bias is None else ref + bias.astype(np.float64).reshape(1, -1, 1, 1)


def _make(case, mode, regime=None, width=8, stride=1):
    """What needs no device, for either stride: the data as drawn, turned into `regime` (tests/regimes.py) and checked against its
    condition, the launch keywords as host arrays and both references at `width`."""
    n, c, groups, h, w = case
    cg = c // groups
    rng = np.random.default_rng(sum(case) + 11)
    signed = "s8" in mode
    x = (rng.standard_normal((n, c, h, w)) * 2).astype(np.float32)
    if not signed:
        x = np.maximum(x, 0)
    wt = (rng.standard_normal((c, cg, 3, 3)) * rng.uniform(0.05, 1.0, (c, 1, 1, 1))).astype(np.float32)
    wt_width = 4 if "w4" in mode else 8
    rps = 1 if "channel" in mode else (cg if "group" in mode else c)
    stored = mode.startswith("offline")
    assert signed or not stored                              # (the modes under a stored threshold are the signed ones)
    x, wt, rthr = R.apply(regime, x, signed, wt, rps, np.float32(2.3) if stored else None, width=width)
    kw, in_max = _input_side(regime, rthr, x, stored)
    R.check(regime, x, in_max, signed, w=wt, rps=rps, wt_width=wt_width, taps=9, width=width)
    okw = dict(in_max=in_max, signed=signed, width=width)
    if "bn_relu" in mode:
        sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
        sh = rng.standard_normal(c).astype(np.float32)
        kw.update(bn_scale=sc, bn_shift=sh, act="relu")
        okw.update(bn_scale=sc, bn_shift=sh, act="relu")
    if "bias" in mode:
        b = rng.standard_normal(c).astype(np.float32)
        kw.update(bias=b)
        okw.update(bias=b)
    k = dict(case=case, cg=cg, signed=signed, x=x, wt=wt, rps=rps, wt_width=wt_width, width=width, kw=kw, okw=okw, ref=None)
    # the project's bar: the dense oracle on the zero-expanded filter (zeros change no scale), bit for bit; a stride subsamples it
    k["want"] = np.ascontiguousarray(O.conv3x3_i8(x, _dense(wt, groups), rps, wt_width, **okw)[:, :, ::stride, ::stride])
    assert np.isfinite(k["want"]).all()
    if "bn_relu" not in mode:
        # (fp32 vs fp64 summation noise: the bound is scale-free, it holds under every regime and at every width)
        wc, ws = O.weight_codes(wt, rps, wt_width)
        wq = (wc.astype(np.float32) * ws[:, None]).astype(np.float32).reshape(wt.shape)
        xq = O.ste_forward(x, O.act_scale(in_max, signed, width), in_max, -in_max if signed else 0.0)
        k["ref"] = _fp64(xq, wq, groups, stride, okw.get("bias"))
    return k


@pytest.mark.parametrize("case", CASES, ids=["%dx%dg%d@%dx%d" % c for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_gconv3x3_i8(dev, ops, case, mode, regime=None, width=8):
    """`regime`: a value regime of tests/regimes.py, applied to the data as drawn (tests/test_gpu_value_regimes.py).
    `width`: the activation width of the launch and of both references (tests/test_gpu_act_widths.py)."""
    k = _make(case, mode, regime, width)
    groups = case[2]
    codes, scales, rowsum = ops.weight_codes_g3x3(T(k["wt"], dev), groups, k["rps"], k["wt_width"])
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.gconv3x3_i8(T(k["x"], dev), codes, scales, rowsum, groups, cur_out=cur, width=width,
                                  flags=ops.act_flags(signed=k["signed"]), **_up(k["kw"], dev, T))
    launch = ops.last_launch()
    got = y.cpu().numpy()
    assert launch[0] == "gconv3x3" and launch[4] == k["cg"], launch
    if case == CASES[-1]:
        assert launch[3] >= 2, "this case is here for a band of several blocks: %s" % (launch,)
    np.testing.assert_array_equal(got, k["want"])
    np.testing.assert_array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(got))
    if "in_stat" in k["kw"]:
        np.testing.assert_array_equal(cur.cpu().numpy(), np.float32([k["okw"]["in_max"]]))
    if k["ref"] is not None:
        np.testing.assert_allclose(got, k["ref"], rtol=2e-5, atol=2e-5 * np.abs(k["ref"]).max())


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
def test_gconv3x3_i8_under_poison(dev, ops, monkeypatch, pattern):
    """As tests/test_gpu_poison.py runs its families: what `ops` allocates is the pattern inside guard bands, the inputs are guarded -
    the kernel writes every output it owns and nothing beside them."""
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setitem(globals(), "T", lambda a, d: proxy.guarded(a, d))
    for case, mode in ((CASES[2], MODES[0]), (CASES[5], MODES[3]), (CASES[6], MODES[2])):
        ops._WS.clear()
        test_gconv3x3_i8(dev, ops, case, mode)
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records
        proxy.release()
    ops._WS.clear()


@pytest.mark.parametrize("c,groups", [(96, 32), (48, 4), (64, 1)], ids=["cg3", "C48", "groups1"])
def test_gconv3x3_refuses_other_shapes(dev, ops, c, groups):
    from quantization.mxnet_amd._lib import FakeQuantError
    assert not ops.gconv3x3_supported(c, c, groups)
    x = torch.ones((1, c, 4, 4), device=dev)
    rows_pad = (c + 63) // 64 * 64
    codes = torch.zeros((2 * rows_pad * 320,), dtype=torch.int8, device=dev)[:rows_pad * 320].view(rows_pad, 320)
    with pytest.raises(FakeQuantError, match="fq_gconv3x3_i8"):
        ops.gconv3x3_i8(x, codes, torch.ones(c, device=dev), torch.zeros(c, dtype=torch.int32, device=dev), groups,
                        in_thr=torch.ones(1, device=dev))
