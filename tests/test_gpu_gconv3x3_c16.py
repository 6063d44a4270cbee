"""fq_gconv3x3_i8_c16: the grouped 3x3 convolution with C16 code tensors on either side - bit for bit the dense oracle on the
zero-expanded filter followed by the consumer's quantiser, and within one code step of an fp64 grouped convolution."""
import functools

import numpy as np
import pytest
import torch

import poison
import regimes as R
from oracle import fq_oracle as O
from test_gpu_gconv3x3 import CASES, T, _dense, dev, ops  # noqa: F401  (the seven shapes of the fp32 form, its fixtures)

pytestmark = pytest.mark.gpu

IO = ["codes-codes", "codes-fp32", "fp32-codes"]
QUANT = {  # name: (input signed, epilogue, output width, output signed)
    "u8_bn_relu_u8": (False, "bn_relu", 8, False),
    "s8_bias_s8": (True, "bias", 8, True),
    "u8_bn_relu_u4": (False, "bn_relu", 4, False)}
IN_THR = np.float32(2.3)


@functools.lru_cache(maxsize=None)
def _expected(case, quant, regime=None, width=8, out_width=None, stride=1):
    """Inputs and both references of one (shape, quantiser, regime, widths) cell, computed once for its three io forms and with no
    device; `stride` 2: the cell of tests/test_gpu_gconv3x3_s2_c16.py.  `out_width` None: the quantiser's own."""
    n, c, groups, h, w = case
    cg = c // groups
    signed, epi, quant_width, out_signed = QUANT[quant]
    out_width = quant_width if out_width is None else out_width
    rng = np.random.default_rng(sum(case) + (23 if stride == 1 else 29))
    x = (rng.standard_normal((n, c, h, w)) * 2).astype(np.float32)
    if not signed:
        x = np.maximum(x, 0)
    wt = (rng.standard_normal((c, cg, 3, 3)) * rng.uniform(0.05, 1.0, (c, 1, 1, 1))).astype(np.float32)
    rps = 1 if signed else cg
    x, wt, thr = R.stored(regime, x, signed, wt, rps, IN_THR, width=width)
    thr = np.float32(thr)
    R.check(regime, x, thr, signed, w=wt, rps=rps, taps=9, width=width)
    e = dict(x=x, wt=wt, rps=rps, thr=thr, out_width=out_width, okw=dict(in_max=thr, signed=signed, width=width))
    if epi == "bn_relu":
        e["sc"], e["sh"] = rng.uniform(0.3, 1.5, c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        e["okw"].update(bn_scale=e["sc"], bn_shift=e["sh"], act="relu")
    else:
        e["b"] = rng.standard_normal(c).astype(np.float32)
        e["okw"].update(bias=e["b"])
    lo_in = -thr if signed else np.float32(0)
    e["cx"] = O.ste_codes(x, O.act_scale(thr, signed, width), thr, lo_in)
    # the project's bar: the dense oracle on the zero-expanded filter (a stride subsamples it), then the consumer's quantiser
    want = e["want"] = np.ascontiguousarray(O.conv3x3_i8(x, _dense(wt, groups), rps, 8, **e["okw"])[:, :, ::stride, ::stride])
    assert np.isfinite(want).all()
    # (the 0.6 of the output's maximum holds for every cell of the width tables: tests/test_act_widths_host.py checks the cap below
    # on the oracle's own codes)
    thr2 = e["thr2"] = np.float32(R.output_threshold(regime, want, out_signed, np.float32(0.6) * np.abs(want).max(), width=out_width))
    R.check_output(regime, want, thr2, out_signed, width=out_width)
    lo2 = -thr2 if out_signed else np.float32(0)
    s2 = O.act_scale(thr2, out_signed, out_width)
    e["want_codes"] = O.ste_codes(want, s2, thr2, lo2)
    # plain and high-precision: the fp64 grouped convolution of the two fake-quantised tensors, the epilogue in fp64
    wc, ws = O.weight_codes(wt, rps, 8)
    wq = (wc.astype(np.float32) * ws[:, None]).astype(np.float32).reshape(wt.shape)
    xq = (e["cx"] * O.act_scale(thr, signed, width)).astype(np.float32)
    ref = torch.nn.functional.conv2d(torch.from_numpy(xq.astype(np.float64)), torch.from_numpy(wq.astype(np.float64)),
                                     stride=stride, padding=1, groups=groups).numpy()
    if epi == "bn_relu":
        ref = np.maximum(ref * e["sc"].astype(np.float64).reshape(1, -1, 1, 1) + e["sh"].astype(np.float64).reshape(1, -1, 1, 1), 0)
    else:
        ref = ref + e["b"].astype(np.float64).reshape(1, -1, 1, 1)
    e["ref"] = ref
    q = np.clip(ref, float(lo2), float(thr2)) / (float(s2) + 1e-10)
    e["ref_codes"] = np.sign(q) * np.floor(np.abs(q) + 0.5)
    return e


def _codes_within_cap(codes, ref_codes):
    """The condition on a code output: no code more than one step off the fp64 reference's, at most 1 in 1000 off at all.  It is
    one about Gaussian data, at every width; a regime of tests/regimes.py sits on rounding ties by construction - there the
    bit-for-bit oracle is the bar and this is not asked."""
    diff = np.abs(codes - ref_codes)
    print("codes off the fp64 reference: %d of %d, largest step %d" % ((diff != 0).sum(), diff.size, diff.max()))
    return diff.max() <= 1 and (diff != 0).sum() * 1000 <= diff.size


def _launch_args(e, quant, io, dev, ops, T):
    """-> (x as the io form takes it, launch keywords, in16, out16) of either stride's C16 op"""
    signed, epi, _, out_signed = QUANT[quant]
    in16, out16 = io.startswith("codes"), io.endswith("codes")
    width = e["okw"]["width"]
    thr_t = T(np.float32([e["thr"]]), dev)
    flags = ops.act_flags(signed=signed)
    kw = dict(in_thr=thr_t, width=width, flags=flags)
    if signed:                                           # (offline with the statistic: it only feeds cur_out)
        kw.update(in_stat=T(O.absmax_per_sample(e["x"]), dev))
    if epi == "bn_relu":
        kw.update(bn_scale=T(e["sc"], dev), bn_shift=T(e["sh"], dev), act="relu")
    else:
        kw.update(bias=T(e["b"], dev))
    if out16:
        kw.update(out_codes=dict(thr=T(np.float32([e["thr2"]]), dev), width=e["out_width"], flags=ops.act_flags(signed=out_signed)))
    xa = ops.Codes16(T(O.to_c16(e["cx"].astype(np.int64), 0 if signed else 128), dev), e["x"].shape, thr_t, width, flags) if in16 \
        else T(e["x"], dev)
    return xa, kw, in16, out16


def _compare(e, quant, regime, y, stat_out, cur, out16, ops):
    """What either stride's launch is held to."""
    signed, _, _, out_signed = QUANT[quant]
    c = e["want"].shape[1]
    np.testing.assert_array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(e["want"]))
    if signed:
        np.testing.assert_array_equal(cur.cpu().numpy(), np.float32([O.batch_mean(O.absmax_per_sample(e["x"]))]))
    if not out16:
        got = y.cpu().numpy()
        np.testing.assert_array_equal(got, e["want"])
        np.testing.assert_allclose(got, e["ref"], rtol=2e-5, atol=2e-5 * np.abs(e["ref"]).max())
        return
    assert isinstance(y, ops.Codes16) and y.shape == e["want"].shape and y.width == e["out_width"]
    zoff = 0 if out_signed else 128
    got = y.t.cpu().numpy()
    assert np.array_equal(got, O.to_c16(e["want_codes"].astype(np.int64), zoff)), "codes of the grouped output"
    if regime is None:
        assert _codes_within_cap(O.from_c16(got, c, *e["want"].shape[2:], zoff), e["ref_codes"])


@pytest.mark.parametrize("case", CASES, ids=["%dx%dg%d@%dx%d" % c for c in CASES])
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("quant", list(QUANT))
def test_gconv3x3_i8_c16(dev, ops, case, io, quant, regime=None, width=8, out_width=None):
    """`regime`, `width`, `out_width`: a value regime of tests/regimes.py and the widths of the two quantisers
    (tests/test_gpu_value_regimes.py, tests/test_gpu_act_widths.py)."""
    n, c, groups, h, w = case
    e = _expected(case, quant, regime, width, out_width)
    codes, scales, rowsum = ops.weight_codes_g3x3(T(e["wt"], dev), groups, e["rps"], 8)
    xa, kw, in16, out16 = _launch_args(e, quant, io, dev, ops, T)
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.gconv3x3_i8(xa, codes, scales, rowsum, groups, cur_out=cur, **kw)
    launch = ops.last_launch()
    assert launch[0] == "gconv3x3c16" and launch[4:] == (c // groups, int(in16), int(out16)), launch
    if case == CASES[-1]:
        assert launch[3] >= 2, "this case is here for a band of several blocks: %s" % (launch,)
    _compare(e, quant, regime, y, stat_out, cur, out16, ops)


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
def test_gconv3x3_i8_c16_under_poison(dev, ops, monkeypatch, pattern):
    """As tests/test_gpu_gconv3x3.py: what `ops` allocates is the pattern inside guard bands, the inputs are guarded - every byte
    of a C16 output is written (the comparison above covers all of it) and nothing beside it."""
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setitem(globals(), "T", lambda a, d: proxy.guarded(a, d))
    for case, io, quant in ((CASES[2], IO[0], "u8_bn_relu_u8"), (CASES[5], IO[2], "s8_bias_s8"), (CASES[6], IO[1], "u8_bn_relu_u4")):
        ops._WS.clear()
        test_gconv3x3_i8_c16(dev, ops, case, io, quant)
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records
        proxy.release()
    ops._WS.clear()


@pytest.mark.parametrize("what", ["stride2_codes_in", "stride2_codes_out", "other_threshold", "too_wide"])
def test_gconv3x3_i8_c16_refuses(dev, ops, what):
    from quantization.mxnet_amd._lib import FakeQuantError
    w = ops.GCONV3X3_C16_MAX_W + 1 if what == "too_wide" else 6
    thr = torch.ones(1, device=dev)
    xc = ops.Codes16(torch.zeros((1, 2, 4 * w, 16), dtype=torch.int8, device=dev), (1, 32, 4, w),
                     torch.ones(1, device=dev) if what == "other_threshold" else thr, 8, 0)
    codes, scales, rowsum = ops.weight_codes_g3x3(torch.ones((32, 4, 3, 3), device=dev), 8, 4)
    kw = dict(in_thr=thr, stride=2 if what.startswith("stride2") else 1)
    if what == "stride2_codes_out":
        xc, kw["out_codes"] = torch.zeros((1, 32, 4, w), device=dev), dict(thr=thr)
    with pytest.raises(FakeQuantError, match="fq_gconv3x3"):
        ops.gconv3x3_i8(xc, codes, scales, rowsum, 8, **kw)
