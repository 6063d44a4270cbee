"""fq_gconv3x3_s2_i8_c16: the stride-2 grouped 3x3 convolution with C16 code tensors on either side - bit for bit the subsampled
dense oracle on the zero-expanded filter followed by the consumer's quantiser, and within one code step of an fp64 strided grouped
convolution."""
import numpy as np
import pytest
import torch

import poison
import test_gpu_gconv3x3_c16 as S1
from oracle import fq_oracle as O
from test_gpu_gconv3x3 import T, dev, ops  # noqa: F401  (fixtures and helpers of the fp32 form)
from test_gpu_gconv3x3_c16 import IN_THR, IO, QUANT     # the stride-1 file's io forms and quantiser cells
from test_gpu_gconv3x3_s2 import CASES                  # the eleven shapes of the fp32 stride-2 form

pytestmark = pytest.mark.gpu


def _expected(case, quant, regime=None, width=8, out_width=None):
    """Inputs and both references of one (shape, quantiser, regime, widths) cell, computed once for its three io forms: the
    stride-1 file's, with this file's seed, subsampled."""
    return S1._expected(case, quant, regime, width, out_width, stride=2)


@pytest.mark.parametrize("case", CASES, ids=["%dx%dg%d@%dx%d" % c for c in CASES])
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("quant", list(QUANT))
def test_gconv3x3_s2_c16(dev, ops, case, io, quant, regime=None, width=8, out_width=None):
    """`regime`, `width`, `out_width`: as in the stride-1 file."""
    n, c, groups, h, w = case
    e = _expected(case, quant, regime, width, out_width)
    codes, scales, rowsum = ops.weight_codes_g3x3(T(e["wt"], dev), groups, e["rps"], 8)
    xa, kw, in16, out16 = S1._launch_args(e, quant, io, dev, ops, T)
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.gconv3x3_s2_c16(xa, codes, scales, rowsum, groups, cur_out=cur, **kw)
    launch = ops.last_launch()                           # (family, WC, PT, NB, CG, IN16, OUT16, NW)
    assert launch[0] == "gconv3x3s2c16" and launch[4:] == (c // groups, int(in16), int(out16), 4), launch
    assert launch[1:3] == ((1, 4) if c == 32 else (2, 2)), launch
    if h == 28:
        assert launch[3] >= 2 and n * 196 > 32 * launch[2], "this case is here for a band of several blocks: %s" % (launch,)
    S1._compare(e, quant, regime, y, stat_out, cur, out16, ops)


def test_gconv3x3_s2_c16_larger_blocks(dev, ops, monkeypatch):
    """The two candidates of DESIGN 3.11 that the default does not take: four pixel tiles per block under four or eight wavefronts."""
    e = _expected(CASES[10], "u8_bn_relu_u8")
    want = O.to_c16(e["want_codes"].astype(np.int64), 128)
    thr_t = T(np.float32([IN_THR]), dev)
    codes, scales, rowsum = ops.weight_codes_g3x3(T(e["wt"], dev), 8, e["rps"], 8)
    xa = ops.Codes16(T(O.to_c16(e["cx"].astype(np.int64), 128), dev), e["x"].shape, thr_t, 8, 0)
    for cfg, nw in (("44", 4), ("48", 8)):
        monkeypatch.setenv("FQ_GCS216_CFG", cfg)
        y, stat_out = ops.gconv3x3_s2_c16(xa, codes, scales, rowsum, 8, in_thr=thr_t, bn_scale=T(e["sc"], dev), bn_shift=T(e["sh"], dev),
                                          act="relu", out_codes=dict(thr=T(np.float32([e["thr2"]]), dev)))
        assert ops.last_launch()[1:3] == (2, 4) and ops.last_launch()[7] == nw, ops.last_launch()
        assert np.array_equal(y.t.cpu().numpy(), want), cfg
        np.testing.assert_array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(e["want"]))


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
def test_gconv3x3_s2_c16_under_poison(dev, ops, monkeypatch, pattern):
    """As tests/test_gpu_gconv3x3_c16.py: what `ops` allocates is the pattern inside guard bands, the inputs are guarded - every
    byte of a C16 output is written (the comparison above covers all of it) and nothing beside it."""
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setitem(globals(), "T", lambda a, d: proxy.guarded(a, d))
    for case, io, quant in ((CASES[2], IO[0], "u8_bn_relu_u8"), (CASES[5], IO[2], "s8_bias_s8"), (CASES[10], IO[1], "u8_bn_relu_u4")):
        ops._WS.clear()
        test_gconv3x3_s2_c16(dev, ops, case, io, quant)
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records
        proxy.release()
    ops._WS.clear()


@pytest.mark.parametrize("what", ["neither_side", "other_threshold", "too_wide"])
def test_gconv3x3_s2_c16_refuses(dev, ops, what):
    from quantization.mxnet_amd._lib import FakeQuantError
    w = ops.GCONV3X3_S2_C16_MAX_W + 1 if what == "too_wide" else 6
    thr = torch.ones(1, device=dev)
    xc = ops.Codes16(torch.zeros((1, 2, 4 * w, 16), dtype=torch.int8, device=dev), (1, 32, 4, w),
                     torch.ones(1, device=dev) if what == "other_threshold" else thr, 8, 0)
    if what == "neither_side":
        xc = torch.zeros((1, 32, 4, w), device=dev)
    codes, scales, rowsum = ops.weight_codes_g3x3(torch.ones((32, 4, 3, 3), device=dev), 8, 4)
    with pytest.raises(FakeQuantError, match="fq_gconv3x3_s2_i8_c16"):
        ops.gconv3x3_s2_c16(xc, codes, scales, rowsum, 8, in_thr=thr)
