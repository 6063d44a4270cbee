"""Every epilogue cell of the int8 MFMA convolutions on the smallest shapes that reach it - the pieces the split 1x1, the
streaming 1x1, the dense 3x3 and the folded shortcut have in common (csrc/fq_mma.h holds some of them): the per-sample
statistic table (more samples in a tile than table slots, a tile boundary inside a sample, a ragged last tile), the per-channel constants (partial channel tile, padded slab,
with and without bias / BatchNorm), both input quantisers (unsigned online, signed offline), the three compile-time epilogues
(BN + ReLU / ReLU6 / none) and the run-time one (bias + BN + ReLU; nothing at all), and the output quantiser of a code output.
Output, per-sample statistic and `cur_out` are compared with == against the oracle of tests/test_gpu_parity.py (the shortcut:
against the two launches and the host twin, as tests/test_gpu_shortcut.py does).  The test is about the kernels, not about where
their text lives.

Cells of a code output that other files pin already and that are therefore NOT repeated here (split form, shape-based choice):
  tests/test_gpu_c16.py::test_pointwise_producer_writes_the_consumers_codes
      u8-out             ReLU6, consumer threshold 1.9 < 6  (the fold's min(hi, 6) takes hi)
      u8-out-relu6-thr9  ReLU6, consumer threshold 9 > 6    (... takes the 6)
      s8-out             no activation, signed consumer range (the general output quantiser)
      s8-out-relu        ReLU in front of a signed consumer range
  tests/test_gpu_c16.py::test_closing_pointwise_stores_the_trunk_twice      side_codes= (the second output), split and streaming
  tests/test_gpu_c16.py::test_dense3x3_with_codes_on_both_sides             3x3: ReLU, unsigned consumer range
  tests/test_gpu_sub2.py                                                    the subsampled output (with and without side_codes=)
What remains and is here: the split form's code output behind NO activation for an UNSIGNED consumer range (the five-instruction
output quantiser chosen by the range alone), and the 3x3's code output behind ReLU6 (threshold below and above 6; the 3x3 folds the
ReLU only), behind no activation (unsigned and signed range) and behind a ReLU in front of a signed range."""
import numpy as np
import pytest
import torch

from oracle import fq_oracle as O
from test_gpu_parity import N, T, _eq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu.torch_device


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


EPILOGUES = ["bn_relu", "bn_relu6", "bn_none", "bias_bn_relu", "plain"]     # three compile-time cells, the run-time one twice
INPUTS = ["online_u8", "offline_s8"]                                         # both forms of the sixteen-values quantiser


def _layer(ops, dev, case, ks, epi, inp, seed, residual=False):
    """Inputs of one call: (x, wt, kw for ops.*, okw for the oracle, the batch mean `cur_out` must hold)."""
    n, cin, cout, h, w = case
    rng = np.random.default_rng(sum(case) + seed)
    x = (rng.standard_normal((n, cin, h, w)) * 2).astype(np.float32)
    if inp == "online_u8":
        x = np.maximum(x, 0)
    wt = (rng.standard_normal((cout, cin, ks, ks)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    stat = O.absmax_per_sample(x)
    kw, okw = dict(in_stat=T(stat, dev), width=8), dict(width=8)
    if inp == "online_u8":
        kw.update(flags=0)
        okw.update(in_max=O.batch_mean(stat), signed=False)
    else:                                                 # (in_stat as well: `cur_out` reports the batch mean in every mode)
        thr = np.float32(2.3)
        kw.update(in_thr=T(np.float32([thr]), dev), flags=ops.act_flags(signed=True))
        okw.update(in_max=thr, signed=True)
    if "bn" in epi:                                       # (a tenth of the channels with a negative scale)
        sc = (rng.uniform(0.3, 1.5, cout) * np.where(rng.random(cout) < 0.1, -1, 1)).astype(np.float32)
        sh = rng.standard_normal(cout).astype(np.float32)
        kw.update(bn_scale=T(sc, dev), bn_shift=T(sh, dev))
        okw.update(bn_scale=sc, bn_shift=sh)
    if "bias" in epi:
        b = rng.standard_normal(cout).astype(np.float32)
        kw.update(bias=T(b, dev))
        okw.update(bias=b)
    act = "relu6" if "relu6" in epi else ("relu" if "relu" in epi else None)
    kw.update(act=act)
    okw.update(act=act)
    if residual:
        res = (rng.standard_normal((n, cout, h, w)) * 3).astype(np.float32)
        kw.update(residual=T(res, dev))
        okw.update(residual=res)
    return x, wt, kw, okw, np.float32([O.batch_mean(stat)])


# (n, cin, cout, h, w).  36 columns: the first 32-pixel tile holds 11 samples - more than the table's 8 slots, lanes of several
# samples in one wavefront -, the second is ragged; Cout 40: a partial channel tile; Cin 24: a padded slab.  5 x 7 planes: a tile
# boundary inside a sample.
PW_CASES = [("split", (12, 24, 40, 1, 3), False), ("split", (2, 64, 72, 5, 7), False),
            ("stream", (12, 32, 64, 1, 3), False), ("stream", (2, 64, 64, 5, 7), False), ("stream", (2, 64, 64, 5, 7), True)]


@pytest.mark.parametrize("form,case,residual", PW_CASES,
                         ids=["%s-%dx%d->%d@%dx%d" % ((f,) + c) + ("-res" if r else "") for f, c, r in PW_CASES])
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("inp", INPUTS)
def test_pointwise_epilogue_cells_vs_oracle(dev, ops, form, case, residual, epi, inp):
    n, cin, cout, h, w = case
    x, wt, kw, okw, mean = _layer(ops, dev, case, 1, epi, inp, 101, residual)
    codes, scales, rowsum = ops.weight_codes(T(wt, dev), cout, 8)
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.pwconv_i8(T(x, dev), codes, scales, rowsum, cur_out=cur, form=form, **kw)
    want = O.pwconv_i8(x, wt, cout, 8, **okw)
    _eq(N(y), want, "output")
    _eq(N(stat_out), O.absmax_per_sample(want), "statistic")
    _eq(N(cur), mean, "cur_out")


# The 3x3 takes Cin = 64, 128, 256 or 512 only: 64 instead of the 32 the pointwise shapes have.  (12, 64, 40, 2, 2): 48 columns,
# samples of 4 pixels - a block's table overflows, Cout 40 is a partial channel tile; 5 x 7 planes: a block boundary inside a sample.
C3_CASES = [(12, 64, 40, 2, 2), (2, 64, 64, 5, 7)]


@pytest.mark.parametrize("case", C3_CASES, ids=["%dx%d->%d@%dx%d" % c for c in C3_CASES])
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("inp", INPUTS)
def test_dense3x3_epilogue_cells_vs_oracle(dev, ops, case, epi, inp):
    n, cin, cout, h, w = case
    x, wt, kw, okw, mean = _layer(ops, dev, case, 3, epi, inp, 103)
    codes, scales, rowsum = ops.weight_codes_3x3(T(wt, dev), cout, 8)
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.conv3x3_i8(T(x, dev), codes, scales, rowsum, cur_out=cur, **kw)
    want = O.conv3x3_i8(x, wt, cout, 8, **okw)
    _eq(N(y), want, "output")
    _eq(N(stat_out), O.absmax_per_sample(want), "statistic")
    _eq(N(cur), mean, "cur_out")


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("inp", INPUTS)
def test_sliced_dense3x3_epilogue_cells_vs_oracle(dev, ops, epi, inp):
    """The three-slice form (a filter that is not on one integer grid) on the second shape: its own sum, the same cells."""
    case = C3_CASES[1]
    x, wt, kw, okw, mean = _layer(ops, dev, case, 3, epi, inp, 107)
    codes, pscale, rowsum = ops.weight_slices_3x3(T(wt, dev))
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.conv3x3_i8(T(x, dev), codes, pscale, rowsum, cur_out=cur, **kw)
    want = O.conv3x3_i8_sliced(x, wt, **okw)
    _eq(N(y), want, "output")
    _eq(N(stat_out), O.absmax_per_sample(want), "statistic")
    _eq(N(cur), mean, "cur_out")


@pytest.mark.parametrize("mode", ["online_u8_relu", "online_s8_none", "offline_u8_relu", "mixed_relu6_bias"])
def test_folded_shortcut_on_a_tile_of_many_samples(dev, ops, mode):
    """64 / 64 -> 256 is the smallest channel triple `pwconv_shortcut_supported` accepts; n = 12 on a 1 x 3 plane: the first tile
    holds 11 samples.  The check is tests/test_gpu_shortcut.py's: the two launches it replaces and the host twin, bit for bit."""
    from test_gpu_shortcut import test_folded_shortcut_equals_the_two_launches_and_the_host_twin as check
    assert ops.pwconv_shortcut_supported(64, 64, 256) and not ops.pwconv_shortcut_supported(32, 32, 128)
    check(dev, ops, (12, 64, 64, 256, 1, 3), mode)


def _codes_case(ops, dev, run, oracle, x, wt, kw, okw, mean, mode):
    """A code output == the oracle's codes of the oracle's fp32 output under the consumer's threshold; statistic and `cur_out`
    are those of the fp32 values."""
    signed_out = "s8" in mode
    thr_out = np.float32(9.0 if "thr9" in mode else 1.9)
    want = oracle(x, wt, **okw)
    lo = np.float32(-thr_out) if signed_out else np.float32(0)
    wantc = O.to_c16(O.ste_codes(want, O.act_scale(thr_out, signed_out, 8), thr_out, lo).astype(np.int64), 0 if signed_out else 128)
    cur = torch.zeros(1, device=dev)
    yc, stat_out = run(cur_out=cur, out_codes=dict(thr=T(np.float32([thr_out]), dev), width=8, flags=ops.act_flags(signed=signed_out)),
                       **kw)
    assert isinstance(yc, ops.Codes16) and yc.shape == want.shape
    _eq(N(yc.t), wantc, "C16 codes")
    _eq(N(stat_out), O.absmax_per_sample(want), "statistic")
    _eq(N(cur), mean, "cur_out")


def test_split_code_output_behind_no_activation_for_an_unsigned_range(dev, ops):
    case = (2, 64, 72, 5, 7)
    x, wt, kw, okw, mean = _layer(ops, dev, case, 1, "bn_none", "offline_s8", 109)
    cw = ops.weight_codes(T(wt, dev), 72, 8)
    _codes_case(ops, dev, lambda **k: ops.pwconv_i8(T(x, dev), *cw, form="split", **k),
                lambda x, wt, **k: O.pwconv_i8(x, wt, 72, 8, **k), x, wt, kw, okw, mean, "u8-out")


@pytest.mark.parametrize("mode", ["bn_relu6-u8-out", "bn_relu6-u8-out-thr9", "bn_none-u8-out", "bn_none-s8-out", "bn_relu-s8-out"])
def test_dense3x3_code_output_cells(dev, ops, mode):
    case = C3_CASES[1]
    x, wt, kw, okw, mean = _layer(ops, dev, case, 3, mode.split("-")[0], "offline_s8", 113)
    if "thr9" in mode:                                    # (values beyond 6, so that the 6 is what clips)
        okw["bn_scale"] = okw["bn_scale"] * np.float32(4)
        kw["bn_scale"] = T(okw["bn_scale"], dev)
    cw = ops.weight_codes_3x3(T(wt, dev), 64, 8)
    _codes_case(ops, dev, lambda **k: ops.conv3x3_i8(T(x, dev), *cw, **k),
                lambda x, wt, **k: O.conv3x3_i8(x, wt, 64, 8, **k), x, wt, kw, okw, mean, mode)
