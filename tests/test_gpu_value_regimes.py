"""Every int8 kernel family under degenerate and saturated VALUES (tests/regimes.py).

The other GPU tests are dense in shapes and thin in values: Gaussian data under a threshold near its maximum.  The kernels
branch on the values - once per launch, wave-uniformly -, so such a test always takes the same side of `fq_nonneg`, of
`q2.denom > 0`, of `make_fast_quot(d).ok`, never has an integer sum beyond 2^24 (where the epilogue's int32 -> fp32 conversion
rounds) and never a scale near the epsilon of ste_func.py:39-41.  Here the same case drivers and the same bit-for-bit
assertions run with their data turned into a named regime; each regime's condition is asserted from the oracle's codes
before anything is compared.  `CASES` is the table: family -> [(driver, arguments, the regimes that apply to it)];
tests/test_value_regimes_host.py checks on the CPU that every family has a case under every regime that applies to it.

No tolerance is added: a driver asserts what its own test asserts; only its checks about Gaussian data are skipped."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import regimes as R
import test_gpu_c16 as C16
import test_gpu_front_dw as FRONT
import test_gpu_gap as GAP
import test_gpu_pair_chain as CHAIN
import test_gpu_parity as P
import test_gpu_poison as POISON
import test_gpu_pwdw as PWDW
import test_gpu_qconv as QC
import test_gpu_shortcut as SC
import test_gpu_sub2 as SUB2
from oracle import fq_oracle as O
from oracle import host as H

pytestmark = pytest.mark.gpu

_eq, N, T = P._eq, P.N, P.T

IN = R.INPUT
# regimes without a threshold of their own - and `boundaries`, whose planted per-sample maxima make the online statistic its threshold
ONLINE = ("zero", "zero_sample", "eps_scale", "tiny", "subnormal", "huge", "boundaries")
NO_QUANTISER = ("zero", "zero_sample", "tiny", "subnormal", "huge")             # a layer that takes fp32 as it is
OUT = R.OUTPUT

Case = collections.namedtuple("Case", "driver kwargs regimes")


def case(driver, regimes, **kwargs):
    return Case(driver, kwargs, tuple(regimes))


# ---- drivers of what has no driver of its own ------------------------------------------------------------------------------
def took_fast_path(dev, d):
    """`make_fast_quot(d).ok` as the recompute kernels decide it (fq_debug_fast_quotient)."""
    from quantization.mxnet_amd import _lib
    c = torch.ones(4, device=dev)
    out = torch.empty_like(c)
    took = torch.full((1,), -1, dtype=torch.int32, device=dev)
    dt = torch.from_numpy(np.float32([d])).to(dev)
    _lib.check_call(_lib.LIB.fq_debug_fast_quotient(ctypes.c_void_p(c.data_ptr()), 4, ctypes.c_void_p(dt.data_ptr()),
                                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(took.data_ptr()),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return int(N(took)[0])


def _pair(dev, ops, case, mode, regime, allones=("in", "mid"), width=8, mid_width=8):
    """`pwconv_i8_stat` + `pwdw_fused` without and with the code buffer (the driver of the poisoned runs).  The fused kernel
    reads at most 256 input channels: 256 * 255 * 127 < 2^24, no shape of it reaches the large sums.  Under `allones_divisor`
    the launch takes the general body for exactly one known cause per named threshold: that divisor - and no other - is one
    `make_fast_quot` declines, both clip ranges start at 0."""
    POISON._pair(dev, ops, case, mode, regime=regime, allones=allones, width=width, mid_width=mid_width)
    if regime == "allones_divisor":
        k = PWDW._make(case, mode, dev, ops, regime=regime, allones=allones, width=width, mid_width=mid_width)
        assert not k["signed"] and k["offline"]
        for name, thr, wd in (("in", k["thr1"], width), ("mid", k["thr2"], mid_width)):
            d = R.divisor(thr, False, wd)
            assert R.has_allones_significand(d) == (name in allones)
            assert took_fast_path(dev, d) == (0 if name in allones else 1), "threshold %r of %s" % (thr, name)


def _front(dev, ops, case, mode, regime, front_width=8, width=8):
    """The folded front layer (tests/test_gpu_front_dw.py): both ways on the regime's data, every byte of both code buffers."""
    n, cin, cout, h, w = case
    assert ops.pwconv_front_supported((n, cin, h, w), cout), "shape refused: %s" % (case,)
    k = FRONT._make(case, mode, regime=regime, front_width=front_width, width=width)
    want = FRONT._two_launches(k, dev, ops)
    got = FRONT._front(k, dev, ops)
    FRONT._compare(got, want, k, regime=regime)
    _eq(got["ycodes"], FRONT._input_codes(k), "codes of the depthwise input vs the host oracle's quantiser")
    if regime == "allones_divisor":
        assert took_fast_path(dev, R.divisor(k["thrB"], k["s_pw"], width)) == 0


def _chain(dev, ops, monkeypatch, case, signed, regime, width=8, mid_width=8):
    """The fused launch in statistic mode + the statistic pass that recomputes the depthwise layer (tests/test_gpu_pair_chain.py)."""
    n, cin, cmid, cout, h, w = case
    assert ops.pwdw_chain_supported((n, cin, h, w), cmid) and ops.pwconv_front_supported((n, cmid, h, w), cout), case
    k = CHAIN._make(case, signed, regime=regime, width=width, mid_width=mid_width)
    CHAIN._set_bands(monkeypatch, case)
    want, host = CHAIN._stored(k, dev, ops), CHAIN._host_mid_codes(k, ops, dev)
    got = CHAIN._chained(k, dev, ops)
    CHAIN._compare(got, want, host, regime=regime)


def _gemm_extremes(dev, ops, n, l, k, cout, zoff):
    """`gemm_i8_codes` with every activation code at an extreme (-128 / 127 as stored) against rows of +-127."""
    rng = np.random.default_rng(n + l + k + cout + zoff)
    xs = np.where(rng.random((n * l, k)) < 0.5, -128, 127).astype(np.int8)
    xs[0], xs[-1] = 127, -128
    w = np.where(rng.random((cout, k)) < 0.5, -127, 127).astype(np.int8)
    w[0], w[1 % cout] = 127, -127
    got = ops.gemm_i8_codes(torch.from_numpy(xs).to(dev), torch.from_numpy(w).to(dev), n, l, zoff)
    want = ((xs.astype(np.int64) + zoff) @ w.astype(np.int64).T).reshape(n, l, cout).transpose(0, 2, 1)
    assert want.max() == k * (255 if zoff else 128) * 127 and (k < 1000 or want.max() > 2 ** 24)
    _eq(N(got).astype(np.int64), want, "integer GEMM on extreme codes")
    _eq(N(got), O.gemm_i8_codes(xs, w, n, l, zoff), "oracle")


def _standalone(dev, ops, regime, shape, signed):
    """The stand-alone apply, statistic and producer kernels: every output and every statistic they emit is the oracle's
    bit for bit, subnormal results included (the BatchNorm shift and the second operand carry the regime's scale too)."""
    rng = np.random.default_rng(sum(shape) + 41)
    c = shape[1]

    def draw(amp):
        v = (rng.standard_normal(shape) * amp).astype(np.float32)
        return R.apply(regime, v if signed else np.maximum(v, 0), signed)[0]
    x, b = draw(2), draw(3)
    R.check(regime, x, R.stored_threshold(x), signed)
    xt = T(x, dev)
    flags = ops.act_flags(signed=signed)
    stat = O.absmax_per_sample(x)
    _eq(N(ops.absmax_per_sample(xt)), stat, "per-sample maxima")
    _eq(H.absmax_per_sample(x), stat, "host twin's per-sample maxima")
    want_y, want_cur, _, want_codes = O.conv_input_fake_quant(x, signed, 8)
    for what, (y, cur, codes) in (("online", ops.fake_quant_online(xt, 8, flags, want_codes=True)),
                                  ("prestat", ops.fake_quant_online_prestat(xt, T(stat, dev), 8, flags, want_codes=True))):
        _eq(N(cur).reshape(-1), np.float32([want_cur]), "%s current_input_max" % what)
        _eq(N(codes), want_codes.astype(np.int32), "%s codes" % what)
        _eq(N(y), want_y, "%s y" % what)
    thr = np.float32(want_cur * np.float32(0.7))
    want_y, want_cur, _, want_codes = O.conv_input_fake_quant(x, signed, 8, offline_threshold=thr)
    y, cur, codes = ops.fake_quant_offline(xt, T(np.float32([thr]), dev), 8, flags, want_codes=True)
    _eq(N(cur).reshape(-1), np.float32([want_cur]), "offline current_input_max")
    _eq(N(codes), want_codes.astype(np.int32), "offline codes")
    _eq(N(y), want_y, "offline y")
    sc = rng.uniform(0.2, 2.0, c).astype(np.float32) * rng.choice([-1, 1], c).astype(np.float32)
    sh = R.apply(regime, rng.standard_normal(c).astype(np.float32).reshape(1, c), True)[0].reshape(c)
    if regime == "zero_sample":
        sh = np.zeros_like(sh)                                        # (the zero sample stays one behind the BatchNorm)
    for act in ("relu", "none"):
        want = O.bn_act(x, sc, sh, act)
        y, st = ops.bn_act_stat(xt, T(sc, dev), T(sh, dev), act)
        _eq(N(y), want, "bn_act_stat %s" % act)
        _eq(N(st), O.absmax_per_sample(want), "bn_act_stat %s: statistic" % act)
        want, wstat = H.add_act(x, b, act, want_stat=True)
        y, st = ops.add_act_stat(xt, T(b, dev), act)
        _eq(N(y), want, "add_act_stat %s" % act)
        _eq(N(st), wstat, "add_act_stat %s: statistic" % act)
        _eq(want, np.maximum(x + b, 0) if act == "relu" else x + b, "host twin vs numpy")
        want, wstat = H.add_act(H.bn_act(x, sc, sh, "none"), b, act, want_stat=True)
        y, st = ops.bn_act_stat(xt, T(sc, dev), T(sh, dev), act, residual=T(b, dev))
        _eq(N(y), want, "bn_add_act_stat %s" % act)
        _eq(N(st), wstat, "bn_add_act_stat %s: statistic" % act)
    y, st = ops.global_avg_pool_stat(xt)
    hy, hs = H.global_avg_pool(x, want_stat=True)
    _eq(N(y).reshape(shape[:2]), np.asarray(hy).reshape(shape[:2]), "global_avg_pool_stat vs the host twin")
    _eq(N(y).reshape(shape[:2]), O.global_avg_pool(x).reshape(shape[:2]), "global_avg_pool_stat vs the numpy oracle")
    _eq(N(st), hs, "global_avg_pool_stat: statistic")
    _eq(N(st), O.absmax_per_sample(np.asarray(hy)), "global_avg_pool_stat: statistic of the oracle's means")


def _qconv_range(dev, ops, regime):
    """`qconv2d` in range mode (the producer's statistic gives the range) on tiny and huge tensors."""
    rng = np.random.default_rng(6)
    n, cin, hw, cout = 4, 128, 14, 256
    x = R.apply(regime, QC.relu_like(rng, (n, cin, hw, hw)), False)[0]
    stat = np.abs(x).reshape(n, -1).max(axis=1).astype(np.float32)
    assert (stat < 2.0 ** -90).all() if regime == "tiny" else (stat > 2.0 ** 90).all()
    w = (rng.standard_normal((cout, cin, 1, 1)) * 0.1).astype(np.float32)
    bsc = (rng.random(cout) + 0.5).astype(np.float32)
    bsh = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    for dt in ("int8", "uint8"):
        want, wstat = QC.H.qconv2d_forward(x, w, None, (1, 1), (0, 0), 1, input_dtype=dt, act="relu", bn_scale=bsc, bn_shift=bsh,
                                           in_stat=stat, want_stat=True)
        ref = QC.H.qconv2d_forward(x, w, None, (1, 1), (0, 0), 1, input_dtype=dt, act="relu", bn_scale=bsc, bn_shift=bsh)
        np.testing.assert_array_equal(want, ref)
        got, gstat = QC.run(ops, dev, x, w, None, (1, 1), (0, 0), 1, input_dtype=dt, act="relu", bn_scale=T(bsc, dev),
                            bn_shift=T(bsh, dev), in_stat=T(stat, dev), want_stat=True)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(gstat, wstat)
    wd = (rng.standard_normal((cin, 1, 3, 3)) * 0.5).astype(np.float32)
    want = QC.H.qconv2d_forward(x, wd, None, (2, 2), (1, 1), cin)
    got = QC.run(ops, dev, x, wd, None, (2, 2), (1, 1), cin, in_stat=T(stat, dev))
    np.testing.assert_array_equal(got, want)


# ---- the table --------------------------------------------------------------------------------------------------------------
# every named form of fq_pwconv_i8 at its smallest accepted shape, and the library's own choice
PW_FORMS = [("two_kernels", (2, 24, 40, 5, 7)), ("stream", (3, 256, 256, 9, 7)), ("split", (1, 3, 8, 4, 4)),
            ("sample", (2, 512, 256, 8, 8)), ("rows", (3, 64, 10, 1, 1)), (None, (2, 144, 24, 14, 14))]
# all three sides of `fq_nonneg`: unsigned; signed with lo = -max (W4 per channel, W8 per layer); the Dense quirk's signed
# levels with lo = 0
PW_MODES = ("online_u8_bn_relu", "offline_s8_channel_w4", "offline_s8_layer", "dense_quirk_bias")
# "large sum" shapes, K * levels * 127 > 2^24: one per MFMA epilogue that can reach it.  fq_pw_stream keeps the whole weight
# matrix in LDS (K <= 256) and cannot; unsigned codes need K >= 519, signed ones K >= 1041.  (An epilogue that converted the
# accumulator and the zoff * rowsum term separately shows at K >= 1181 only, in the sparse odd samples of the regime - below
# that both terms are exact in fp32: the 2048-channel shapes and the 256-channel 3x3 catch it, the 960-channel ones cannot.)
PW_LARGE = [("two_kernels", (2, 960, 320, 7, 7), ("online_u8_layer",)),
            (None, (2, 960, 320, 7, 7), ("online_u8_layer",)),
            ("split", (2, 2048, 512, 7, 7), ("online_u8_layer", "offline_s8_layer", "dense_quirk_bias")),
            ("sample", (2, 2048, 256, 8, 8), ("online_u8_layer", "offline_s8_layer")),
            ("rows", (5, 2048, 1000, 1, 1), ("online_u8_layer", "offline_s8_layer"))]
DW_SHAPES = [(2, 8, 7, 7), (3, 16, 14, 14), (2, 32, 28, 28), (1, 3, 9, 11), (5, 4, 7, 3), (1, 2, 30, 70)]
PAIR_CASES = [(2, 32, 64, 40, 36, 1), (2, 32, 32, 30, 32, 2)]
C3_SHAPES = [(5, 64, 96, 3, 3), (9, 256, 32, 4, 4), (2, 64, 64, 9, 11)]        # (the first two reach the large sums: u8 / s8)

CASES = collections.OrderedDict()

CASES["pointwise1x1"] = (
    [case(P._pwconv_case, IN, case=c, mode=m, form=f) for f, c in PW_FORMS for m in PW_MODES] +
    [case(P._pwconv_case, ("saturated",), case=c, mode=m, form=f) for f, c, modes in PW_LARGE for m in modes] +
    [case(P.test_pwconv_i8_residual_vs_oracle, IN, form=f, case=c, mode=m)
     for f, c in (("split", (3, 384, 64, 7, 7)), (None, (2, 128, 512, 9, 11)), ("sample", (2, 512, 1024, 8, 8)))
     for m in ("online_u8_bn_relu", "offline_s8_channel_w4_bn_none")] +
    [case(P.test_pwconv_i8_stride2_vs_oracle, IN, case=c, mode=m)
     for c in ((2, 64, 128, 9, 11), (4, 96, 40, 6, 7)) for m in ("online_u8_bn_relu", "offline_s8_channel_w4")] +
    # (with a residual operand the driver plants the sample's maximum, 97, on a pixel that is not stored: `huge` goes through
    # the mode without one)
    [case(SUB2.test_sub2_stores_the_even_pixels_of_the_whole_launch_and_keeps_its_statistic,
          IN if "nores" in m else [r for r in IN if r != "huge"], case=c, mode=m)
     for c in ((3, 64, 160, 9, 13), (9, 40, 192, 5, 6))
     for m in ("online_u8_bn_res_relu", "online_s8_bn_res_none", "offline_u8_bn_res_relu", "online_u8_bias_nores_relu6")] +
    [case(SUB2.test_dual_sub2_stores_both_outputs_subsampled, IN + OUT, case=(3, 64, 256, 9, 11))] +
    [case(SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin, IN, case=(2, 64, 64, 256, 5, 3), mode=m)
     for m in ("online_u8_relu", "online_s8_none", "mixed_relu6_bias")] +
    # fq_pw_short's large sums: 1024 channels on the shortcut operand (the widest instantiation), 512 on the closing one
    [case(SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin, ("saturated",), case=(2, 512, 1024, 2048, 7, 7),
          mode="online_u8_relu")] +
    [case(GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, IN, case=c, mode=m)
     for c in ((5, 512, 512, 7, 7, False), (4, 512, 2048, 7, 7, True))
     for m in ("online_u8_bn_relu", "online_s8_bn_none", "offline_u8_bias_relu6")] +
    [case(GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, ("saturated",), case=(3, 2048, 512, 7, 7, False), mode=m)
     for m in ("online_u8_bn_relu", "online_s8_bn_none")] +
    [case(C16.test_pointwise_producer_writes_the_consumers_codes, IN + OUT, case=c, mode=m)
     for c in ((3, 16, 96, 9, 11, 1), (2, 256, 512, 8, 8, 2)) for m in ("u8-out", "s8-out-relu")] +
    [case(C16.test_pointwise_consumer_of_codes_equals_consumer_of_fp32, IN, case=c, mode=m)
     for c in ((3, 16, 96, 9, 11, 1), (2, 256, 512, 8, 8, 2)) for m in ("u8_bn_relu", "s8_res")] +
    [case(C16.test_pointwise_between_two_code_tensors, IN + OUT, case=(2, 256, 64, 9, 11, 1)),
     case(C16.test_closing_pointwise_stores_the_trunk_twice, IN + OUT, case=(3, 64, 256, 9, 11))])

CASES["dense3x3"] = (
    [case(P.test_conv3x3_i8_vs_oracle, IN, case=c, mode=m)
     for c in C3_SHAPES for m in ("online_u8_bn_relu", "offline_s8_channel_w4", "online_s8_bias")] +
    [case(P.test_conv3x3_i8_sliced_vs_oracle, IN, case=c, mode=m)
     for c in C3_SHAPES for m in ("online_u8_bn_relu_wino", "offline_s8_bias")] +
    [case(C16.test_dense3x3_with_codes_on_both_sides, IN + OUT, case=c, signed=sg)
     for c in C3_SHAPES[::2] for sg in (False, True)])

CASES["depthwise3x3"] = (
    [case(P._dwconv_case, IN, shape=s, stride=st, mode=m)
     for s in DW_SHAPES for st in (1, 2) for m in ("offline_signed", "bn_relu_online")] +
    [case(P._dwconv_case, NO_QUANTISER, shape=s, stride=st, mode=m)
     for s in DW_SHAPES for st in (1, 2) for m in ("plain", "bias_relu6")] +
    [case(C16.test_depthwise_between_two_code_tensors, IN + OUT, case=c, signed=sg)
     for c in ((3, 24, 9, 11, 1), (4, 40, 5, 6, 2)) for sg in (False, True)])

CASES["recompute_pair"] = (
    # (signed codes take the general body already: `allones_divisor` runs where it is the one cause of that)
    [case(_pair, [r for r in IN if "s8" not in m or r != "allones_divisor"], case=c, mode=m)
     for c in PAIR_CASES for m in ("online_u8_bn_relu", "online_s8_lo_neg", "offline_u8_bn_relu")] +
    [case(_pair, ("allones_divisor",), case=PAIR_CASES[0], mode="offline_u8_bn_relu", allones=a) for a in (("in",), ("mid",))] +
    # (the quantisers in front of the folded layer and inside the chain work online: `saturated` has no threshold to sit in;
    # `allones_divisor` is the stored threshold of the 1x1 behind the folded layer)
    [case(_front, ONLINE + ("allones_divisor",), case=c, mode=m)
     for c in (FRONT.TAKEN[0], FRONT.TAKEN[4]) for m in ("u8_bn_relu", "s8_both")] +
    [case(_chain, ONLINE, case=(3, 32, 64, 64, 5, 28), signed=False),
     case(_chain, ONLINE, case=CHAIN.SIGNED_CASES[1], signed=True)])

CASES["head"] = (
    [case(P.test_dense_i8_eval_vs_oracle, IN, n=n, cin=ci, units=u, mode=m)
     for n, ci, u in ((7, 64, 10), (70, 100, 37)) for m in ("online", "offline_channel_w4")] +
    [case(_gemm_extremes, ("saturated",), n=n, l=l, k=k, cout=co, zoff=z)
     for n, l, k, co, z in ((1, 7, 9, 5, 128), (1, 33, 64, 33, 0), (2, 49, 27, 32, 128), (1, 33, 1152, 33, 128), (1, 33, 1152, 33, 0))])

CASES["standalone"] = [case(_standalone, R.STANDALONE, shape=s, signed=sg)
                       for s in ((3, 5, 9, 11), (4, 8, 7, 7), (5, 3, 2, 3), (2, 3, 40, 70)) for sg in (False, True)]

CASES["qconv2d"] = [case(_qconv_range, ("tiny", "huge"))]

# drivers that take the regime by that name; the others (`_gemm_extremes`) ARE their regime
_TAKES_REGIME = lambda c: c.driver is not _gemm_extremes      # noqa: E731


def regimes_of(family):
    return [r for r in R.ALL if any(r in c.regimes for c in CASES[family])]


PAIRS = [(f, r) for f in CASES for r in regimes_of(f)]


# ---- the runs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


def _describe(c):
    return "%s(%s)" % (c.driver.__name__, ", ".join("%s=%r" % kv for kv in sorted(c.kwargs.items())))


def test_the_all_ones_divisors_are_declined(dev):
    """The two thresholds the regimes store give the divisor 0x3cffffff, and `make_fast_quot` declines it - and takes the
    divisors of the thresholds the drivers store otherwise."""
    for signed in (False, True):
        d = R.divisor(R.allones_threshold(signed), signed)
        assert int(d.view(np.uint32)) == 0x3CFFFFFF and took_fast_path(dev, d) == 0
    for thr in (4.25, 3.5, 2.3):
        assert took_fast_path(dev, R.divisor(np.float32(thr), False)) == 1


@pytest.mark.parametrize("family,regime", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_family_under_regime(dev, ops, monkeypatch, family, regime):
    ran = 0
    for c in CASES[family]:
        if regime not in c.regimes:
            continue
        kw = dict(c.kwargs)
        if _TAKES_REGIME(c):
            kw["regime"] = regime
        if c.driver is _chain:
            kw["monkeypatch"] = monkeypatch
        try:
            c.driver(dev=dev, ops=ops, **kw)
        except AssertionError as e:
            raise AssertionError("regime %s, %s: %s" % (regime, _describe(c), e)) from e
        ran += 1
    assert ran > 0
