"""The value regimes of tests/regimes.py without a GPU: the table of tests/test_gpu_value_regimes.py with the numpy oracle
(oracle/patch.py: ops.py restated on it) in the place of the HIP entry points, for every driver whose launches both the numpy
oracle and the host twin (oracle/fq_host.cpp) implement.  The drivers then compare the two references bit for bit - and assert
each regime's condition from the oracle's codes, so a regime that no longer reaches its branch shows up here first.  Then:
the GPU table has a case of every family under every regime that applies to it."""
import numpy as np
import pytest
import torch

import regimes as R
import test_gpu_front_dw as FRONT
import test_gpu_pair_chain as CHAIN
import test_gpu_parity as P
import test_gpu_pwdw as PWDW
import test_gpu_shortcut as SC
import test_gpu_sub2 as SUB2
import test_gpu_value_regimes as V
from oracle import fq_oracle as O
from oracle import host as H
from oracle import patch

# drivers whose every launch oracle/patch.py restates (no code tensors, no fused pair, no pooled producer, no refusals)
HOST_DRIVERS = (P._pwconv_case, P._dwconv_case, P.test_conv3x3_i8_vs_oracle, P.test_conv3x3_i8_sliced_vs_oracle,
                P.test_pwconv_i8_residual_vs_oracle, P.test_dense_i8_eval_vs_oracle,
                SUB2.test_sub2_stores_the_even_pixels_of_the_whole_launch_and_keeps_its_statistic,
                SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin)
MAX_MACS = 3e7                                    # the numpy einsum of the larger shapes is the GPU run's to pay

# family -> the regimes that apply to it (what the GPU table must cover)
APPLIES = {
    "pointwise1x1": R.INPUT + R.OUTPUT,
    "dense3x3": R.INPUT + R.OUTPUT,
    "depthwise3x3": R.INPUT + R.OUTPUT,
    "recompute_pair": R.INPUT,
    "head": R.INPUT,
    "standalone": R.STANDALONE,
    "qconv2d": ("tiny", "huge"),
}


def _macs(c):
    shape = c.kwargs.get("case") or c.kwargs.get("shape") or ()
    return float(np.prod([v for v in shape if not isinstance(v, bool)])) if shape else 0.0


def test_the_threshold_constants_are_the_scanned_ones():
    """7.9687495 (255 levels) and 3.9687498 (127 levels): the divisor is 0x3cffffff, its significand all ones; another width
    gets a constant of its own."""
    assert R.allones_threshold(False) == np.float32(7.9687495) and R.allones_threshold(True) == np.float32(3.9687498)
    for signed, width in ((False, 8), (True, 8), (True, 4), (False, 4), (True, 2)):
        d = R.divisor(R.allones_threshold(signed, width), signed, width)
        assert int(d.view(np.uint32)) == 0x3CFFFFFF and R.has_allones_significand(d)
    assert not R.has_allones_significand(R.divisor(np.float32(2.3), True))
    # `boundaries` stores 2.75: the divisor's significand exceeds 4 / 3 for every level count, so an input just below 0.5 * d has
    # the quotient pred(0.5) - the only one on which trunc(Q + 0.5f) is not roundf(Q); 2.5 gives that with 3, 7 and 15 levels only
    assert R.BOUNDARY_THRESHOLD == np.float32(2.75)
    for signed in (False, True):
        for width in range(2, 9):
            assert R.reaches_half_pred(R.boundary_table(signed, width), R.BOUNDARY_THRESHOLD, signed, width), (signed, width)
            d = int(R.divisor(R.BOUNDARY_THRESHOLD, signed, width).view(np.uint32)) & 0x7FFFFF
            assert d > 0x2AAAAA                                     # significand > 4 / 3
    row = np.nextafter(np.float32(0.5) * R.divisor(np.float32(2.5), False), np.float32(0))
    assert not R.reaches_half_pred(row, np.float32(2.5), False)


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
@pytest.mark.parametrize("regime", R.INPUT)
def test_oracle_equals_host_twin_under_regime(regime, signed):
    """pwconv_i8, conv3x3_i8 and dwconv3x3 directly: both references agree bit for bit and every output is finite, the
    depthwise fmaf chain included (the numpy emulation of fmaf may differ at double-rounding ties on Gaussian data; here it
    does not)."""
    rng = np.random.default_rng(5)
    for taps, (n, cin, cout, h, w) in ((1, (2, 32, 40, 5, 7)), (1, (2, 1024, 64, 3, 3)), (9, (2, 64, 32, 5, 6))):
        x = (rng.standard_normal((n, cin, h, w)) * 2).astype(np.float32)
        x = x if signed else np.maximum(x, 0)
        wt = (rng.standard_normal((cout, cin) + ((1, 1) if taps == 1 else (3, 3))) * 0.1).astype(np.float32)
        x, wt, thr = R.apply(regime, x, signed, wt, cout)
        in_max = R.stored_threshold(x) if thr is None else thr
        R.check(regime, x, in_max, signed, w=wt, rps=cout, taps=taps)
        if regime == "saturated" and not signed and cin * taps >= 576:
            assert R.max_isum(x, in_max, signed, wt, cout, taps=taps) > 2 ** 24
        fo, fh = (O.pwconv_i8, H.pwconv_i8) if taps == 1 else (O.conv3x3_i8, H.conv3x3_i8)
        want = fo(x, wt, cout, 8, in_max, signed=signed)
        assert np.isfinite(want).all()
        P._eq(fh(x, wt, cout, 8, in_max=in_max, signed=signed), want, "host twin vs numpy oracle, %d taps" % taps)
    x = (rng.standard_normal((2, 8, 7, 7)) * 2).astype(np.float32)
    x = x if signed else np.maximum(x, 0)
    wt = (rng.standard_normal((8, 1, 3, 3)) * 0.5).astype(np.float32)
    x, _, thr = R.apply(regime, x, signed)
    in_max = R.stored_threshold(x) if thr is None else thr
    R.check(regime, x, in_max, signed)
    for stride in (1, 2):
        want = O.dwconv3x3(x, wt, stride=stride, in_max=in_max, signed=signed)
        assert np.isfinite(want).all()
        P._eq(H.dwconv3x3(x, wt, stride=stride, in_max=in_max, signed=signed), want, "depthwise: host twin vs numpy oracle")


@pytest.mark.parametrize("family,regime", V.PAIRS, ids=["%s-%s" % p for p in V.PAIRS])
def test_family_under_regime_on_the_references(family, regime):
    from quantization.mxnet_amd import ops
    dev = torch.device("cpu")
    ran = 0
    with patch.oracle_ops():
        for c in V.CASES[family]:
            if regime not in c.regimes:
                continue
            # the drivers that need a device: at least the data they make meets the regime's condition
            if c.driver is V._pair:
                PWDW._make(c.kwargs["case"], c.kwargs["mode"], None, None, regime=regime, allones=c.kwargs.get("allones", ("in", "mid")))
            elif c.driver is V._front:
                FRONT._make(c.kwargs["case"], c.kwargs["mode"], regime=regime)
            elif c.driver is V._chain:
                CHAIN._make(c.kwargs["case"], c.kwargs["signed"], regime=regime)
            elif c.driver in HOST_DRIVERS and _macs(c) <= MAX_MACS:
                try:
                    c.driver(dev=dev, ops=ops, regime=regime, **c.kwargs)
                except AssertionError as e:
                    raise AssertionError("regime %s, %s: %s" % (regime, V._describe(c), e)) from e
            else:
                continue
            ran += 1
    # (the launches that write codes are not restated on the references: the output-side regimes run on the GPU only, their
    # conditions below)
    assert ran > 0 or family in ("standalone", "qconv2d") or regime in R.OUTPUT


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_output_side_regimes_meet_their_conditions(signed):
    rng = np.random.default_rng(13)
    x = np.maximum(rng.standard_normal((2, 64, 9, 11)) * 2, 0).astype(np.float32)
    wt = (rng.standard_normal((96, 64, 1, 1)) * 0.2).astype(np.float32)
    y = O.pwconv_i8(x, wt, 1, 8, np.float32(2.3), act=None if signed else "relu")
    for regime in R.OUTPUT:
        thr = R.output_threshold(regime, y, signed, np.float32(1.9))
        assert thr != np.float32(1.9)
        R.check_output(regime, y, thr, signed)
        codes = O.ste_codes(y, O.act_scale(thr, signed, 8), thr, np.float32(-thr) if signed else np.float32(0))
        assert np.isfinite(codes).all() and np.abs(codes).max() <= R.levels(signed)
    assert R.output_threshold("saturated", y, signed, np.float32(1.9)) == np.float32(1.9)


def test_standalone_references_under_regime():
    """The producers' two references on the stand-alone regimes: equal bit for bit, statistics included (subnormal ones too)."""
    rng = np.random.default_rng(9)
    shape = (3, 5, 9, 11)
    for regime in R.STANDALONE:
        for signed in (False, True):
            v = (rng.standard_normal(shape) * 2).astype(np.float32)
            x = R.apply(regime, v if signed else np.maximum(v, 0), signed)[0]
            b = R.apply(regime, (rng.standard_normal(shape) * 3).astype(np.float32), True)[0]
            R.check(regime, x, R.stored_threshold(x), signed)
            flags = H.act_flags(signed=signed)
            want_y, want_cur, _, want_codes = O.conv_input_fake_quant(x, signed, 8)
            hy, hcur, hcodes = H.fake_quant_online(x, 8, flags, want_codes=True)
            P._eq(hy, want_y, "%s: y" % regime)
            P._eq(np.float32([hcur]).reshape(-1), np.float32([want_cur]), "%s: current_input_max" % regime)
            P._eq(np.asarray(hcodes).astype(np.int32).reshape(shape), want_codes.astype(np.int32), "%s: codes" % regime)
            P._eq(H.absmax_per_sample(x), O.absmax_per_sample(x), "%s: per-sample maxima" % regime)
            sc = rng.uniform(0.2, 2.0, shape[1]).astype(np.float32)
            sh = R.apply(regime, rng.standard_normal((1, shape[1])).astype(np.float32), True)[0].reshape(-1)
            y, st = H.bn_act(x, sc, sh, "none", want_stat=True)
            P._eq(y, O.bn_act(x, sc, sh, "none"), "%s: bn_act" % regime)
            P._eq(st, O.absmax_per_sample(y), "%s: bn_act statistic" % regime)
            y, st = H.add_act(x, b, "none", want_stat=True)
            P._eq(y, (x + b).astype(np.float32), "%s: add_act" % regime)
            P._eq(st, O.absmax_per_sample(y), "%s: add_act statistic" % regime)
            y, st = H.global_avg_pool(x, want_stat=True)
            P._eq(np.asarray(y).reshape(shape[:2]), O.global_avg_pool(x).reshape(shape[:2]), "%s: plane means" % regime)
            if regime == "subnormal":
                assert 0 < np.abs(x).max() < np.finfo(np.float32).tiny and st.max() > 0


def test_every_family_has_a_case_under_every_regime_that_applies_to_it():
    assert set(V.CASES) == set(APPLIES)
    for family, regimes in APPLIES.items():
        have = set(V.regimes_of(family))
        assert have == set(regimes), "%s: missing %s, beyond what applies %s" % (family, sorted(set(regimes) - have),
                                                                               sorted(have - set(regimes)))
    # the modes of the pointwise cases meet all three sides of fq_nonneg under `saturated`
    modes = {c.kwargs["mode"] for c in V.CASES["pointwise1x1"] if c.driver is P._pwconv_case and "saturated" in c.regimes}
    assert {"online_u8_bn_relu", "offline_s8_layer", "dense_quirk_bias"} <= modes
    # every MFMA epilogue that can reach them has a `saturated` case whose shape gives K * levels * 127 > 2^24
    large = {}
    for c in V.CASES["pointwise1x1"]:
        if c.driver is P._pwconv_case and "saturated" in c.regimes and "w4" not in c.kwargs["mode"]:
            signed = not c.kwargs["mode"].startswith("online")
            if R.reaches_large_sums(c.kwargs["case"][1], signed):
                large.setdefault(c.kwargs["form"], set()).add(signed)
    assert set(large) == {"two_kernels", "split", "sample", "rows", None}, large
    assert all(True in large[f] for f in ("split", "sample", "rows"))
    for driver, k in ((SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin, lambda c: c[2]),
                      (V.GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, lambda c: c[1]),
                      (P.test_conv3x3_i8_vs_oracle, lambda c: 9 * c[1]), (P.test_conv3x3_i8_sliced_vs_oracle, lambda c: 9 * c[1])):
        assert any(c.driver is driver and "saturated" in c.regimes and R.reaches_large_sums(k(c.kwargs["case"]), False)
                   for cs in V.CASES.values() for c in cs), driver.__name__
    # the pair's fused kernel (at most 256 input channels) and the streaming form (K <= 256) cannot
    assert not R.reaches_large_sums(256, False)
