"""Every int8 MFMA family at activation widths other than 8, on Gaussian data, on every rounding boundary and saturated.

The C ABI takes `in_width`, `out_width`, `mid_width`, `front_width` and `width2` from 2 to 8 and the product sends every net
with `in_width <= 8` down these paths; a kernel sees the width as `levels` only, so a wrong 8 would hide in the plumbing around
it: `out_levels` and the re-centring of the code-writing epilogues, `Codes16.matches`, `side_codes`, `width2`, the `mid_width`
a recompute plan forwards, `front_width`.  Here the case drivers of the other files - the same data, the same bit-for-bit
assertions against the numpy oracle and the host twin at that width - run with their width keyword set, under three regimes of
tests/regimes.py: None (Gaussian data), `boundaries` (every input within three fp32 neighbours of a quotient k + 0.5: at two
bits there are 3 such ties, at four 15, so every tensor here holds all of them) and `saturated`.  Where a launch hands out
codes (`x_codes_out`, `mid_codes_out`, `Codes16`) its driver compares them byte for byte with the oracle's codes at that width:
there a wrong code cannot hide behind a zero weight.

`CASES`: (family, width setting) -> [(driver, arguments, regimes)]; the shapes are the smallest that reach each form, taken from
the tables of tests/test_gpu_value_regimes.py.  tests/test_act_widths_host.py runs the same table on the two references.
No tolerance is added."""
import collections

import pytest
import torch

import test_gpu_c16 as C16
import test_gpu_front_dw as FRONT
import test_gpu_gap as GAP
import test_gpu_pair_chain as CHAIN
import test_gpu_parity as P
import test_gpu_shortcut as SC
import test_gpu_sub2 as SUB2
import test_gpu_value_regimes as V

pytestmark = pytest.mark.gpu

REGIMES = (None, "boundaries", "saturated")
STORED = REGIMES                                   # a quantiser with a threshold to store `saturated` in
ONLINE_ONLY = (None, "boundaries")                 # the front layer and the chain quantise online throughout

case = V.case

# width settings of one quantiser: unsigned; signed with lo = -max (at two bits one level: codes -1, 0, 1); the Dense quirk
UNSIGNED = collections.OrderedDict((("u2", 2), ("u4", 4), ("u7", 7)))
SIGNED = collections.OrderedDict((("s2", 2), ("s4", 4)))
QUIRK = collections.OrderedDict((("quirk4", 4),))
# (input width, output width) of the code-writing launches; (input, middle) of a recompute pair; the two operands of the
# folded shortcut
IN_OUT = collections.OrderedDict((("in2-out2", (2, 2)), ("in4-out4", (4, 4)), ("in8-out4", (8, 4)), ("in4-out8", (4, 8))))
IN_MID = collections.OrderedDict((("in4-mid4", (4, 4)), ("in8-mid4", (8, 4)), ("in4-mid8", (4, 8))))
OPERANDS = collections.OrderedDict((("x4-x2_4", (4, 4)), ("x8-x2_4", (8, 4))))

CASES = collections.OrderedDict()


def _add(family, setting, cases):
    CASES.setdefault((family, setting), []).extend(cases)


for kind, settings in (("u", UNSIGNED), ("s", SIGNED), ("q", QUIRK)):
    for name, wd in settings.items():
        mode = {"u": "online_u8_bn_relu", "s": "offline_s8_channel_w4", "q": "dense_quirk_bias"}[kind]
        # every named form of fq_pwconv_i8 and the library's own choice
        _add("pointwise1x1", name, [case(P._pwconv_case, STORED, case=c, mode=mode, form=f, width=wd) for f, c in V.PW_FORMS])
        if kind == "q":
            continue
        sg = kind == "s"
        _add("pointwise1x1", name, [
            case(P.test_pwconv_i8_residual_vs_oracle, STORED, form="split", case=(3, 384, 64, 7, 7),
                 mode="offline_s8_channel_w4_bn_none" if sg else "online_u8_bn_relu", width=wd),
            case(P.test_pwconv_i8_stride2_vs_oracle, STORED, case=(4, 96, 40, 6, 7), mode=mode, width=wd),
            case(SUB2.test_sub2_stores_the_even_pixels_of_the_whole_launch_and_keeps_its_statistic, STORED, case=(9, 40, 192, 5, 6),
                 mode="online_s8_bn_res_none" if sg else "online_u8_bn_res_relu", width=wd),
            case(GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, STORED, case=(5, 512, 512, 7, 7, False),
                 mode="online_s8_bn_none" if sg else "online_u8_bn_relu", width=wd)])
        # one and three digit slices
        _add("dense3x3", name,
             [case(P.test_conv3x3_i8_vs_oracle, STORED, case=c, mode=mode, width=wd) for c in ((2, 64, 64, 9, 11), (5, 64, 96, 3, 3))] +
             [case(P.test_conv3x3_i8_sliced_vs_oracle, STORED, case=c, mode="offline_s8_bias" if sg else "online_u8_bn_relu_wino",
                   width=wd) for c in ((2, 64, 64, 9, 11), (5, 64, 96, 3, 3))])
        _add("depthwise3x3", name, [case(P._dwconv_case, STORED, shape=s, stride=st, mode="offline_signed" if sg else "bn_relu_online",
                                         width=wd) for s in V.DW_SHAPES for st in (1, 2)])
        if not sg:                                 # (the classifier's input is a ReLU's: unsigned codes, clipped at 0)
            _add("head", name, [case(P.test_dense_i8_eval_vs_oracle, STORED, n=7, cin=64, units=10, mode=m, width=wd)
                                for m in ("online", "offline_channel_w4")])

for name, (wd, wd2) in OPERANDS.items():
    _add("pointwise1x1", name, [case(SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin, STORED,
                                     case=(2, 64, 64, 256, 5, 3), mode=m, width=wd, width2=wd2)
                                for m in ("online_u8_relu", "online_s8_none")])

# launches that read or write codes: the producer's out_levels and re-centring, what `Codes16` records and `matches` compares,
# the side copy of the closing 1x1 (whole and subsampled)
for name, (wd, owd) in IN_OUT.items():
    _add("codes", name,
         [case(C16.test_pointwise_producer_writes_the_consumers_codes, STORED, case=(3, 16, 96, 9, 11, 1), mode=m, width=wd, out_width=owd)
          for m in ("u8-out", "s8-out-relu")] +
         [case(C16.test_pointwise_consumer_of_codes_equals_consumer_of_fp32, STORED, case=(3, 16, 96, 9, 11, 1), mode=m, width=wd)
          for m in ("u8_bn_relu", "s8_res") if owd == wd or wd != 8] +
         [case(C16.test_pointwise_between_two_code_tensors, STORED, case=(2, 256, 64, 9, 11, 1), width=wd, out_width=owd),
          case(C16.test_closing_pointwise_stores_the_trunk_twice, STORED, case=(3, 64, 256, 9, 11), width=wd, out_width=owd),
          case(SUB2.test_dual_sub2_stores_both_outputs_subsampled, STORED, case=(3, 64, 256, 9, 11), width=wd, out_width=owd)] +
         [case(C16.test_dense3x3_with_codes_on_both_sides, STORED, case=(2, 64, 64, 9, 11), signed=sg, width=wd, out_width=owd)
          for sg in (False, True)] +
         [case(C16.test_depthwise_between_two_code_tensors, STORED, case=c, signed=sg, width=wd, out_width=owd)
          for c in ((3, 24, 9, 11, 1), (4, 40, 5, 6, 2)) for sg in (False, True)])

# the recompute pair (`mid_width`, `x_codes_out`), the folded front layer (`front_width`: its depthwise quantiser is the pair's
# first, the 1x1 behind it the second) and the chained pair (`mid_codes_out`)
for name, (wd, mid) in IN_MID.items():
    _add("recompute_pair", name,
         [case(V._pair, STORED, case=c, mode=m, width=wd, mid_width=mid)
          for c in V.PAIR_CASES for m in ("online_u8_bn_relu", "online_s8_lo_neg", "offline_u8_bn_relu")] +
         [case(V._front, ONLINE_ONLY, case=FRONT.TAKEN[0], mode=m, front_width=wd, width=mid) for m in ("u8_bn_relu", "s8_both")] +
         [case(V._chain, ONLINE_ONLY, case=(3, 32, 64, 64, 5, 28), signed=False, width=wd, mid_width=mid),
          case(V._chain, ONLINE_ONLY, case=CHAIN.SIGNED_CASES[1], signed=True, width=wd, mid_width=mid)])

TRIPLES = [(f, s, r) for (f, s), cs in CASES.items() for r in REGIMES if any(r in c.regimes for c in cs)]


def _id(t):
    return "%s-%s-%s" % (t[0], t[1], t[2] or "gaussian")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("family,setting,regime", TRIPLES, ids=[_id(t) for t in TRIPLES])
def test_family_at_width_under_regime(dev, ops, monkeypatch, family, setting, regime):
    ran = 0
    for c in CASES[(family, setting)]:
        if regime not in c.regimes:
            continue
        kw = dict(c.kwargs, regime=regime)
        if c.driver is V._chain:
            kw["monkeypatch"] = monkeypatch
        try:
            c.driver(dev=dev, ops=ops, **kw)
        except AssertionError as e:
            raise AssertionError("%s, regime %s, %s: %s" % (setting, regime, V._describe(c), e)) from e
        ran += 1
    assert ran > 0


def test_codes_carry_their_width_and_a_launch_that_names_another_is_refused(dev, ops):
    """What `Codes16` records and `matches` compares: a producer told `out_codes["width"] = 4` hands over a tensor that says 4,
    its consumers at width 4 - 1x1, dense 3x3, depthwise 3x3 - compute what they compute from the fp32
    tensor under that threshold, and every one of them refuses the same tensor under the same threshold at width 8 or 2 before
    anything is launched (the codes would be read against the wrong scale)."""
    import numpy as np
    from oracle import fq_oracle as O
    T, N = P.T, P.N
    rng = np.random.default_rng(77)
    n, cin, c, h, w = 2, 32, 64, 5, 6
    x = np.maximum(rng.standard_normal((n, cin, h, w)) * 2, 0).astype(np.float32)
    wt = (rng.standard_normal((c, cin, 1, 1)) * 0.2).astype(np.float32)
    codes = ops.weight_codes(T(wt, dev), 1, 8)
    thr, thr2 = T(np.float32([2.3]), dev), T(np.float32([1.9]), dev)
    kw = dict(in_thr=thr, width=8, flags=0, act="relu")
    y, _ = ops.pwconv_i8(T(x, dev), *codes, form="split", **kw)
    yc, _ = ops.pwconv_i8(T(x, dev), *codes, out_codes=dict(thr=thr2, width=4, flags=0), **kw)
    assert isinstance(yc, ops.Codes16) and yc.width == 4 and yc.matches(thr2, 4, 0)
    assert not yc.matches(thr2, 8, 0) and not yc.matches(thr2, 2, 0) and not yc.matches(thr2, 4, ops.act_flags(signed=True))
    want = O.ste_codes(N(y), O.act_scale(np.float32(1.9), False, 4), np.float32(1.9), np.float32(0))
    P._eq(N(yc.t), O.to_c16(want.astype(np.int64), 128), "codes at four bits")
    assert want.max() == 15
    pw = ops.weight_codes(T((rng.standard_normal((c, c, 1, 1)) * 0.1).astype(np.float32), dev), 1, 8)
    c3 = ops.weight_codes_3x3(T((rng.standard_normal((c, c, 3, 3)) * 0.1).astype(np.float32), dev), 1, 8)
    dww = T((rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32), dev)
    oc = dict(thr=T(np.float32([1.7]), dev), width=8, flags=0)

    def consumers(src, width):
        a = ops.pwconv_i8(src, *pw, in_thr=thr2, width=width, flags=0, act="relu", **(dict() if src is yc else dict(form="split")))[0]
        b = ops.conv3x3_i8(src, *c3, in_thr=thr2, width=width, flags=0, act="relu")[0]
        return a, b
    for g, r, what in zip(consumers(yc, 4), consumers(y, 4), ("1x1", "dense 3x3")):
        assert torch.equal(g, r), what
    dw_c = ops.dwconv3x3_c16(yc, dww, in_thr=thr2, width=4, flags=0, act="relu", out_codes=oc)[0]
    dw_f = ops.dwconv3x3(y, dww, in_thr=thr2, width=4, flags=0, act="relu")[0]
    wantc = O.ste_codes(N(dw_f), O.act_scale(np.float32(1.7), False, 8), np.float32(1.7), np.float32(0))
    P._eq(N(dw_c.t), O.to_c16(wantc.astype(np.int64), 128), "depthwise on four-bit codes")
    for width in (8, 2):
        with pytest.raises(ValueError, match="width"):
            ops.pwconv_i8(yc, *pw, in_thr=thr2, width=width, flags=0)
        with pytest.raises(ValueError, match="width"):
            ops.conv3x3_i8(yc, *c3, in_thr=thr2, width=width, flags=0)
        with pytest.raises(ValueError, match="width"):
            ops.dwconv3x3_c16(yc, dww, in_thr=thr2, width=width, flags=0, out_codes=oc)
