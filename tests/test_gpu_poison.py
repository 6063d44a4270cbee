"""Every kernel family under poisoned, guard-banded memory (tests/poison.py).

The other GPU tests launch a baseline and a variant at the same shape in one process, and torch's caching allocator hands
the variant the block the baseline just wrote: a kernel that skips a strip, leaves a statistic slot uninitialised, reads
workspace it did not write in this call or runs a few elements past a buffer can pass them.  Here the same case drivers and
the same assertions run with `ops`' outputs, statistic targets and workspaces taken from freshly poisoned buffers between
guard bands, the test inputs between guard bands of their own, under both byte patterns - and the guards are checked after
a device synchronise.  `CASES` is the table: family -> [(entry points of ops.py it runs, driver, arguments)]; the CPU test
tests/test_poison_harness.py asserts that every allocating entry point of ops.py is named in it.

No tolerance is added here: a driver asserts exactly what its own test asserts (bit for bit wherever that holds)."""
import collections
import inspect

import numpy as np
import pytest
import torch

import poison
import test_gpu_c16 as C16
import test_gpu_gap as GAP
import test_gpu_kl_fused as KLF
import test_gpu_parity as P
import test_gpu_pwdw as PWDW
import test_gpu_pwdw_codes as PWDWC
import test_gpu_qconv as QC
import test_gpu_shortcut as SC
import test_gpu_sub2 as SUB2
from oracle import fq_oracle as O
from oracle import host as H
from oracle import patch as REF          # ops.py's entry points restated on the numpy oracle, same signatures

pytestmark = pytest.mark.gpu

DRIVER_MODULES = (P, PWDW, PWDWC, C16, GAP, KLF, QC, SC, SUB2)     # their `T` / `_t` make the guarded inputs

Case = collections.namedtuple("Case", "entries driver kwargs")


def case(entries, driver, **kwargs):
    return Case(tuple(entries.split()), driver, kwargs)


_eq, N = P._eq, P.N


# ---- drivers of what has no driver of its own -------------------------------------------------------------------------------
def _apply_extras(dev, ops, shape):
    """The entry points around the apply kernels against ops.py restated on the numpy oracle (oracle/patch.py) and the host
    twins: apply with a given statistic (+ codes), the batch means, the calibration-step records, the generic STE."""
    rng = np.random.default_rng(sum(shape) + 5)
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    n = shape[0]
    xt = P.T(x, dev)
    stat = ops.absmax_per_sample(xt)
    _eq(N(stat), O.absmax_per_sample(x), "per-sample maxima")
    _eq(N(ops.absmax_per_sample(xt, no_abs=True)), N(REF.absmax_per_sample(xt, no_abs=True)), "per-sample maxima, no abs")
    for width, flags in ((8, ops.act_flags(signed=True)), (4, 0)):
        y, cur, codes = ops.fake_quant_online_prestat(xt, stat, width, flags, want_codes=True)
        hy, hcur, hcodes = H.fake_quant_online_prestat(x, O.absmax_per_sample(x), width, flags, want_codes=True)
        _eq(N(y), hy, "prestat y")
        _eq(N(cur).reshape(-1), np.asarray(hcur, np.float32).reshape(-1), "prestat current_max")
        _eq(N(codes), np.asarray(hcodes).astype(np.int32).reshape(shape), "prestat codes")
        y2, cur2, codes2 = ops.fake_quant_online(xt, width, flags, want_codes=True)
        _eq(N(y2), hy, "online y")
        _eq(N(codes2), N(codes), "online codes")
        thr = P.T(np.float32([1.9]), dev)
        y3, cur3, codes3 = ops.fake_quant_offline(xt, thr, width, flags, want_codes=True)
        ry, rcur, rcodes = REF.fake_quant_offline(xt, thr, width, flags, want_codes=True)
        _eq(N(y3), N(ry), "offline y")
        _eq(N(cur3), N(rcur), "offline current_max")
        _eq(N(codes3), N(rcodes), "offline codes")
    _eq(N(ops.batch_mean(stat)), N(REF.batch_mean(stat)), "batch mean")
    rows = (rng.random((3, n)) * 10).astype(np.float32)
    rt = P.T(rows, dev)
    _eq(N(ops.batch_mean_rows(rt)), N(REF.batch_mean_rows(rt)), "row-wise batch means")
    for take in sorted({1, n}):
        rec = ops.stat_rows_sum(rt, take)
        _eq(N(rec), N(REF.stat_rows_sum(rt, take)), "fp64 sums of the first %d maxima of each row, then the count" % take)
        _eq(N(ops.mean_from_sums(rec)), N(REF.mean_from_sums(rec)), "means from the sums")
    packs = np.zeros((2, n + 2), np.float32)                       # two ranks' records {count, values...}
    packs[0, 0], packs[0, 1:1 + n] = n, rows[0]
    packs[1, 0], packs[1, 1:2] = 1, rows[1, :1]
    pt = P.T(packs, dev)
    _eq(N(ops.batch_mean_gathered(pt)), N(REF.batch_mean_gathered(pt)), "batch mean of gathered records")
    for scales, clip in ((np.float32([0.037]), (2.5, -2.5)), ((rng.random(n) * 0.1 + 0.01).astype(np.float32), (None, None)),
                         ((rng.random(n) * 0.1 + 0.01).astype(np.float32), (1.5, None))):
        st = P.T(scales, dev)
        y = ops.ste_forward(xt, st, clip[0], clip[1])
        _eq(N(y), H.ste_forward(x, scales, clip[0], clip[1]), "STE forward, %d scales, clip %s" % (scales.size, clip))
        _eq(N(y), N(REF.ste_forward(xt, st, clip[0], clip[1])), "STE forward vs the numpy oracle")


def _apply_unaligned(dev, ops):
    """4-byte-aligned views: the scalar forms of the apply, statistic and STE kernels."""
    rng = np.random.default_rng(3)
    big = rng.standard_normal(3 * 1001 + 1).astype(np.float32)
    xt = P.T(big, dev)[1:].reshape(3, 1001)
    x = big[1:].reshape(3, 1001)
    assert xt.data_ptr() % 16 != 0 and xt.is_contiguous()
    want_y, want_cur, _, want_codes = O.conv_input_fake_quant(x, True, 8)
    y, cur, codes = ops.fake_quant_online(xt, 8, ops.act_flags(signed=True), want_codes=True)
    assert N(cur)[0] == want_cur
    _eq(N(y), want_y, "y")
    _eq(N(codes), want_codes.astype(np.int32), "codes")
    _eq(N(ops.absmax_per_sample(xt)), O.absmax_per_sample(x), "per-sample maxima")
    thr = np.float32(want_cur * np.float32(0.7))
    want_y, want_cur, _, want_codes = O.conv_input_fake_quant(x, True, 8, offline_threshold=thr)
    y, cur, codes = ops.fake_quant_offline(xt, P.T(np.float32([thr]), dev), 8, ops.act_flags(signed=True), want_codes=True)
    assert N(cur)[0] == want_cur
    _eq(N(y), want_y, "offline y")
    _eq(N(codes), want_codes.astype(np.int32), "offline codes")
    sc = np.float32([0.01, 0.02, 0.03])
    _eq(N(ops.ste_forward(xt, P.T(sc, dev), 2.0, -2.0)), H.ste_forward(x, sc, 2.0, -2.0), "STE forward")


def _hist_sinks(dev, ops, shape, bins):
    KLF.test_batchnorm_pass_bins_what_it_stores(dev, ops, shape, "relu", bins)
    KLF.test_batchnorm_pass_bins_what_it_stores(dev, ops, shape, "none", bins)
    KLF.test_residual_pass_bins_what_it_stores(dev, ops, shape, 2048)
    # ... and the residual form of the BatchNorm pass with a sink: the counts the separate histogram pass adds
    rng = np.random.default_rng(sum(shape) + bins)
    x, r = (P.T((rng.standard_normal(shape) * 2).astype(np.float32), dev) for _ in range(2))
    sc = P.T((rng.random(shape[1]) + 0.5).astype(np.float32), dev)
    sh = P.T(rng.standard_normal(shape[1]).astype(np.float32), dev)
    y0, s0 = ops.bn_act_stat(x, sc, sh, "relu", residual=r)
    mx_ = float(y0.max()) * 0.8
    want, got = KLF.Sink(bins, mx_, dev), KLF.Sink(bins, mx_, dev)
    ops.histogram_accumulate(y0, want.fm_max, want.hist, want.neg)
    y1, s1 = ops.bn_act_stat(x, sc, sh, "relu", residual=r, hist=got)
    assert torch.equal(y1, y0) and torch.equal(s1, s0)
    assert torch.equal(got.hist, want.hist) and int(got.neg) == int(want.neg) == 0


def _pair(dev, ops, case, mode, regime=None, allones=("in", "mid"), width=8, mid_width=8):
    """`pwconv_i8_stat` + `pwdw_fused`, without and with the handed-over codes, against the two storing launches and the
    host twins (the assertions of test_pwdw_fused_equals_the_two_launches_and_the_host_twins), and the code buffer - taken
    from poisoned memory - against the host quantiser's codes, every byte."""
    n, cin, cout, h, w, stride = case
    assert ops.pwdw_supported((n, cin, h, w), cout, stride), "shape refused: %s" % (case,)
    PWDW.test_pwdw_fused_equals_the_two_launches_and_the_host_twins(dev, ops, case, mode, regime=regime, allones=allones, width=width,
                                                                    mid_width=mid_width)
    k = PWDW._make(case, mode, dev, ops, regime=regime, allones=allones, width=width, mid_width=mid_width)
    two = PWDW._run_pair(k, dev, ops, fused=False)
    buf = ops.torch.empty(ops.pair_codes_shape((n, cin, h, w)), dtype=torch.int8, device=dev)     # the proxy's: poisoned
    hand = PWDW._run_pair(k, dev, ops, fused=True, codes_buf=buf)
    for name in ("ystat", "cur1", "cur2", "z", "zstat"):
        _eq(hand[name], two[name], "%s with the codes handed over vs the two launches" % name)
    host = PWDW._host_pair(k, ops, dev)
    _eq(hand["z"], host["z"], "fused output on the codes vs host twins")
    _eq(hand["zstat"], host["zstat"], "fused statistic on the codes vs host twins")
    flags = H.act_flags(signed=k["signed"])
    if k["offline"]:
        codes = H.fake_quant_offline(k["x"], k["thr1"], width, flags, want_codes=True, want_stat=False)[2]
    else:
        codes = H.fake_quant_online_prestat(k["x"], H.absmax_per_sample(k["x"]), width, flags, want_codes=True)[2]
    cb = 2 * ((cin + 31) // 32)
    full = np.zeros((n, cb * 16, h * w), np.int64)
    full[:, :cin] = np.asarray(codes).reshape(n, cin, h * w)
    byte = ((full + 128 - (0 if k["signed"] else 128)) ^ 0x80) & 0xFF
    _eq(N(buf), byte.astype(np.uint8).view(np.int8).reshape(n, cb, 16, h * w).transpose(0, 1, 3, 2),
        "code buffer vs the host oracle's quantiser")


def _weight_codes(dev, ops, shape):
    """`weight_codes` against the oracle - and the PADDED rows and columns of the code buffer are zero (consumers multiply
    by them), both copies' worth of buffer stays inside its allocation."""
    rng = np.random.default_rng(sum(shape))
    w = (rng.standard_normal(shape) * rng.uniform(0.01, 2.0, (shape[0],) + (1,) * (len(shape) - 1))).astype(np.float32)
    rows, row_len = shape[0], int(np.prod(shape[1:]))
    for rps, width in ((1, 8), (rows, 8), (1, 4)):
        codes, scales, rowsum = ops.weight_codes(P.T(w, dev), rps, width)
        ocodes, oscales = O.weight_codes(w, rps, width)
        got = N(codes)
        assert got.shape == ((rows + 63) // 64 * 64, (row_len + 63) // 64 * 64)
        _eq(got[:rows, :row_len], ocodes.reshape(rows, row_len).astype(np.int8), "weight codes")
        assert not got[rows:].any(), "padded rows of the code buffer are not zero"
        assert not got[:, row_len:].any(), "padded columns of the code buffer are not zero"
        _eq(N(scales), oscales, "weight scales")
        _eq(N(rowsum), ocodes.reshape(rows, row_len).sum(axis=1).astype(np.int32), "row sums")
        hc, hs, hr = H.weight_codes(w, rps, width)
        _eq(got, np.asarray(hc), "host twin's codes, padding included")
        _eq(N(scales), hs, "host twin's scales")


def _weights_3x3(dev, ops, shape):
    """`weight_codes_3x3` ((tap, ci) order, zero padding) and `weight_slices_3x3` (three digit slices) against the oracle."""
    cout, cin = shape[0], shape[1]
    rng = np.random.default_rng(sum(shape) + 1)
    w = (rng.standard_normal(shape) * rng.uniform(0.02, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    w[1] = 0.0
    for rps, width in ((1, 4), (cout, 8)):
        codes, scales, rowsum = ops.weight_codes_3x3(P.T(w, dev), rps, width)
        ocodes, oscales = O.weight_codes(w, rps, width)
        got = N(codes)
        _eq(got[:cout, :9 * cin], ocodes.reshape(cout, cin, 3, 3).transpose(0, 2, 3, 1).reshape(cout, -1).astype(np.int8),
            "weight codes in (tap, ci) order")
        assert not got[cout:].any() and not got[:, 9 * cin:].any(), "padding of the code buffer is not zero"
        _eq(N(scales), oscales, "weight scales")
        _eq(N(rowsum), ocodes.reshape(cout, -1).sum(axis=1).astype(np.int32), "row sums")
    codes, pscale, rowsum = ops.weight_slices_3x3(P.T(w, dev))
    m, p = O.weight_slices(w.transpose(0, 2, 3, 1).reshape(cout, -1))
    _eq(N(pscale), p, "per-channel power-of-two scale")
    rows_pad, row_pad = (cout + 63) // 64 * 64, (9 * cin + 63) // 64 * 64
    for sl, d in enumerate(O.slice_digits(m)):
        got = N(codes)[sl, :rows_pad * row_pad].reshape(rows_pad, row_pad)
        _eq(got[:cout, :9 * cin], d.astype(np.int8), "digit slice %d" % sl)
        assert not got[cout:].any() and not got[:, 9 * cin:].any(), "padding of digit slice %d is not zero" % sl
        _eq(N(rowsum)[sl], d.sum(axis=1).astype(np.int32), "row sums of slice %d" % sl)


def _wino_weight(dev, ops, shape):
    rng = np.random.default_rng(sum(shape) + 2)
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    for variant, width in (("F23", 8), ("F43", 8), ("F63", 4)):
        want, want_sc, _ = O.wino_weight_fake_quant(w, variant, width)
        wq, sc = ops.wino_weight_fake_quant(P.T(w, dev), variant, width, want_scales=True)
        _eq(N(sc), want_sc, "%s scales" % variant)
        _eq(N(wq), want, "%s weights" % variant)


def _calibration_unaligned(dev, ops):
    """`global_max` and `histogram_accumulate` through a view that is only 4-byte aligned (the scalar histogram kernel),
    beside the aligned call on the same values."""
    rng = np.random.default_rng(17)
    big = np.maximum(rng.standard_normal(4 * 2500 + 1), 0).astype(np.float32) * 3
    for off in (0, 1):
        x = big[off:off + 4 * 2500].copy()
        xt = P.T(big, dev)[off:off + 4 * 2500]
        assert (xt.data_ptr() % 16 != 0) == bool(off) and xt.is_contiguous()
        mx = ops.global_max(xt)
        assert N(mx)[0] == x.max() == H.global_max(x)
        for bins in (2048, 100):
            hist = torch.zeros(bins, dtype=torch.int64, device=dev)
            neg = torch.zeros(1, dtype=torch.int32, device=dev)
            for _ in range(2):
                ops.histogram_accumulate(xt, mx, hist, neg)
            want, _ = O.discrete_histogram(x, bins, x.max())
            _eq(N(hist).astype(np.float32), 2 * want, "histogram, %d bins, offset %d" % (bins, off))
            _eq(N(ops.hist_to_float(hist)), 2 * want, "counts as fp32")
            assert int(N(neg)[0]) == 0
            hh, hneg = H.histogram_accumulate(x, x.max(), bins)
            _eq(N(hist), 2 * hh.astype(np.int64), "host twin's counts")
    xs = (rng.standard_normal(1001) * 2).astype(np.float32)                    # with negatives, through the unaligned view
    xt = P.T(np.concatenate([np.float32([0]), xs]), dev)[1:]
    hist = torch.zeros(64, dtype=torch.int64, device=dev)
    neg = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.histogram_accumulate(xt, P.T(np.float32([xs.max()]), dev), hist, neg)
    hh, hneg = H.histogram_accumulate(xs, xs.max(), 64)
    _eq(N(hist), hh.astype(np.int64), "counts beside negatives")
    assert int(N(neg)[0]) == hneg == int((xs < 0).sum())


def _kl_search(dev, ops, golden):
    P.test_kl_search_golden_all_cases_one_launch_per_level(golden, dev, ops)
    g = golden("g2_kl")
    names = ["halfnormal", "exponential", "relu_outlier", "accumulated6", "sparse", "spike"]
    hists = np.stack([g[n + "/hist"] for n in names])
    for levels, min_bins in ((128, 128), (128, 384), (16, 16)):
        _eq(N(ops.kl_search(P.T(hists, dev), levels, min_bins)), H.kl_search(hists, levels, min_bins),
            "levels %d, min_bins %d vs the host twin" % (levels, min_bins))


def _codes_roundtrip(dev, ops, golden):
    for name in ("u01", "normal", "shifted"):
        for t in ("int8", "uint8"):
            P.test_quantize_codes_golden(golden, dev, ops, name, t)
    P.test_quantize_codes_fixed_range_and_explicit_scale(dev, ops)
    rng = np.random.default_rng(23)
    x = (rng.standard_normal((3, 5, 9, 11)) * 2).astype(np.float32)
    xt = P.T(np.concatenate([np.float32([0]), x.reshape(-1)]), dev)[1:].reshape(x.shape)       # 4-byte aligned only
    for t in ("int8", "uint8"):
        codes, r = ops.quantize_codes(xt, t)
        rc, rr = REF.quantize_codes(xt, t)
        _eq(N(codes), N(rc), "%s codes" % t)
        _eq(N(r), N(rr), "%s range record" % t)
        _eq(N(ops.dequantize(codes, r[2:3])), N(REF.dequantize(codes, r[2:3])), "dequantised")
    for tag in ("layer_w8", "channel_w4"):
        P.test_ema_golden(golden, dev, ops, tag)


def _qconv_direct(dev, ops, which, in_dt, w_dt):
    QC.test_direct_kernel_every_geometry(dev, ops, QC.DIRECT_CASES[which], in_dt, w_dt)


# ---- the table --------------------------------------------------------------------------------------------------------------
PW = "pwconv_i8 weight_codes"
PW_MODES = ("online_u8_bn_relu", "offline_s8_channel_w4", "dense_quirk_bias")
# every named form of P.FORM_CASES at its smallest accepted shape(s), then the padded / partial-tile shapes under the
# library's own choice and under the forms that take them
PW_FORMS = [("two_kernels", (2, 24, 40, 5, 7)), ("stream", (3, 256, 256, 9, 7)), ("split", (1, 3, 8, 4, 4)),
            ("sample", (5, 128, 512, 10, 10)), ("sample", (2, 512, 256, 8, 8)), ("rows", (3, 64, 10, 1, 1)),
            (None, (2, 24, 40, 5, 7)), ("split", (2, 24, 40, 5, 7)), (None, (1, 3, 8, 4, 4)),
            (None, (2, 144, 24, 14, 14)), ("two_kernels", (2, 144, 24, 14, 14)), ("split", (2, 144, 24, 14, 14)),
            (None, (33, 100, 37, 1, 1)), ("rows", (33, 100, 37, 1, 1))]
DW_SHAPES = [(2, 8, 7, 7), (3, 16, 14, 14), (2, 32, 28, 28), (1, 3, 9, 11), (5, 4, 7, 3), (1, 2, 30, 70), (1, 2, 130, 64)]
PAIR_CASES = [(2, 32, 64, 40, 36, 1), (2, 32, 32, 30, 32, 2), (1, 64, 64, 18, 60, 1), (3, 128, 256, 28, 28, 1)]
C3_SHAPES = [(5, 64, 96, 3, 3), (9, 256, 32, 4, 4), (1, 128, 64, 1, 50), (2, 64, 64, 9, 11)]

CASES = collections.OrderedDict()

CASES["apply_and_statistic"] = (
    [case("fake_quant_online fake_quant_offline absmax_per_sample", P.test_activation_vs_oracle, shape=s, signed=sg, width=wd)
     for s in ((1, 1, 1, 1), (3, 5, 9, 11), (2, 8196)) for sg, wd in ((False, 8), (True, 2))] +
    [case("fake_quant_online_prestat fake_quant_online fake_quant_offline absmax_per_sample batch_mean batch_mean_rows "
          "batch_mean_gathered stat_rows_sum mean_from_sums ste_forward", _apply_extras, shape=s)
     for s in ((1, 1, 1, 1), (3, 5, 9, 11), (2, 8196))] +
    [case("fake_quant_online fake_quant_offline absmax_per_sample ste_forward", _apply_unaligned),
     case("fake_quant_online", P.test_unaligned_views_take_the_scalar_path),
     case("fake_quant_online", P.test_act_output_variant_no_abs_no_eps),
     case("batch_mean", P.test_batch_mean_is_the_defined_order)])

CASES["batchnorm_add_pooling_producers"] = (
    [case("bn_act_stat fake_quant_online fake_quant_online_prestat", P.test_bn_act_stat_vs_oracle, shape=s, act=a)
     for s in ((3, 5, 9, 11), (5, 3, 1, 1), (4, 8, 7, 7)) for a in ("relu", "relu6", "none")] +
    [case("bn_act_stat add_act_stat", P.test_bn_add_act_stat_is_the_two_passes_in_one, shape=s, act=a)
     for s in ((3, 5, 9, 11), (5, 3, 1, 1), (4, 8, 7, 7)) for a in ("relu", "none")] +
    [case("add_act_stat", P.test_add_act_stat_vs_oracle, shape=s, act=a)
     for s in ((3, 5, 9, 11), (3, 64, 7, 7), (4, 8, 7, 7), (2, 10, 5, 3)) for a in ("relu", "relu6", "none")] +     # (planes of two rows or more: it slices one off)
    [case("bn_act_maxpool_stat", P.test_bn_act_maxpool_stat_vs_oracle, shape=s, act=a)
     for s in ((3, 5, 9, 12), (1, 3, 8, 8), (2, 4, 7, 4)) for a in ("relu", "none")] +
    [case("global_avg_pool_stat", P.test_global_avg_pool_stat_vs_oracle, shape=s)
     for s in ((3, 5, 9, 11), (5, 3, 1, 1), (4, 8, 7, 7), (3, 17, 5, 4))] +
    [case("bn_act_stat add_act_stat", _hist_sinks, shape=s, bins=b)
     for s, b in (((3, 5, 9, 11), 128), ((7, 33, 7, 7), 2048), ((1, 8, 4, 4), 2048))])

CASES["first_convolutions"] = (
    [case("stem_conv_s2", P.test_stem_conv_s2_vs_oracle, shape=s, mode=m, ks=ks, cout=co)
     for s in ((3, 3, 33, 47), (5, 3, 18, 130), (3, 3, 45, 64)) for ks, co in ((3, 32), (7, 64)) for m in ("bn_relu", "bias_relu6")] +
    [case("stem_conv_s2 bn_act_maxpool_stat", P.test_stem_conv7x7_with_maxpool_in_one_launch_vs_oracle, shape=s, mode=m)
     for s in ((1, 3, 195, 201), (5, 3, 31, 250)) for m in ("bn_relu", "plain")] +
    [case("stem_conv_s2", C16.test_first_convolution_hands_its_consumers_codes_over, shape=s, act=a)
     for s in ((2, 33, 47), (3, 64, 64)) for a in ("relu6", "relu6-thr9")])

CASES["depthwise3x3"] = (
    [case("dwconv3x3", P._dwconv_case, shape=s, stride=st, mode=m, twin=True)
     for s in DW_SHAPES for st in (1, 2) for m in ("plain", "offline_signed", "bn_relu_online", "bias_relu6")] +
    [case("dwconv3x3_c16 dwconv3x3", C16.test_depthwise_between_two_code_tensors, case=c, signed=sg)
     for c in ((3, 24, 9, 11, 1), (4, 40, 5, 6, 2)) for sg in (False, True)] +
    [case("dwconv3x3_c16", C16.test_depthwise_on_codes_every_epilogue_on_planes_shorter_than_the_prefetch, case=c, epi=e)
     for c in ((2, 16, 1, 1, 1), (2, 20, 1, 5, 2), (2, 16, 3, 70, 2), (1, 16, 7, 66, 1), (1, 16, 9, 130, 2))
     for e in ("bn-relu", "bn-none-signed-out")])

CASES["pointwise1x1"] = (
    [case(PW, P._pwconv_case, case=c, mode=m, form=f) for f, c in PW_FORMS for m in PW_MODES] +
    [case(PW, P.test_pwconv_i8_residual_vs_oracle, form=f, case=c, mode=m)
     for f, c in (("split", (2, 144, 24, 14, 14)), ("split", (3, 384, 64, 7, 7)), (None, (2, 128, 512, 9, 11)),
                  ("stream", (2, 64, 256, 28, 28)), ("sample", (2, 512, 1024, 8, 8)))
     for m in ("online_u8_bn_relu", "offline_s8_channel_w4_bn_none")] +
    [case(PW, P.test_pwconv_i8_residual_partial_tile_statistic_ignores_the_next_sample, case=c)
     for c in ((3, 144, 24, 14, 14), (4, 192, 40, 7, 7))] +
    [case(PW, P.test_pwconv_i8_stride2_vs_oracle, case=c, mode=m)
     for c in ((2, 64, 128, 9, 11), (4, 96, 40, 6, 7)) for m in ("online_u8_bn_relu", "offline_s8_channel_w4")] +
    [case(PW, SUB2.test_sub2_stores_the_even_pixels_of_the_whole_launch_and_keeps_its_statistic, case=c, mode=m)
     for c in ((3, 64, 160, 9, 13), (9, 40, 192, 5, 6), (2, 128, 256, 1, 8))
     for m in ("online_u8_bn_res_relu", "offline_u8_bn_res_relu", "online_u8_bias_nores_relu6")] +
    [case(PW, SUB2.test_dual_sub2_stores_both_outputs_subsampled, case=(3, 64, 256, 9, 11))] +
    [case("pwconv_i8_shortcut " + PW, SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin, case=c, mode=m)
     for c in ((2, 64, 64, 256, 5, 3), (9, 256, 512, 1024, 7, 7)) for m in ("online_u8_relu", "offline_u8_relu", "mixed_relu6_bias")] +
    [case("pwconv_i8_shortcut " + PW, SC.test_folded_shortcut_under_stored_thresholds_equals_the_two_launches, case=c)
     for c in ((9, 256, 512, 1024, 7, 7, False), (5, 256, 512, 1024, 14, 14, True))] +
    [case("pwconv_i8_gap global_avg_pool_stat " + PW, GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, case=c, mode=m)
     for c in ((5, 512, 512, 7, 7, False), (4, 512, 2048, 7, 7, True), (3, 512, 1024, 8, 8, False))
     for m in ("online_u8_bn_relu", "offline_u8_bias_relu6")] +
    [case(PW, C16.test_pointwise_producer_writes_the_consumers_codes, case=c, mode=m)
     for c in ((3, 16, 96, 9, 11, 1), (2, 96, 40, 5, 6, 1), (2, 256, 512, 8, 8, 2)) for m in ("u8-out", "s8-out-relu")] +
    [case(PW, C16.test_pointwise_consumer_of_codes_equals_consumer_of_fp32, case=c, mode=m)
     for c in ((3, 16, 96, 9, 11, 1), (2, 144, 24, 7, 7, 1), (2, 256, 512, 8, 8, 2)) for m in ("u8_bn_relu", "s8_res")] +
    [case(PW, C16.test_pointwise_between_two_code_tensors, case=(2, 256, 64, 9, 11, 1)),
     case(PW, C16.test_closing_pointwise_stores_the_trunk_twice, case=(3, 64, 256, 9, 11))])

CASES["recompute_pair"] = [
    case("pwconv_i8_stat pwdw_fused pwconv_i8 dwconv3x3 weight_codes weight_fake_quant absmax_per_sample", _pair, case=c, mode=m)
    for c in PAIR_CASES for m in ("online_u8_bn_relu", "offline_u8_bn_relu")]

CASES["dense3x3"] = (
    [case("conv3x3_i8 weight_codes", P.test_conv3x3_i8_vs_oracle, case=c, mode=m)
     for c in C3_SHAPES for m in ("online_u8_bn_relu", "offline_s8_channel_w4", "online_s8_bias")] +
    [case("conv3x3_i8 weight_slices_3x3", P.test_conv3x3_i8_sliced_vs_oracle, case=c, mode=m)
     for c in C3_SHAPES for m in ("online_u8_bn_relu_wino", "offline_s8_bias")] +
    [case("conv3x3_i8 weight_codes", C16.test_dense3x3_with_codes_on_both_sides, case=c, signed=sg)
     for c in C3_SHAPES for sg in (False, True)])

CASES["head"] = (
    [case("dense_i8_eval pwconv_i8 weight_codes", P.test_dense_i8_eval_vs_oracle, n=n, cin=ci, units=u, mode=m)
     for n, ci, u in ((7, 64, 10), (1, 512, 3), (70, 100, 37)) for m in ("online", "offline_channel_w4")] +
    [case("eval_counters", P.test_eval_counters_vs_oracle, n=n, classes=c) for n, c in ((1, 1), (7, 10), (300, 37))] +
    [case("gemm_i8_codes", P.test_gemm_i8_codes_is_exact, n=n, l=l, k=k, cout=co, zoff=z)
     for n, l, k, co, z in ((1, 7, 9, 5, 128), (1, 33, 64, 33, 0), (2, 49, 27, 32, 128))])

CASES["weights"] = (
    [case("weight_codes", _weight_codes, shape=s) for s in ((5, 9001), (3, 8193), (64, 3, 7, 7), (8, 4, 3, 3))] +
    [case("weight_fake_quant", P.test_weight_vs_oracle_real_layer_shapes, shape=s, rows=r)
     for s, r in (((5, 9001), 5), ((3, 8193), 3), ((64, 3, 7, 7), 64), ((64, 3, 7, 7), 1))] +
    [case("weight_fake_quant", P.test_weight_golden),
     case("weight_codes weight_slices_3x3", _weights_3x3, shape=(8, 4, 3, 3)),
     case("weight_codes weight_slices_3x3", _weights_3x3, shape=(70, 8, 3, 3)),
     case("wino_weight_fake_quant", _wino_weight, shape=(8, 4, 3, 3)),
     case("wino_weight_fake_quant", P.test_winograd_golden, variant="F43")])

CASES["calibration_and_codes"] = (
    [case("global_max histogram_accumulate hist_to_float", P.test_histogram_golden, name=n) for n in ("halfnormal", "tiny_range", "shape4d")] +
    [case("global_max histogram_accumulate hist_to_float", _calibration_unaligned),
     case("histogram_accumulate", P.test_histogram_counts_negatives_and_clamps_last_bin),
     case("kl_search", _kl_search),
     case("quantize_codes dequantize", _codes_roundtrip)])

CASES["qconv2d"] = (
    [case("qconv2d qconv_weights qconv_workspace", _qconv_direct, which=i, in_dt=a, w_dt=b)
     for i, a, b in ((1, "uint8", "int8"), (3, "int8", "uint8"), (4, "uint8", "int8"))] +
    [case("qconv2d qconv_weights qconv_workspace", QC.test_pointwise_on_the_matrix_cores, case=(3, 24, 20, 40)),
     case("qconv2d qconv_weights qconv_workspace", QC.test_pointwise_on_the_matrix_cores, case=(2, 96, 9, 200)),
     case("qconv2d qconv_weights qconv_workspace", QC.test_dense3x3_on_the_matrix_cores, case=(3, 64, 9, 13, 96)),
     case("qconv2d qconv_weights qconv_workspace", QC.test_depthwise_on_integer_codes, case=(3, 40, 10, 10, 1)),
     case("qconv2d qconv_weights qconv_workspace", QC.test_depthwise_on_integer_codes, case=(2, 24, 19, 23, 2)),
     case("qconv2d qconv_weights qconv_workspace", QC.test_range_from_the_producers_statistic_and_folded_batchnorm)])


def covered_entry_points():
    """Names of the entry points of ops.py that some case of the table runs (tests/test_poison_harness.py)."""
    return {e for cases in CASES.values() for c in cases for e in c.entries}


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


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
def test_the_harness_sees_device_memory(dev, ops, monkeypatch, pattern):
    """On the device as on the CPU (tests/test_poison_harness.py): what `ops` allocates is the pattern until a kernel writes
    it, a guarded input is its values between poison, and one element stored past a body is reported."""
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    ws = ops._workspace(dev, 100)
    assert ws.numel() == 1 << 16 and bool((ws == pattern).all()) and len(proxy.records) == 1
    ops._WS.clear()
    stat, _ = ops._stat_target(3, dev, True)
    assert stat.is_cuda and stat.view(torch.uint8).tolist() == [pattern] * 12
    x = proxy.guarded(np.float32([[1, -2, 3]]), dev)
    raw, g, body = proxy.records[-1][:3]
    assert body == 12 and N(raw[g - 4:g + 16].view(torch.uint8)).tolist() == [pattern] * 4 + list(np.float32([1, -2, 3]).view(np.uint8)) + [pattern] * 4
    y = ops.absmax_per_sample(x)
    torch.cuda.synchronize()
    assert N(y).tolist() == [3.0] and proxy.guards_intact() is True
    torch.as_strided(y, (2,), (1,))[1] = 0.0                 # inside the raw buffer, one element past the body
    torch.cuda.synchronize()
    with pytest.raises(poison.GuardError, match=r"float32, shape \(1,\), 4 bytes\): guard after the body changed, first at byte offset 4 "):
        proxy.guards_intact()


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
@pytest.mark.parametrize("family", list(CASES))
def test_family_under_poison(dev, ops, golden, monkeypatch, family, pattern):
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    for mod in DRIVER_MODULES:
        for name in ("T", "_t"):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, lambda a, d, _p=proxy: None if a is None else _p.guarded(a, d))
    ran = 0
    for c in CASES[family]:
        ops._WS.clear()                                  # the scratch cache is taken anew, poisoned, in every case
        kw = dict(c.kwargs)
        if "golden" in inspect.signature(c.driver).parameters:
            kw["golden"] = golden
        try:
            c.driver(dev=dev, ops=ops, **kw)
            torch.cuda.synchronize()
            proxy.guards_intact()
            assert proxy.records, "the case took neither an input nor an allocation from the proxy: it checks nothing here"
        except AssertionError as e:
            raise AssertionError("pattern 0x%02X, %s: %s" % (pattern, _describe(c), e)) from e
        proxy.release()
        ran += 1
    ops._WS.clear()
    assert ran == len(CASES[family])
