"""Kernel families on tensors past 2 GiB and 4 GiB ("Large tensors"; helpers and the two references:
tests/big_tensors.py).

The kernels carry 32-bit lane offsets, buffer resources clamped to 4 GiB - 1, windows capped below 2 GiB and the lane offset 2^31
as "outside every resource", and the host guards that keep a shape on the right side of each.  Every case here puts ONE tensor of
a launch just past such a limit (or at the last shape before it), draws every sample differently, takes outputs from poisoned
memory, and compares bit for bit: the selected samples with the host twin, every sample with the same entry point on sub-batches
of at most 256 MB.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import big_tensors as B
import poison
from oracle import fq_oracle as O
from oracle import host as H
from quantization.mxnet_amd._lib import FakeQuantError

pytestmark = pytest.mark.gpu

GIB = B.GIB


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32)) if got.dtype == np.float32 \
            else np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError("%s: %d of %d elements differ, first at flat index %d: %r vs %r"
                             % (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


# ---- fq_pwconv_i8 -------------------------------------------------------------------------------------------------------------
# 112 x 112 planes: 16 -> 64 writes 3 211 264 bytes per sample (4 GiB at n = 1337.5), 64 -> 32 reads as many; 24 -> 40 (ragged on both
# sides: the thin instantiations) writes 2 007 040 (2 GiB at n = 1069.98, 4 GiB at 2139.96).
# (form, n, cin, cout, h, w, residual, online, what must hold the shape, boundaries some tensor of the case contains)
# (a NAMED form is pinned - a shape it does not take raises; under the library's choice the form in the comment is what the
# dispatcher picks today and is not asserted: the case then pins the values of whatever form takes the shape)
PW_CASES = [
    # the streaming form at the last batch its 32-bit lane offsets reach: y ends 1.5 MB below 4 GiB, and past 2 GiB all the way
    ("stream", 1337, 16, 64, 112, 112, False, False, "named", (1 << 31,)),
    (None, 1337, 16, 64, 112, 112, False, True, "stream takes it by the library's choice too", (1 << 31,)),
    ("stream", 1337, 64, 32, 112, 112, False, False, "named", (1 << 31,)),
    # ... and the first batches past it: the split form, whose resources are re-based per workgroup, takes the shape
    (None, 1340, 16, 64, 112, 112, False, False, "split", (1 << 31, 1 << 32)),
    (None, 1340, 64, 32, 112, 112, False, False, "split", (1 << 31, 1 << 32)),
    (None, 1340, 16, 64, 112, 112, True, False, "split", (1 << 31, 1 << 32)),
    ("split", 1340, 16, 64, 112, 112, False, True, "named", (1 << 31, 1 << 32)),
    # thin instantiations (ragged Cin and Cout, masked channel tile): the last batch whose output stays within 2 GiB, where the
    # masking lane offset 2^31 is still outside the resource; the first past it and the last below 4 GiB, where the split form
    # (windows below 2 GiB) must take over; and past 4 GiB
    ("stream", 1069, 24, 40, 112, 112, False, False, "named: the thin instantiations are the streaming form's", ()),
    # ... ragged Cin alone (Cout % 32 == 0: no masked channel) stays with the thin instantiations up to 4 GiB - the whole-tensor
    # resource and the 32-bit output offsets at 4 293 459 968 bytes of y
    ("stream", 1337, 24, 64, 112, 112, False, False, "named: thin, the last batch below 4 GiB", (1 << 31,)),
    (None, 1071, 24, 40, 112, 112, True, False, "split", (1 << 31,)),
    (None, 2139, 24, 40, 112, 112, False, False, "split", (1 << 31,)),
    (None, 2142, 24, 40, 112, 112, False, False, "split", (1 << 31, 1 << 32)),
]


def _pw_id(c):
    form, n, cin, cout, h, w, res, online = c[:8]
    return "%s-%dx%d->%d@%dx%d%s%s" % (form or "auto", n, cin, cout, h, w, "+res" if res else "", "-online" if online else "")


@pytest.mark.parametrize("case", PW_CASES, ids=[_pw_id(c) for c in PW_CASES])
def test_pointwise_past_the_limits(dev, ops, monkeypatch, case):
    form, n, cin, cout, h, w, with_res, online, _, edges = case
    hw = h * w
    cin_pad = (cin + 63) // 64 * 64
    sizes = [4 * cin * hw, 4 * cout * hw, cin_pad * hw] + ([4 * cout * hw] if with_res else [])
    assert tuple(B.crossed(n, sizes)) == tuple(edges), "the case does not sit where its comment says"
    rng = np.random.default_rng(n + cin + cout)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + cin).t
        res = B.Drawn((n, cout, h, w), dev, seed=n + cout + 1, signed=True, scale=3.0).t if with_res else None
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
        bn = dict(bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        if online:
            stat_in = ops.absmax_per_sample(x)
            cur = torch.zeros(1, device=dev)
            y, stat = ops.pwconv_i8(x, codes, scales, rowsum, in_stat=stat_in, cur_out=cur, form=form, residual=res, **bn)
            hstat = B.host(stat_in)
            thr = np.float32(O.batch_mean(hstat))
            _same(B.host(cur), np.float32([thr]), "current_input_max vs the oracle's batch mean of the %d statistics" % n)
            _same(hstat[sel], H.absmax_per_sample(B.host(x, sel)), "in_stat of the selected samples")
        else:
            thr = np.float32(5.5)
            y, stat = ops.pwconv_i8(x, codes, scales, rowsum, in_thr=_t(np.float32([thr]), dev), form=form, residual=res, **bn)
        thr_t = _t(np.float32([thr]), dev)
        keep = len(proxy.records)
        # reference 2: every sample, against the launches the rest of the suite holds to the oracle (the library's own choice of form)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.pwconv_i8(x[lo:hi], codes, scales, rowsum, in_thr=thr_t, residual=None if res is None else res[lo:hi], **bn)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        # reference 1: the host twin on the selected samples
        want, wstat = H.pwconv_i8(B.host(x, sel), wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu",
                                  residual=None if res is None else B.host(res, sel), want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del x, res, y, stat


def test_streaming_form_named_past_4_gib_is_refused(dev, ops):
    """`form="stream"` on a tensor its 32-bit lane offsets do not reach: refused with the form's message, nothing launched (the
    library's own choice hands the shape to the split form: PW_CASES)."""
    B.need_free_memory()
    n, cin, cout, h, w = 1338, 16, 64, 112, 112
    rng = np.random.default_rng(0)
    wt = rng.standard_normal((cout, cin, 1, 1)).astype(np.float32)
    codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
    x = torch.zeros((n, cin, h, w), device=dev)
    with pytest.raises(FakeQuantError, match="does not fit the streaming kernel"):
        ops.pwconv_i8(x, codes, scales, rowsum, in_thr=_t(np.float32([1.0]), dev), form="stream")
    del x
    torch.cuda.empty_cache()


# ---- the streaming families (fq_stream.hip, fq_calib.hip): flat chunked walks whose chunk arithmetic is the index itself -------
# (n, inner): numel just past 2^30 (4 GiB) - and, where named, just past 2^31 elements (8.6 GB: one tensor, read or in place)
S30 = (1028, 1 << 20)
S31 = (2052, 1 << 20)


def _stream_shapes(both):
    return [pytest.param(S30, id="numel-2^30"), pytest.param(S31, id="numel-2^31")] if both else [pytest.param(S30, id="numel-2^30")]


@pytest.mark.parametrize("shape", _stream_shapes(True))
def test_absmax_per_sample_past_the_limits(dev, ops, monkeypatch, shape):
    n, inner = shape
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(shape, dev, seed=n, signed=True)
        sel = B.picks(n, [4 * inner])
        B.assert_distinct(d.t, sel)
        stat = ops.absmax_per_sample(d.t)
        raw = ops.absmax_per_sample(d.t, no_abs=True)
        keep = len(proxy.records)
        for lo, hi, p in d.replay():
            assert torch.equal(p, d.t[lo:hi]), "the replayed piece is not the drawn one"
            assert torch.equal(stat[lo:hi], ops.absmax_per_sample(p))
            assert torch.equal(raw[lo:hi], ops.absmax_per_sample(p, no_abs=True))
            B.drop(proxy, keep)
        xs = B.host(d.t, sel)
        _same(B.host(stat)[sel], O.absmax_per_sample(xs), "per-sample maxima")
        _same(B.host(raw)[sel], H.absmax_per_sample(xs, no_abs=True), "per-sample maxima, no abs")
        del d, stat, raw


@pytest.mark.parametrize("shape", _stream_shapes(True))
def test_fake_quant_offline_in_place_past_the_limits(dev, ops, monkeypatch, shape):
    n, inner = shape
    thr = np.float32(3.1)
    flags = ops.act_flags(signed=True)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(shape, dev, seed=n + 1, signed=True)
        sel = B.picks(n, [4 * inner])
        B.assert_distinct(d.t, sel)
        xs = B.host(d.t, sel)
        thr_t = _t(np.float32([thr]), dev)
        y, cur, _ = ops.fake_quant_offline(d.t, thr_t, 8, flags, out=d.t)
        assert y.data_ptr() == d.t.data_ptr()
        keep = len(proxy.records)
        stats = []
        for lo, hi, p in d.replay():
            stats.append(ops.absmax_per_sample(p).clone())
            ys, _, _ = ops.fake_quant_offline(p, thr_t, 8, flags, out=p)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            B.drop(proxy, keep)
        hy, _, _ = H.fake_quant_offline(xs, thr, 8, H.act_flags(signed=True))
        _same(B.host(y, sel), hy, "samples %s vs the host twin" % (sel,))
        # (the batch statistic an offline consumer reports on the side: the batch mean of all n per-sample maxima of the INPUT)
        _same(B.host(cur), np.float32([O.batch_mean(B.host(torch.cat(stats)))]), "current_max")
        del d, y, stats


def test_fake_quant_online_past_4_gib(dev, ops, monkeypatch):
    n, inner = S30
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(S30, dev, seed=7)
        sel = B.picks(n, [4 * inner])
        y, cur, _ = ops.fake_quant_online(d.t, 8, 0)
        stat = ops.absmax_per_sample(d.t)
        hstat = B.host(stat)
        thr = np.float32(O.batch_mean(hstat))
        _same(B.host(cur), np.float32([thr]), "current_max vs the oracle's batch mean of the %d statistics" % n)
        thr_t = _t(np.float32([thr]), dev)
        keep = len(proxy.records)
        for lo, hi, p in d.replay():
            ys, _, _ = ops.fake_quant_offline(p, thr_t, 8, 0)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch under the stored batch mean" % (lo, hi - 1)
            del ys
            B.drop(proxy, keep)
        hy, _, _ = H.fake_quant_offline(B.host(d.t, sel), thr, 8, 0)
        _same(B.host(y, sel), hy, "samples %s vs the host twin under that batch mean" % (sel,))
        del d, y


def test_quantize_codes_and_dequantize_past_4_gib(dev, ops, monkeypatch):
    n, inner = S30
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(S30, dev, seed=61, signed=True)
        d.t[n - 1, inner - 5] = -40.0                               # the range's end sits past every boundary
        sel = B.picks(n, [4 * inner])
        codes, r = ops.quantize_codes(d.t, "int8")
        _same(B.host(r), np.float32([-40.0, 40.0, np.float32(40.0) / np.float32(127.0)]), "range record")
        y = ops.dequantize(codes, r[2:3])
        keep = len(proxy.records)
        for lo, hi, p in d.replay():
            if hi == n:
                p[hi - lo - 1, inner - 5] = -40.0
            cs, _ = ops.quantize_codes(p, "scale", r.clone())
            assert torch.equal(codes[lo:hi], cs), "codes of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(y[lo:hi], ops.dequantize(cs, r[2:3])), "dequantised samples %d .. %d differ" % (lo, hi - 1)
            del cs
            B.drop(proxy, keep)
        hc, _ = H.quantize_codes(B.host(d.t, sel), "scale", B.host(r))
        _same(B.host(codes, sel), hc, "codes of samples %s vs the host twin" % (sel,))
        _same(B.host(y, sel), H.dequantize(hc, B.host(r)[2]), "dequantised samples vs the host twin")
        del d, codes, y


# (n, c, h, w) with numel just past 2^30: the channel of an element comes from a 32-bit index inside the sample
BN_SHAPE = (1028, 64, 128, 128)


@pytest.mark.parametrize("mode", ["plain", "residual", "histogram"])
def test_bn_act_stat_past_4_gib(dev, ops, monkeypatch, mode):
    n, c, h, w = BN_SHAPE
    rng = np.random.default_rng(5)
    sc, sh = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    sct, sht = _t(sc, dev), _t(sh, dev)
    bins = 2048
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(BN_SHAPE, dev, seed=11, signed=True)
        r = B.Drawn(BN_SHAPE, dev, seed=12, signed=True, scale=1.0) if mode == "residual" else None
        sel = B.picks(n, [4 * c * h * w])
        sink = part = None
        if mode == "histogram":
            sink, part = B.Sink(bins, 4.0, dev), B.Sink(bins, 4.0, dev)
        y, stat = ops.bn_act_stat(d.t, sct, sht, "relu", hist=sink, residual=None if r is None else r.t)
        keep = len(proxy.records)
        rr = r.replay() if r is not None else None
        positive = 0
        for lo, hi, p in d.replay():
            pr = next(rr)[2] if rr is not None else None
            ys, ss = ops.bn_act_stat(p, sct, sht, "relu", hist=part, residual=pr)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss)
            positive += int(torch.count_nonzero(ys))
            del ys, ss
            B.drop(proxy, keep)
        if mode == "histogram":
            assert torch.equal(sink.hist, part.hist) and int(sink.neg) == int(part.neg), "counts vs the sum of the sub-batch histograms"
            assert int(sink.hist.sum()) == positive, "every positive output is counted once"
        xs = B.host(d.t, sel)
        if mode == "residual":
            want = H.add_act(H.bn_act(xs, sc, sh, "none"), B.host(r.t, sel), "relu")
        else:
            want = H.bn_act(xs, sc, sh, "relu")
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], O.absmax_per_sample(want), "statistics vs the oracle")
        del d, r, y, stat


def test_add_act_stat_past_4_gib(dev, ops, monkeypatch):
    n, inner = S30
    with B.bounded(monkeypatch, ops, poison) as proxy:
        a, b = B.Drawn(S30, dev, seed=21, signed=True), B.Drawn(S30, dev, seed=22, signed=True)
        sel = B.picks(n, [4 * inner])
        y, stat = ops.add_act_stat(a.t, b.t, "relu")
        keep = len(proxy.records)
        rb = b.replay()
        for lo, hi, pa in a.replay():
            ys, ss = ops.add_act_stat(pa, next(rb)[2], "relu")
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss)
            del ys, ss
            B.drop(proxy, keep)
        want = H.add_act(B.host(a.t, sel), B.host(b.t, sel), "relu")
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], O.absmax_per_sample(want), "statistics vs the oracle")
        del a, b, y, stat


def test_bn_act_maxpool_stat_past_4_gib(dev, ops, monkeypatch):
    n, c, h, w = BN_SHAPE
    rng = np.random.default_rng(6)
    sc, sh = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    sct, sht = _t(sc, dev), _t(sh, dev)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(BN_SHAPE, dev, seed=31, signed=True)
        sel = B.picks(n, [4 * c * h * w, c * h * w])
        y, stat = ops.bn_act_maxpool_stat(d.t, sct, sht, "relu")
        keep = len(proxy.records)
        for lo, hi, p in d.replay():
            ys, ss = ops.bn_act_maxpool_stat(p, sct, sht, "relu")
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss)
            del ys, ss
            B.drop(proxy, keep)
        want, wstat = H.bn_act_maxpool(B.host(d.t, sel), sc, sh, "relu", want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics vs the host twin")
        del d, y, stat


def test_global_avg_pool_stat_past_4_gib(dev, ops, monkeypatch):
    # planes of 49 pixels (the LDS kernel) and of 16 384 (a thread per plane)
    for shape in ((21400, 1024, 7, 7), BN_SHAPE):
        n = shape[0]
        per = 4 * int(np.prod(shape[1:]))
        assert n * per > (1 << 32)
        with B.bounded(monkeypatch, ops, poison) as proxy:
            d = B.Drawn(shape, dev, seed=41, signed=True)
            sel = B.picks(n, [per])
            y, stat = ops.global_avg_pool_stat(d.t)
            keep = len(proxy.records)
            for lo, hi, p in d.replay():
                ys, ss = ops.global_avg_pool_stat(p)
                assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
                assert torch.equal(stat[lo:hi], ss)
                del ys, ss
                B.drop(proxy, keep)
            want, wstat = H.global_avg_pool(B.host(d.t, sel), want_stat=True)
            _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
            _same(B.host(stat)[sel], wstat, "statistics vs the host twin")
            del d, y, stat


@pytest.mark.parametrize("shape", _stream_shapes(True))
def test_global_max_and_histogram_past_the_limits(dev, ops, monkeypatch, shape):
    n, inner = shape
    bins = 2048
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn(shape, dev, seed=n + 51)
        # (one element that is the maximum, in the last sample: past every boundary)
        d.t[n - 1, inner - 3] = 77.0
        mx = ops.global_max(d.t)
        _same(B.host(mx), np.float32([77.0]), "global maximum")
        rng_max = _t(np.float32([6.0]), dev)
        hist = torch.zeros(bins, dtype=torch.int64, device=dev)
        neg = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.histogram_accumulate(d.t, rng_max, hist, neg)
        part = torch.zeros(bins, dtype=torch.int64, device=dev)
        pneg = torch.zeros(1, dtype=torch.int32, device=dev)
        want = np.zeros(bins, np.uint64)
        keep = len(proxy.records)
        first, positive = True, 0
        for lo, hi, p in d.replay():
            if hi == n:
                p[hi - lo - 1, inner - 3] = 77.0
            positive += int(torch.count_nonzero(p))
            ops.histogram_accumulate(p, rng_max, part, pneg)
            if first or hi == n:                                   # the host twin's counts of the first and the last piece
                hh, _ = H.histogram_accumulate(B.host(p), 6.0, bins)
                one = torch.zeros(bins, dtype=torch.int64, device=dev)
                ops.histogram_accumulate(p, rng_max, one, pneg)
                _same(B.host(one).astype(np.uint64), hh.astype(np.uint64), "counts of samples %d .. %d vs the host twin" % (lo, hi - 1))
                first = False
            B.drop(proxy, keep)
        assert torch.equal(hist, part), "counts vs the sum of the sub-batch histograms"
        assert int(hist.sum()) == positive and int(neg) == 0
        del d


# ---- fq_dwconv3x3 -------------------------------------------------------------------------------------------------------------
# The flat (28 x 28, 14 x 14, 7 x 7) and whole-plane (14 or 7 rows, other widths) forms address the WHOLE tensor through one
# resource and mask with the lane offset 2^31: their guard is n * c * h * w * 4 < 2^31, above it a column form (64-bit pointers)
# takes the shape.  The depthwise forms cannot be named per call: the form in each row is the dispatcher's choice today, not
# asserted.  (n, c, h, w, stride, online, form expected to hold it, boundaries inside x or y)
DW_CASES = [
    # 512 planes of 28 x 28 per sample = 1 605 632 bytes: 1337 samples = 2 146 729 984 < 2^31 <= 1338 samples = 2 148 335 616
    (1337, 512, 28, 28, 1, False, "flat, last shape below the guard", ()),
    (1337, 512, 28, 28, 2, True, "flat, last shape below the guard", ()),
    (1338, 512, 28, 28, 1, True, "four columns per lane, first shape above", (1 << 31,)),
    (1338, 512, 28, 28, 2, False, "four columns per lane, first shape above", (1 << 31,)),
    # 1024 planes of 14 x 16 per sample = 917 504 bytes: 2340 samples = 2 146 959 360 < 2^31 <= 2341 samples = 2 147 876 864
    (2340, 1024, 14, 16, 1, False, "whole planes, last shape below the guard", ()),
    (2341, 1024, 14, 16, 1, False, "four columns per lane, first shape above", (1 << 31,)),
    # the column forms past 4 GiB: 32 planes of 112 x 112 = 1 605 632 bytes per sample, 2678 samples = 4 299 882 496
    (2678, 32, 112, 112, 2, False, "four columns per lane", (1 << 31, 1 << 32)),
    (2678, 32, 112, 112, 1, False, "four columns per lane", (1 << 31, 1 << 32)),
    # ... one column per lane (rows of 30 floats): 512 planes of 30 x 30 = 1 843 200 bytes per sample, 2331 samples = 4 296 499 200
    (2331, 512, 30, 30, 1, False, "one column per lane", (1 << 31, 1 << 32)),
    (2331, 512, 30, 30, 2, False, "one column per lane", (1 << 31, 1 << 32)),
]


def _dw_id(c):
    return "%dx%d@%dx%d-s%d%s" % (c[0], c[1], c[2], c[3], c[4], "-online" if c[5] else "")


@pytest.mark.parametrize("case", DW_CASES, ids=[_dw_id(c) for c in DW_CASES])
def test_depthwise_on_both_sides_of_the_guards(dev, ops, monkeypatch, case):
    n, c, h, w, stride, online, _, edges = case
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    sizes = [4 * c * h * w, 4 * c * ho * wo]
    assert tuple(B.crossed(n, sizes)) == tuple(edges), "the case does not sit where its comment says"
    rng = np.random.default_rng(n + c + h)
    wt = (rng.standard_normal((c, 1, 3, 3)) * 0.5).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
    sh = rng.standard_normal(c).astype(np.float32)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, c, h, w), dev, seed=n + c).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        wtt = _t(wt, dev)
        bn = dict(bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu", stride=stride)
        if online:
            stat_in = ops.absmax_per_sample(x)
            cur = torch.zeros(1, device=dev)
            y, stat = ops.dwconv3x3(x, wtt, in_stat=stat_in, cur_out=cur, **bn)
            thr = np.float32(O.batch_mean(B.host(stat_in)))
            _same(B.host(cur), np.float32([thr]), "current_input_max vs the oracle's batch mean of the %d statistics" % n)
        else:
            thr = np.float32(4.7)
            y, stat = ops.dwconv3x3(x, wtt, in_thr=_t(np.float32([thr]), dev), **bn)
        thr_t = _t(np.float32([thr]), dev)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.dwconv3x3(x[lo:hi], wtt, in_thr=thr_t, **bn)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        want, wstat = H.dwconv3x3(B.host(x, sel), wt, stride=stride, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh,
                                  act="relu", want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twin's fmaf chain" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del x, y, stat


@pytest.mark.parametrize("n,what", [(1337, "flat form, last shape below the guard"), (1338, "four columns per lane, x past 2 GiB")])
def test_depthwise_statistic_pass_keeps_the_codes_of_x(dev, ops, monkeypatch, n, what):
    """`dwconv3x3(store=False, x_codes_out=)` on 512 planes of 28 x 28: the per-sample maxima of the launch that stores, and one
    byte per element of x - the code the quantise-on-load made of it."""
    c, h, w = 512, 28, 28
    rng = np.random.default_rng(n)
    wt = (rng.standard_normal((c, 1, 3, 3)) * 0.5).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
    sh = rng.standard_normal(c).astype(np.float32)
    thr = np.float32(4.7)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, c, h, w), dev, seed=n + 3).t
        sel = B.picks(n, [4 * c * h * w, c * h * w])
        wtt, thr_t = _t(wt, dev), _t(np.float32([thr]), dev)
        bn = dict(bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        buf = ops.torch.empty(ops.front_codes_shape(x.shape), dtype=torch.int8, device=dev)         # the proxy's: poisoned
        none, stat = ops.dwconv3x3(x, wtt, in_thr=thr_t, store=False, x_codes_out=buf, **bn)
        assert none is None
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, 4 * c * h * w):
            part = ops.torch.empty(ops.front_codes_shape(x[lo:hi].shape), dtype=torch.int8, device=dev)
            _, ss = ops.dwconv3x3(x[lo:hi], wtt, in_thr=thr_t, store=False, x_codes_out=part, **bn)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(buf[lo:hi], part), "codes of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del part, ss
            B.drop(proxy, keep)
        xs = B.host(x, sel)
        _, wstat = H.dwconv3x3(xs, wt, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu", want_stat=True)
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        codes = H.fake_quant_offline(xs, thr, 8, 0, want_codes=True, want_stat=False)[2]
        _same(B.host(buf, sel), (np.asarray(codes).astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(len(sel), c, h * w),
              "codes of samples %s vs the host quantiser" % (sel,))
        del x, buf, stat


# ---- the recompute pair: fq_pwconv_i8_stat and fq_pwdw_fused ------------------------------------------------------------------
def _pair_bytes(codes, cin, signed=False):
    """The bytes `pwconv_i8_stat(x_codes_out=)` keeps for the codes (n, cin, hw) of x: whole 32-channel slabs of 16-channel blocks,
    [n][block][pixel][16], channels past cin as the code of zero."""
    n, _, hw = codes.shape
    cb = 2 * ((cin + 31) // 32)
    full = np.zeros((n, cb * 16, hw), np.int64)
    full[:, :cin] = codes
    byte = ((full + 128 - (0 if signed else 128)) ^ 0x80) & 0xFF
    return byte.astype(np.uint8).view(np.int8).reshape(n, cb, 16, hw).transpose(0, 1, 3, 2)


# (n, cin, cout, h, w, what, boundaries inside x or the code buffer)
STAT_CASES = [
    # x between 2 and 4 GiB, the last 32-pixel tile ragged (32001 * 784 = 16 mod 32): 100 352 bytes per sample = 3 211 364 352
    (32001, 32, 64, 28, 28, "ragged last tile", (1 << 31,)),
    # the last shape below 4 GiB: 1 605 632 bytes per sample, 2674 samples = 4 293 459 968
    (2674, 32, 64, 112, 112, "last shape below the guard", (1 << 31,)),
    # a half-slab past Cin (16 channels), masked with the lane offset 2^31: the last shape whose x stays within 2 GiB
    # (802 816 bytes per sample, 2674 samples = 2 146 729 984) - the padding block of the code buffer holds the code of zero
    (2674, 16, 64, 112, 112, "masked half-slab, last shape inside its guard", ()),
]


@pytest.mark.parametrize("case", STAT_CASES, ids=["%dx%d->%d@%dx%d" % c[:5] for c in STAT_CASES])
def test_statistic_pass_of_the_pair_past_2_gib(dev, ops, monkeypatch, case):
    n, cin, cout, h, w, _, edges = case
    hw = h * w
    sizes = [4 * cin * hw, 2 * ((cin + 31) // 32) * 16 * hw]
    assert tuple(B.crossed(n, sizes)) == tuple(edges), "the case does not sit where its comment says"
    assert ops.pwdw_supported((n, cin, h, w), cout, 2), "the pair must take this shape"
    rng = np.random.default_rng(n + cin)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * 0.2).astype(np.float32)
    sc = ((0.5 + rng.random(cout)) * np.where(rng.random(cout) < 0.1, -1, 1)).astype(np.float32)
    sh = (rng.standard_normal(cout) * 0.3).astype(np.float32)
    thr = np.float32(4.25)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + cin + 2, scale=1.7).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        buf = ops.torch.empty(ops.pair_codes_shape(x.shape), dtype=torch.int8, device=dev)          # the proxy's: poisoned
        stat = ops.pwconv_i8_stat(x, codes, scales, rowsum, x_codes_out=buf, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(4 * cin * hw, 4 * cout * hw)):
            # the storing launch's statistic (what the pass stands for), and the pass itself on the sub-batch for the codes
            _, ss = ops.pwconv_i8(x[lo:hi], codes, scales, rowsum, **kw)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the storing sub-batch launch" % (lo, hi - 1)
            part = ops.torch.empty(ops.pair_codes_shape(x[lo:hi].shape), dtype=torch.int8, device=dev)
            s2 = ops.pwconv_i8_stat(x[lo:hi], codes, scales, rowsum, x_codes_out=part, **kw)
            assert torch.equal(stat[lo:hi], s2) and torch.equal(buf[lo:hi], part), \
                "codes of samples %d .. %d differ from the sub-batch pass" % (lo, hi - 1)
            del ss, s2, part
            B.drop(proxy, keep)
            ops._WS.clear()
        xs = B.host(x, sel)
        _, wstat = H.pwconv_i8(xs, wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu", want_stat=True)
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        hc = H.fake_quant_offline(xs, thr, 8, 0, want_codes=True, want_stat=False)[2]
        _same(B.host(buf, sel), np.ascontiguousarray(_pair_bytes(np.asarray(hc).reshape(len(sel), cin, hw), cin)),
              "code buffer of samples %s vs the host quantiser, padding included" % (sel,))
        del x, buf, stat


def test_statistic_pass_refuses_a_masked_half_slab_past_2_gib(dev, ops):
    """16 channels (a half-slab past Cin, masked with the lane offset 2^31) and x past 2 GiB: the pair is not taken - the layers
    run as the two storing launches - and the entry point itself refuses."""
    B.need_free_memory()
    n, cin, cout, h, w = 2675, 16, 64, 112, 112
    assert not ops.pwdw_supported((n, cin, h, w), cout, 1) and not ops.pwdw_supported((n, cin, h, w), cout, 2)
    assert ops.pwdw_supported((n - 1, cin, h, w), cout, 2)
    wt = np.random.default_rng(1).standard_normal((cout, cin, 1, 1)).astype(np.float32)
    codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
    x = torch.zeros((n, cin, h, w), device=dev)
    with pytest.raises(FakeQuantError, match="shape not taken"):
        ops.pwconv_i8_stat(x, codes, scales, rowsum, in_thr=_t(np.float32([1.0]), dev))
    del x
    torch.cuda.empty_cache()


# (n, cin, cout, h, w, stride, what, boundaries inside x, the code buffer or z)
PAIR_CASES = [
    # x at the last shape below 4 GiB (fq_pwdw.hip, pwdw_plan), stride 2: z = 2674 * 64 * 56 * 56 * 4 = 2 146 729 984 bytes
    (2674, 32, 64, 112, 112, 2, "x below 4 GiB", (1 << 31,)),
    # z at the last shape below 2^31 ELEMENTS, stride 1: 2674 * 64 * 112 * 112 = 2 146 729 984 elements, 8.6 GB
    (2674, 16, 64, 112, 112, 1, "z below 2^31 elements", (1 << 31, 1 << 32)),
]


@pytest.mark.parametrize("case", PAIR_CASES, ids=["%dx%d->%d@%dx%d-s%d" % c[:6] for c in PAIR_CASES])
def test_fused_pair_at_the_last_shape_its_guards_accept(dev, ops, monkeypatch, case):
    n, cin, cout, h, w, stride, _, edges = case
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    sizes = [4 * cin * h * w, 2 * ((cin + 31) // 32) * 16 * h * w, 4 * cout * ho * wo]
    assert tuple(B.crossed(n, sizes)) == tuple(edges), "the case does not sit where its comment says"
    assert ops.pwdw_supported((n, cin, h, w), cout, stride) and not ops.pwdw_supported((n + 1, cin, h, w), cout, stride)
    rng = np.random.default_rng(n + cin + stride)
    w1 = (rng.standard_normal((cout, cin, 1, 1)) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((cout, 1, 3, 3)) * 0.3).astype(np.float32)
    bn1 = ((0.5 + rng.random(cout)).astype(np.float32), (rng.standard_normal(cout) * 0.3).astype(np.float32))
    bn2 = ((0.5 + rng.random(cout)).astype(np.float32), (rng.standard_normal(cout) * 0.3).astype(np.float32))
    thr1, thr2 = np.float32(4.25), np.float32(3.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + cin + stride, scale=1.7).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes, scales, rowsum = ops.weight_codes(_t(w1, dev), cout, 8)
        w2q = ops.weight_fake_quant(_t(w2, dev), cout, 8)
        t1, t2 = _t(np.float32([thr1]), dev), _t(np.float32([thr2]), dev)
        kw = dict(in_thr=t1, pw_bn_scale=_t(bn1[0], dev), pw_bn_shift=_t(bn1[1], dev), pw_act="relu", mid_thr=t2, stride=stride,
                  dw_bn_scale=_t(bn2[0], dev), dw_bn_shift=_t(bn2[1], dev), dw_act="relu")
        buf = ops.torch.empty(ops.pair_codes_shape(x.shape), dtype=torch.int8, device=dev)
        ops.pwconv_i8_stat(x, codes, scales, rowsum, in_thr=t1, bn_scale=kw["pw_bn_scale"], bn_shift=kw["pw_bn_shift"], act="relu",
                           x_codes_out=buf)
        z, zstat = ops.pwdw_fused(x, codes, scales, rowsum, w2q, x_codes=buf, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            zs, ss = ops.pwdw_fused(x[lo:hi], codes, scales, rowsum, w2q, **kw)                  # (reads x itself)
            assert torch.equal(z[lo:hi], zs), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(zstat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del zs, ss
            B.drop(proxy, keep)
        y = H.pwconv_i8(B.host(x, sel), w1, cout, 8, in_max=thr1, signed=False, width=8, bn_scale=bn1[0], bn_shift=bn1[1], act="relu")
        want, wstat = H.dwconv3x3(y, B.host(w2q), None, stride, in_max=thr2, signed=False, width=8, bn_scale=bn2[0], bn_shift=bn2[1],
                                  act="relu", want_stat=True)
        _same(B.host(z, sel), want, "samples %s vs the host twins" % (sel,))
        _same(B.host(zstat)[sel], wstat, "statistics of samples %s vs the host twins" % (sel,))
        del x, buf, z, zstat


# ---- fq_conv3x3_i8 and fq_conv3x3_i8_sliced: pixel blocks re-based per workgroup ----------------------------------------------
# 64 -> 64 @56x56: 802 816 bytes per sample on both sides; 5353 samples = 4 297 474 048 bytes, input and output past 4 GiB
@pytest.mark.parametrize("sliced", [False, True], ids=["one-slice", "three-slices"])
def test_dense3x3_past_4_gib(dev, ops, monkeypatch, sliced):
    n, cin, cout, h, w = 5353, 64, 64, 56, 56
    sizes = [4 * cin * h * w, 4 * cout * h * w]
    assert B.crossed(n, sizes) == [1 << 31, 1 << 32]
    rng = np.random.default_rng(n + sliced)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    if sliced:
        wt = O.wino_weight_fake_quant(wt, "F43", 8)[0]
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    thr = np.float32(5.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + 7).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        wargs = ops.weight_slices_3x3(_t(wt, dev)) if sliced else ops.weight_codes_3x3(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        y, stat = ops.conv3x3_i8(x, *wargs, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.conv3x3_i8(x[lo:hi], *wargs, **kw)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        okw = dict(in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu", want_stat=True)
        xs = B.host(x, sel)
        want, wstat = H.conv3x3_i8_sliced(xs, wt, **okw) if sliced else H.conv3x3_i8(xs, wt, cout, 8, **okw)
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del x, y, stat


# ---- the other forms of fq_pwconv_i8 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["stride2", "sub2"])
def test_split_form_strided_and_subsampled_over_an_input_past_4_gib(dev, ops, monkeypatch, mode):
    """Only the split form reads a strided input or stores a subsampled output; its resources are re-based per workgroup.
    64 channels of 112 x 112: 3 211 264 bytes per sample, 1340 samples = 4 303 093 760."""
    n, cin, h, w = 1340, 64, 112, 112
    cout = 32 if mode == "stride2" else 160
    assert mode == "stride2" or ops.pwconv_sub2_supported(cin, cout)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    sizes = [4 * cin * h * w, 4 * cout * ho * wo]
    assert B.crossed(n, sizes)[-1] == 1 << 32
    rng = np.random.default_rng(n + cout)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    thr = np.float32(5.5)
    how = dict(stride=2) if mode == "stride2" else dict(subsample=True)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + cout).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu", **how)
        y, stat = ops.pwconv_i8(x, codes, scales, rowsum, **kw)
        assert tuple(y.shape) == (n, cout, ho, wo)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.pwconv_i8(x[lo:hi], codes, scales, rowsum, **kw)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        want, wstat = H.pwconv_i8(B.host(x, sel), wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu",
                                  want_stat=True, **how)
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del x, y, stat


# (form, n, cin, cout, h, w, what, boundaries inside x, y or the workspace)
FORM_CASES = [
    # two kernels: the code workspace is n * cin_pad * hw bytes - 64 * 12 544 = 802 816 per sample, 5351 samples = 4 295 868 416
    ("two_kernels", 5351, 3, 8, 112, 112, "workspace past 4 GiB", (1 << 31, 1 << 32)),
    # rows (planes of one pixel): one resource over x, n * cin * 4 < 2^31 - 2048 channels: 262 143 samples = 2 147 475 456 bytes
    ("rows", 262143, 2048, 1000, 1, 1, "last shape below the guard", ()),
    (None, 262143, 2048, 1000, 1, 1, "rows by the library's choice", ()),
    # ... 262 145 samples = 2 147 491 840 bytes: the split form takes over (32 samples per tile, statistic slots run out)
    (None, 262145, 2048, 1000, 1, 1, "split above the guard", (1 << 31,)),
]


@pytest.mark.parametrize("case", FORM_CASES, ids=["%s-%dx%d->%d@%dx%d" % ((c[0] or "auto",) + c[1:6]) for c in FORM_CASES])
def test_pointwise_forms_at_their_guards(dev, ops, monkeypatch, case):
    form, n, cin, cout, h, w, _, edges = case
    hw = h * w
    cin_pad = (cin + 63) // 64 * 64
    sizes = [4 * cin * hw, 4 * cout * hw, cin_pad * hw]
    assert tuple(B.crossed(n, sizes)) == tuple(edges), "the case does not sit where its comment says"
    rng = np.random.default_rng(n + cin)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    thr = np.float32(5.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + 9).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes, scales, rowsum = ops.weight_codes(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bias=_t(b, dev), act="relu")
        y, stat = ops.pwconv_i8(x, codes, scales, rowsum, form=form, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.pwconv_i8(x[lo:hi], codes, scales, rowsum, **kw)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        want, wstat = H.pwconv_i8(B.host(x, sel), wt, cout, 8, in_max=thr, signed=False, width=8, bias=b, act="relu", want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twin" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del x, y, stat


# ---- the first convolutions: per-sample resources, 64-bit sample bases -------------------------------------------------------
# 224 x 224 inputs.  3x3 -> 32: 1 605 632 output bytes per sample, 2675 samples = 4 295 065 600; 7x7 -> 64: 3 211 264, 1340 samples
@pytest.mark.parametrize("ks,cout,n", [(3, 32, 2675), (7, 64, 1340)], ids=["3x3->32", "7x7->64"])
def test_first_convolution_with_its_output_past_4_gib(dev, ops, monkeypatch, ks, cout, n):
    h = w = 224
    sizes = [4 * 3 * h * w, 4 * cout * (h // 2) * (w // 2)]
    assert B.crossed(n, sizes)[-1] == 1 << 32
    rng = np.random.default_rng(n + ks)
    wt = (rng.standard_normal((cout, 3, ks, ks)) * 0.3).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, 3, h, w), dev, seed=n + ks, signed=True, scale=1.0).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        wtt = _t(wt, dev)
        kw = dict(bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        y, stat = ops.stem_conv_s2(x, wtt, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.stem_conv_s2(x[lo:hi], wtt, **kw)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        want = H.stem_conv_s2(B.host(x, sel), wt, bn_scale=sc, bn_shift=sh, act="relu")
        _same(B.host(y, sel), want, "samples %s vs the host twin's fmaf chain" % (sel,))
        _same(B.host(stat)[sel], O.absmax_per_sample(want), "statistics of samples %s vs the oracle" % (sel,))
        del x, y, stat


# ---- the folded shortcut and the pooled producer ------------------------------------------------------------------------------
def test_folded_shortcut_past_2_gib_of_y(dev, ops, monkeypatch):
    """fq_pwconv_i8_shortcut, 64 / 64 -> 256 @56x56: 3 211 264 output bytes per sample, 669 samples = 2 148 335 616 - windows capped
    below 2 GiB and re-based per workgroup, on both sides of byte 2^31."""
    n, cin, cin2, cout, h, w = 669, 64, 64, 256, 56, 56
    assert ops.pwconv_shortcut_supported(cin, cin2, cout)
    sizes = [4 * cin * h * w, 4 * cin2 * h * w, 4 * cout * h * w]
    assert B.crossed(n, sizes) == [1 << 31]
    rng = np.random.default_rng(n)
    w1 = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    w2 = (rng.standard_normal((cout, cin2, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    bn1 = (rng.uniform(0.3, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32))
    bn2 = (rng.uniform(0.3, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32))
    thr1, thr2 = np.float32(5.5), np.float32(4.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + 1).t
        x2 = B.Drawn((n, cin2, h, w), dev, seed=n + 2).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        c1 = ops.weight_codes(_t(w1, dev), cout, 8)
        c2 = ops.weight_codes(_t(w2, dev), cout, 8)
        t1, t2 = _t(np.float32([thr1]), dev), _t(np.float32([thr2]), dev)
        k1 = dict(in_thr=t1, bn_scale=_t(bn1[0], dev), bn_shift=_t(bn1[1], dev), act="relu")
        k2 = dict(in_thr=t2, bn_scale=_t(bn2[0], dev), bn_shift=_t(bn2[1], dev))
        y, stat = ops.pwconv_i8_shortcut(x, *c1, x2=x2, wcodes2=c2[0], wscale2=c2[1], wsum2=c2[2], in_thr2=t2, bn_scale2=k2["bn_scale"],
                                         bn_shift2=k2["bn_shift"], **k1)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            sc_, _ = ops.pwconv_i8(x2[lo:hi], *c2, want_stat=False, **k2)                       # the two launches it stands for
            ys, ss = ops.pwconv_i8(x[lo:hi], *c1, residual=sc_, **k1)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the two sub-batch launches" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ" % (lo, hi - 1)
            del sc_, ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        short = H.pwconv_i8(B.host(x2, sel), w2, cout, 8, in_max=thr2, signed=False, width=8, bn_scale=bn2[0], bn_shift=bn2[1])
        want, wstat = H.pwconv_i8(B.host(x, sel), w1, cout, 8, in_max=thr1, signed=False, width=8, bn_scale=bn1[0], bn_shift=bn1[1],
                                  act="relu", residual=short, want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twins" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twins" % (sel,))
        del x, x2, y, stat


def test_pooled_producer_past_2_gib_of_x(dev, ops, monkeypatch):
    """fq_pwconv_i8_gap, 512 -> 512 @7x7 (per-sample resources, 64-bit sample bases): 100 352 input bytes per sample, 21 401
    samples = 2 147 633 152."""
    n, cin, cout, h, w = 21401, 512, 512, 7, 7
    assert ops.pwconv_gap_supported((n, cin, h, w), cout)
    sizes = [4 * cin * h * w, cin * h * w]
    assert B.crossed(n, sizes) == [1 << 31]
    rng = np.random.default_rng(n)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    thr = np.float32(5.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + 1).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        codes = ops.weight_codes(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        y, stat = ops.pwconv_i8_gap(x, *codes, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            full, _ = ops.pwconv_i8(x[lo:hi], *codes, want_stat=False, **kw)                    # the two launches it stands for
            ys, ss = ops.global_avg_pool_stat(full)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the two sub-batch launches" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ" % (lo, hi - 1)
            del full, ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        conv = H.pwconv_i8(B.host(x, sel), wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu")
        want, wstat = H.global_avg_pool(conv, want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twins" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twins" % (sel,))
        del x, y, stat


# ---- C16 code tensors past 4 GiB -----------------------------------------------------------------------------------------------
class DrawnCodes(object):
    """An (n, C, h, w) activation as a C16 code tensor of unsigned 8-bit codes, drawn on the device piece by piece: every byte
    is a legal code (byte = code ^ 0x80), C a multiple of 16 so that no padding channel exists."""

    def __init__(self, shape, dev, seed):
        n, c, h, w = shape
        assert c % 16 == 0
        self.shape = tuple(shape)
        self.sample_bytes = c * h * w
        self.t = torch.empty((n, c // 16, h * w, 16), dtype=torch.int8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        for lo, hi in B.pieces(n, self.sample_bytes):
            self.t[lo:hi] = torch.randint(-128, 128, (hi - lo,) + tuple(self.t.shape[1:]), dtype=torch.int8, device=dev, generator=g)

    def values(self, sel, thr):
        """fp32 values of the samples `sel`: code * fp32(thr / 255), what a consumer of the codes dequantises."""
        n, c, h, w = self.shape
        codes = O.from_c16(B.host(self.t, sel), c, h, w, 128)
        return (codes.astype(np.float32) * O.act_scale(thr, False, 8)).astype(np.float32)


def _c16_of(want, thr2):
    return O.to_c16(O.ste_codes(want, O.act_scale(thr2, False, 8), thr2, np.float32(0)).astype(np.int64), 128)


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_between_code_tensors_past_4_gib(dev, ops, monkeypatch, stride):
    """fq_dwconv3x3_c16, 32 channels of 112 x 112: 401 408 code bytes per sample, 10 701 samples = 4 295 467 008 (stride 1: as many
    out).  Resources per workgroup on 64-bit bases, lanes without an output masked with the lane offset 2^31."""
    n, c, h, w = 10701, 32, 112, 112
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    sizes = [c * h * w, c * ho * wo]
    assert B.crossed(n, sizes)[-1] == 1 << 32
    rng = np.random.default_rng(n + stride)
    wt = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
    sh = rng.standard_normal(c).astype(np.float32)
    thr, thr2 = np.float32(5.5), np.float32(3.7)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = DrawnCodes((n, c, h, w), dev, seed=n + stride)
        sel = B.picks(n, sizes)
        B.assert_distinct(d.t, sel)
        thr_t, thr2_t, wtt = _t(np.float32([thr]), dev), _t(np.float32([thr2]), dev), _t(wt, dev)
        kw = dict(stride=stride, in_thr=thr_t, width=8, flags=0, bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu6",
                  out_codes=dict(thr=thr2_t, width=8, flags=0))
        y, stat = ops.dwconv3x3_c16(ops.Codes16(d.t, d.shape, thr_t, 8, 0), wtt, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.dwconv3x3_c16(ops.Codes16(d.t[lo:hi], (hi - lo, c, h, w), thr_t, 8, 0), wtt, **kw)
            assert torch.equal(y.t[lo:hi], ys.t), "codes of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        want, wstat = H.dwconv3x3(d.values(sel, thr), wt, stride=stride, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh,
                                  act="relu6", want_stat=True)
        _same(B.host(y.t, sel), _c16_of(want, thr2), "codes of samples %s vs the host twin's fmaf chain, quantised by the oracle" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del d, y, stat


def test_dense3x3_between_code_tensors_past_4_gib(dev, ops, monkeypatch):
    """fq_conv3x3_i8_c16, 64 -> 64 @56x56 with codes on both sides: 200 704 bytes per sample, 21 401 samples = 4 295 266 304."""
    n, cin, cout, h, w = 21401, 64, 64, 56, 56
    sizes = [cin * h * w, cout * h * w]
    assert B.crossed(n, sizes) == [1 << 31, 1 << 32]
    rng = np.random.default_rng(n)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    thr, thr2 = np.float32(5.5), np.float32(40.0)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = DrawnCodes((n, cin, h, w), dev, seed=n)
        sel = B.picks(n, sizes)
        B.assert_distinct(d.t, sel)
        thr_t, thr2_t = _t(np.float32([thr]), dev), _t(np.float32([thr2]), dev)
        wargs = ops.weight_codes_3x3(_t(wt, dev), cout, 8)
        kw = dict(in_thr=thr_t, width=8, flags=0, bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu",
                  out_codes=dict(thr=thr2_t, width=8, flags=0))
        y, stat = ops.conv3x3_i8(ops.Codes16(d.t, d.shape, thr_t, 8, 0), *wargs, **kw)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.conv3x3_i8(ops.Codes16(d.t[lo:hi], (hi - lo, cin, h, w), thr_t, 8, 0), *wargs, **kw)
            assert torch.equal(y.t[lo:hi], ys.t), "codes of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        want, wstat = H.conv3x3_i8(d.values(sel, thr), wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh,
                                   act="relu", want_stat=True)
        _same(B.host(y.t, sel), _c16_of(want, thr2), "codes of samples %s vs the host twin, quantised by the oracle" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twin" % (sel,))
        del d, y, stat


def test_first_convolution_with_pooling_past_2_gib_of_x(dev, ops, monkeypatch):
    """fq_stem_conv7x7s2_pool at 224 x 224: 602 112 input bytes per sample, 3568 samples = 2 148 335 616.  `ops` allocates the
    unpooled tensor beside the pooled one (16 / 3 of x), so this is the batch the memory bound allows: x 2.15 GB + 11.46 GB + the
    pooled 2.86 GB = 16.47 GB of the 17.18 GB that 16 GiB are."""
    n, h, w = 3568, 224, 224
    assert ops.stem_pool_supported(h, w)
    sizes = [4 * 3 * h * w, 4 * 64 * 56 * 56]
    assert B.crossed(n, sizes) == [1 << 31]
    rng = np.random.default_rng(n)
    wt = (rng.standard_normal((64, 3, 7, 7)) * 0.3).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, 64).astype(np.float32)
    sh = rng.standard_normal(64).astype(np.float32)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, 3, h, w), dev, seed=n, signed=True, scale=1.0).t
        sel = B.picks(n, sizes)
        B.assert_distinct(x, sel)
        wtt = _t(wt, dev)
        kw = dict(bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu", pool=True)
        y, stat = ops.stem_conv_s2(x, wtt, **kw)
        # (the unpooled tensor `ops` allocates and the launch never touches: its guard bands are checked, then it is let go)
        B.guards_intact(proxy)
        spare = [i for i, r in enumerate(proxy.records) if r[4] == (n, 64, h // 2, w // 2)]
        assert len(spare) == 1
        del proxy.records[spare[0]]
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, max(sizes)):
            ys, ss = ops.stem_conv_s2(x[lo:hi], wtt, **kw)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        conv = H.stem_conv_s2(B.host(x, sel), wt, bn_scale=sc, bn_shift=sh, act="relu")
        want = O.bn_act_maxpool(conv, np.ones(64, np.float32), np.zeros(64, np.float32), "none")
        _same(B.host(y, sel), want, "samples %s vs the host twin's fmaf chain, pooled by the oracle" % (sel,))
        _same(B.host(stat)[sel], O.absmax_per_sample(want), "statistics of samples %s vs the oracle" % (sel,))
        del x, y, stat


# ---- the pair's front, chained and front-storing modes at the last shape their `_supported` functions accept -----------------
def _low_bytes(codes, shape):
    return (np.asarray(codes).astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(shape)


def test_front_mode_of_the_statistic_pass_at_its_guard(dev, ops, monkeypatch):
    """`dwconv3x3(store=False, x_codes_out=)` + `pwconv_i8_stat(front=)`, 32 -> 64 @112x112 at 2674 samples: the tensor the front
    layer stands for is 4 293 459 968 bytes, one sample more is refused.  Against the two storing launches on sub-batches and the
    host twins; the handed-over codes byte for byte."""
    n, cin, cout, h, w = 2674, 32, 64, 112, 112
    assert ops.pwconv_front_supported((n, cin, h, w), cout) and not ops.pwconv_front_supported((n + 1, cin, h, w), cout)
    hw = h * w
    sizes = [4 * cin * hw, cin * hw]
    assert B.crossed(n, sizes) == [1 << 31]
    rng = np.random.default_rng(n)
    dww = (rng.standard_normal((cin, 1, 3, 3)) * 0.4).astype(np.float32)
    w1 = (rng.standard_normal((cout, cin, 1, 1)) * 0.2).astype(np.float32)
    bnA = ((0.5 + rng.random(cin)).astype(np.float32), (rng.standard_normal(cin) * 0.3).astype(np.float32))
    bnB = ((0.5 + rng.random(cout)).astype(np.float32), (rng.standard_normal(cout) * 0.3).astype(np.float32))
    thrA, thrB = np.float32(4.5), np.float32(3.25)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        y0 = B.Drawn((n, cin, h, w), dev, seed=n + 5, scale=1.9).t
        sel = B.picks(n, sizes)
        B.assert_distinct(y0, sel)
        tA, tB, dwt = _t(np.float32([thrA]), dev), _t(np.float32([thrB]), dev), _t(dww, dev)
        wc = ops.weight_codes(_t(w1, dev), cout, 8)
        kA = dict(in_thr=tA, bn_scale=_t(bnA[0], dev), bn_shift=_t(bnA[1], dev), act="relu")
        kB = dict(in_thr=tB, bn_scale=_t(bnB[0], dev), bn_shift=_t(bnB[1], dev), act="relu")
        ycodes = ops.torch.empty(ops.front_codes_shape(y0.shape), dtype=torch.int8, device=dev)
        _, zstat = ops.dwconv3x3(y0, dwt, store=False, x_codes_out=ycodes, **kA)
        buf = ops.torch.empty(ops.pair_codes_shape(y0.shape), dtype=torch.int8, device=dev)
        front = dict(x_codes=ycodes, w=dwt, bn_scale=kA["bn_scale"], bn_shift=kA["bn_shift"], act="relu", in_thr=tA)
        pstat = ops.pwconv_i8_stat(y0, *wc, x_codes_out=buf, front=front, **kB)         # (x is never read: only its shape counts)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, 4 * max(cin, cout) * hw):
            z, zs = ops.dwconv3x3(y0[lo:hi], dwt, **kA)
            part = ops.torch.empty(ops.pair_codes_shape(z.shape), dtype=torch.int8, device=dev)
            ps = ops.pwconv_i8_stat(z, *wc, x_codes_out=part, **kB)
            assert torch.equal(zstat[lo:hi], zs) and torch.equal(pstat[lo:hi], ps), "statistics of samples %d .. %d differ" % (lo, hi - 1)
            assert torch.equal(buf[lo:hi], part), "codes of samples %d .. %d differ from the two storing launches" % (lo, hi - 1)
            del z, zs, part, ps
            B.drop(proxy, keep)
        ys = B.host(y0, sel)
        z, wz = H.dwconv3x3(ys, dww, in_max=thrA, signed=False, width=8, bn_scale=bnA[0], bn_shift=bnA[1], act="relu", want_stat=True)
        _, wp = H.pwconv_i8(z, w1, cout, 8, in_max=thrB, signed=False, width=8, bn_scale=bnB[0], bn_shift=bnB[1], act="relu", want_stat=True)
        _same(B.host(zstat)[sel], wz, "depthwise statistics of samples %s vs the host twin" % (sel,))
        _same(B.host(pstat)[sel], wp, "1x1 statistics of samples %s vs the host twins" % (sel,))
        hc = H.fake_quant_offline(ys, thrA, 8, 0, want_codes=True, want_stat=False)[2]
        _same(B.host(ycodes, sel), _low_bytes(hc, (len(sel), cin, hw)), "codes of the depthwise input vs the host quantiser")
        hz = H.fake_quant_offline(z, thrB, 8, 0, want_codes=True, want_stat=False)[2]
        _same(B.host(buf, sel), np.ascontiguousarray(_pair_bytes(np.asarray(hz).reshape(len(sel), cin, hw), cin)),
              "codes of the recomputed depthwise output vs the host twins")
        del y0, ycodes, buf, zstat, pstat


def test_chained_mode_of_the_fused_pair_at_its_guard(dev, ops, monkeypatch):
    """`pwdw_fused(store=False, mid_codes_out=)`, 16 -> 64 @112x112 at 2674 samples: 2 146 729 984 elements of the 1x1 output (its
    codes: as many bytes), one sample more is refused."""
    n, cin, cout, h, w = 2674, 16, 64, 112, 112
    assert ops.pwdw_chain_supported((n, cin, h, w), cout) and not ops.pwdw_chain_supported((n + 1, cin, h, w), cout)
    hw = h * w
    sizes = [4 * cin * hw, 32 * hw, cout * hw]
    assert B.crossed(n, sizes) == []
    rng = np.random.default_rng(n + 1)
    w1 = (rng.standard_normal((cout, cin, 1, 1)) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((cout, 1, 3, 3)) * 0.3).astype(np.float32)
    bn1 = ((0.5 + rng.random(cout)).astype(np.float32), (rng.standard_normal(cout) * 0.3).astype(np.float32))
    bn2 = ((0.5 + rng.random(cout)).astype(np.float32), (rng.standard_normal(cout) * 0.3).astype(np.float32))
    thr1, thr2 = np.float32(4.25), np.float32(3.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, h, w), dev, seed=n + 6, scale=1.7).t
        sel = B.picks(n, sizes) + [n // 2]
        B.assert_distinct(x, sel)
        wc = ops.weight_codes(_t(w1, dev), cout, 8)
        w2q = ops.weight_fake_quant(_t(w2, dev), cout, 8)
        t1, t2 = _t(np.float32([thr1]), dev), _t(np.float32([thr2]), dev)
        kw = dict(in_thr=t1, pw_bn_scale=_t(bn1[0], dev), pw_bn_shift=_t(bn1[1], dev), pw_act="relu", mid_thr=t2,
                  dw_bn_scale=_t(bn2[0], dev), dw_bn_shift=_t(bn2[1], dev), dw_act="relu")

        def run(xs):
            xc = ops.torch.empty(ops.pair_codes_shape(xs.shape), dtype=torch.int8, device=dev)
            ops.pwconv_i8_stat(xs, *wc, in_thr=t1, bn_scale=kw["pw_bn_scale"], bn_shift=kw["pw_bn_shift"], act="relu", x_codes_out=xc)
            mid = ops.torch.empty(ops.front_codes_shape((xs.shape[0], cout, h, w)), dtype=torch.int8, device=dev)
            none, zs = ops.pwdw_fused(xs, *wc, w2q, x_codes=xc, store=False, mid_codes_out=mid, **kw)
            assert none is None
            return mid, zs
        mid, zstat = run(x)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, 4 * cout * hw):
            m2, z2 = run(x[lo:hi])
            _, zs = ops.pwdw_fused(x[lo:hi], *wc, w2q, **kw)                                     # the storing launch's statistic
            assert torch.equal(zstat[lo:hi], z2) and torch.equal(zstat[lo:hi], zs), "statistics of samples %d .. %d differ" % (lo, hi - 1)
            assert torch.equal(mid[lo:hi], m2), "codes of samples %d .. %d differ from the sub-batch launch" % (lo, hi - 1)
            del m2, z2, zs
            B.drop(proxy, keep)
        y = H.pwconv_i8(B.host(x, sel), w1, cout, 8, in_max=thr1, signed=False, width=8, bn_scale=bn1[0], bn_shift=bn1[1], act="relu")
        _, wstat = H.dwconv3x3(y, B.host(w2q), None, 1, in_max=thr2, signed=False, width=8, bn_scale=bn2[0], bn_shift=bn2[1],
                               act="relu", want_stat=True)
        _same(B.host(zstat)[sel], wstat, "statistics of samples %s vs the host twins" % (sel,))
        hc = H.fake_quant_offline(y, thr2, 8, 0, want_codes=True, want_stat=False)[2]
        _same(B.host(mid, sel), _low_bytes(hc, (len(sel), cout, hw)), "codes of the 1x1 output vs the host twins")
        del x, mid, zstat


def test_front_storing_pointwise_at_its_guard(dev, ops, monkeypatch):
    """`pwconv_i8(front=)`, 256 -> 256 @28x28 at 5349 samples: the tensor the front layer stands for is 4 294 262 784 bytes, and so
    is y; one sample more is refused."""
    n, c, h, w = 5349, 256, 28, 28
    assert ops.pwconv_front_store_supported((n, c, h, w), c) and not ops.pwconv_front_store_supported((n + 1, c, h, w), c)
    hw = h * w
    sizes = [4 * c * hw, c * hw]
    assert B.crossed(n, sizes) == [1 << 31]
    rng = np.random.default_rng(n + 2)
    dww = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(np.float32)
    w1 = (rng.standard_normal((c, c, 1, 1)) * 0.1).astype(np.float32)
    bnA = ((0.5 + rng.random(c)).astype(np.float32), (rng.standard_normal(c) * 0.3).astype(np.float32))
    bnB = ((0.5 + rng.random(c)).astype(np.float32), (rng.standard_normal(c) * 0.3).astype(np.float32))
    thrA, thrB = np.float32(4.5), np.float32(3.25)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        y0 = B.Drawn((n, c, h, w), dev, seed=n + 7, scale=1.9).t
        sel = B.picks(n, sizes)
        B.assert_distinct(y0, sel)
        tA, tB, dwt = _t(np.float32([thrA]), dev), _t(np.float32([thrB]), dev), _t(dww, dev)
        wc = ops.weight_codes(_t(w1, dev), c, 8)
        kA = dict(in_thr=tA, bn_scale=_t(bnA[0], dev), bn_shift=_t(bnA[1], dev), act="relu")
        kB = dict(in_thr=tB, bn_scale=_t(bnB[0], dev), bn_shift=_t(bnB[1], dev), act="relu")
        ycodes = ops.torch.empty(ops.front_codes_shape(y0.shape), dtype=torch.int8, device=dev)
        ops.dwconv3x3(y0, dwt, store=False, x_codes_out=ycodes, **kA)
        front = dict(x_codes=ycodes, w=dwt, bn_scale=kA["bn_scale"], bn_shift=kA["bn_shift"], act="relu", in_thr=tA)
        y, stat = ops.pwconv_i8((n, c, h, w), *wc, front=front, **kB)
        keep = len(proxy.records)
        for lo, hi in B.pieces(n, 4 * c * hw):
            z, _ = ops.dwconv3x3(y0[lo:hi], dwt, want_stat=False, **kA)
            ys, ss = ops.pwconv_i8(z, *wc, **kB)
            assert torch.equal(y[lo:hi], ys), "samples %d .. %d differ from the two storing launches" % (lo, hi - 1)
            assert torch.equal(stat[lo:hi], ss), "statistics of samples %d .. %d differ" % (lo, hi - 1)
            del z, ys, ss
            B.drop(proxy, keep)
            ops._WS.clear()
        z = H.dwconv3x3(B.host(y0, sel), dww, in_max=thrA, signed=False, width=8, bn_scale=bnA[0], bn_shift=bnA[1], act="relu")
        want, wstat = H.pwconv_i8(z, w1, c, 8, in_max=thrB, signed=False, width=8, bn_scale=bnB[0], bn_shift=bnB[1], act="relu",
                                  want_stat=True)
        _same(B.host(y, sel), want, "samples %s vs the host twins" % (sel,))
        _same(B.host(stat)[sel], wstat, "statistics of samples %s vs the host twins" % (sel,))
        del y0, ycodes, y, stat


# ---- the sample form of fq_pwconv_i8: per-sample resources, 2 GiB samples ---------------------------------------------------
# Planes of 524 284 pixels (4096 blocks of 128 or 124 pixels: the last pixel tile of most blocks is ragged, so the masking lane
# offset 2^31 is live).  A sample cannot be cut into sub-batches here, so reference 2 is the two-kernel form (64-bit indices, no
# resource) on the same tensor, and the host twin - a 1x1 convolution is pixel-wise - sees three windows of 256 pixels per sample.
# (cin, cout, what, boundaries inside x or y)
SAMPLE_CASES = [
    # `fq_pw_sample.hip`: one sample of x below 2 GiB - 1024 channels: 2 147 467 264 bytes
    (1024, 256, "x: last plane below the guard", (1 << 31,)),
    # ... and one sample of y (a wavefront's window runs to the end of the sample) - 1024 output channels: 2 147 467 264 bytes
    (128, 1024, "y: last plane below the guard", (1 << 31,)),
]
SAMPLE_HW = 524284


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=["%d->%d" % c[:2] for c in SAMPLE_CASES])
def test_sample_form_on_samples_of_2_gib(dev, ops, monkeypatch, case):
    cin, cout, _, edges = case
    n, hw = 2, SAMPLE_HW
    sizes = [4 * cin * hw, 4 * cout * hw]
    assert max(sizes) < (1 << 31) <= max(sizes) // hw * (hw + 4) and tuple(B.crossed(n, sizes)) == tuple(edges)
    rng = np.random.default_rng(cin)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    sc = rng.uniform(0.3, 1.5, cout).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    thr = np.float32(5.5)
    with B.bounded(monkeypatch, ops, poison) as proxy:
        x = B.Drawn((n, cin, 1, hw), dev, seed=cin).t
        assert not torch.equal(x[0], x[1])
        codes = ops.weight_codes(_t(wt, dev), cout, 8)
        kw = dict(in_thr=_t(np.float32([thr]), dev), bn_scale=_t(sc, dev), bn_shift=_t(sh, dev), act="relu")
        y, stat = ops.pwconv_i8(x, *codes, form="sample", **kw)
        y2, stat2 = ops.pwconv_i8(x, *codes, form="two_kernels", **kw)
        assert torch.equal(y, y2), "the sample form differs from the two-kernel form"
        assert torch.equal(stat, stat2) and torch.equal(stat, torch.amax(y.view(n, -1), 1)), "statistic"
        del y2, stat2
        idx = torch.cat([torch.arange(a, a + 256) for a in (0, (hw // 2) // 128 * 128 - 130, hw - 256)]).to(dev)
        xs = x[:, :, :, idx].cpu().numpy()
        want = H.pwconv_i8(xs, wt, cout, 8, in_max=thr, signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu")
        _same(y[:, :, :, idx].cpu().numpy(), want, "three windows of 256 pixels of both samples vs the host twin")
        del x, y, stat


@pytest.mark.parametrize("cin,cout", [(1024, 256), (128, 1024)], ids=["x", "y"])
def test_sample_form_refuses_a_sample_of_2_gib(dev, ops, cin, cout):
    """One plane of four pixels more: 1024 channels are 2^31 bytes per sample of x (1024 -> 256) or of y (128 -> 1024) - the named
    form is refused with its message before anything is launched (the library's own choice falls through to the two-kernel
    form)."""
    B.need_free_memory()
    n, hw = 2, SAMPLE_HW + 4
    wt = np.random.default_rng(2).standard_normal((cout, cin, 1, 1)).astype(np.float32)
    codes = ops.weight_codes(_t(wt, dev), cout, 8)
    x = torch.zeros((n, cin, 1, hw), device=dev)
    with pytest.raises(FakeQuantError, match="the sample form takes"):
        ops.pwconv_i8(x, *codes, in_thr=_t(np.float32([1.0]), dev), form="sample")
    del x
    torch.cuda.empty_cache()


# ---- fq_qconv2d_forward past the range-mode limit of the one-launch forms ---------------------------------------------------
def test_qconv2d_on_a_plane_of_2_30_pixels_takes_the_exact_direct_form(dev, ops, monkeypatch):
    """nn.Conv2D(quantized=True), 1 -> 1 channel, 1x1, on ONE plane of 32768 x 32768 = 2^30 pixels (x and y 4 GiB each): the
    one-launch pointwise form takes planes below 2^30 pixels only (`fq_pwconv.hip`, pwconv_dispatch), so the exact direct kernel -
    64-bit indices throughout - must take the layer; it says so by leaving -1 in the statistic it does not keep.  Reference 2: the
    same call on bands of 2048 rows (256 MB, contiguous for one channel) under the same fixed input range, which the one-launch
    form takes; reference 1: the host twin on the rows at either end and around byte 2^31."""
    side = 32768
    rng_in = (0.0, 6.0)
    wt = np.float32([[[[0.75]]]])
    b = np.float32([0.3])
    with B.bounded(monkeypatch, ops, poison) as proxy:
        d = B.Drawn((side, side), dev, seed=87)                         # rows as "samples": drawn in pieces of 2048 rows
        x = d.t.view(1, 1, side, side)
        assert B.crossed(1, [4 * side * side]) == [1 << 31]
        wtt, bt = _t(wt, dev), _t(b, dev)
        geom = ((1, 1), (0, 0), 1)
        assert ops.qconv_kind(wt.shape, *geom) == "pointwise"
        wbuf = ops.qconv_weights(wtt, *geom)
        ws = ops.qconv_workspace(1, dev)
        y, stat = ops.qconv2d(x, wtt, wbuf, bt, *geom, ws, input_range=rng_in, act="relu", want_stat=True)
        assert float(stat[0]) == -1.0, "the exact direct form did not take the layer"
        keep = len(proxy.records)
        for lo, hi in B.pieces(side, 4 * side):
            ys, ss = ops.qconv2d(x[:, :, lo:hi], wtt, wbuf, bt, *geom, ws, input_range=rng_in, act="relu", want_stat=True)
            assert float(ss[0]) >= 0.0, "the band was expected to run the one-launch form"
            assert torch.equal(y[:, :, lo:hi], ys), "rows %d .. %d differ from the band's launch" % (lo, hi - 1)
            del ys, ss
            B.drop(proxy, keep)
        mid = (1 << 31) // (4 * side)
        rows = [0, 1, mid - 1, mid, mid + 1, side - 2, side - 1]
        idx = torch.as_tensor(rows, device=dev)
        want = H.qconv2d_forward(x[:, :, idx].cpu().numpy(), wt, b, (1, 1), (0, 0), 1, input_range=rng_in, act="relu")
        _same(y[:, :, idx].cpu().numpy(), want, "rows %s vs the host twin" % (rows,))
        del d, x, y, stat
