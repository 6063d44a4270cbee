"""Named value regimes for the drivers of the int8 families (tests/test_gpu_value_regimes.py, tests/test_value_regimes_host.py).

The drivers draw Gaussian data under thresholds near the data's maximum, so every value-dependent, wave-uniform branch of a
kernel - `fq_nonneg`, `q2.denom > 0`, `make_fast_quot(d).ok`, the exactness of the int32 -> fp32 conversion in the epilogue,
the scale against the epsilon of ste_func.py:39-41 - is taken on one side only.  A regime turns a driver's seeded input, its
weights and its thresholds into values that take the other side; `apply` does that right after the driver drew its data,
`check` asserts FROM THE ORACLE'S CODES that the regime did what its name says - before the driver compares anything, so that
a regime that no longer reaches its branch fails instead of passing vacuously.

`boundaries` is about rounding, not about a branch: Gaussian data essentially never lands within a few ulp of a quotient
k + 0.5, so the tie behaviour of the quantisers copied into the kernels (`v_cvt_rpi`, `copysign(0.49999997f)`, the fast
quotient) goes unseen.  The regime fills x with the fp32 neighbours of every (k + 0.5) * d under a stored threshold of its own
and plants that threshold as every sample's maximum, so an online launch divides by the same d.

A plain helper: numpy and the numpy oracle only, no device memory, no fixtures."""
import numpy as np

from oracle import fq_oracle as O

F32 = np.float32

INPUT = ("zero", "zero_sample", "eps_scale", "tiny", "subnormal", "huge", "saturated", "allones_divisor", "boundaries")
OUTPUT = ("out_saturated", "out_zero_codes", "out_allones_divisor")
STANDALONE = ("zero_sample", "eps_scale", "tiny", "subnormal", "huge")      # kernels without weights or a stored threshold
ALL = INPUT + OUTPUT

SATURATED_VALUE = F32(8.0)
SATURATED_THRESHOLD = F32(0.25)
BOUNDARY_THRESHOLD = F32(2.75)
BOUNDARY_NEIGHBOURS = 3                              # fp32 neighbours on either side of fp32((k + 0.5) * d)
_HALF_PRED = np.nextafter(F32(0.5), F32(0))          # the one quotient at which trunc(Q + 0.5f) and roundf(Q) differ
_SCALE = {"tiny": F32(2.0) ** -100, "subnormal": F32(1e-41), "huge": F32(2.0) ** 100}
_MIN_NORMAL = np.finfo(np.float32).tiny


def levels(signed, width=8):
    return (2 ** (width - 1) - 1) if signed else (2 ** width - 1)


def eps_factor(signed, width=8):
    """2^-27 for unsigned 8-bit codes: a maximum near 8 then gives a scale of about twice the epsilon of ste_func.py:39-41 and a
    largest code of about 180 of 255.  Fewer levels take a proportionally smaller power of two (2^-28 for 127 levels), so that
    the scale, not the maximum, keeps its place against the epsilon."""
    return F32(2.0 ** (-27 - int(np.round(np.log2(255.0 / levels(signed, width))))))


def divisor(thr, signed, width=8):
    """fp32(fp32(thr / levels) + 1e-10): what every quantiser divides by (ste_func.py:39-41)."""
    return F32(O.act_scale(thr, signed, width) + O.EPS)


def has_allones_significand(d):
    return int(np.asarray(d, F32).view(np.uint32)) & 0x7FFFFF == 0x7FFFFF


_ALLONES = {}


def allones_threshold(signed, width=8, near=None):
    """The fp32 threshold nearest to `near` (default: levels / 32 - 8 for unsigned, 4 for signed 8-bit codes, about the
    drivers' Gaussian maxima) whose divisor has an all-ones significand - found by walking the fp32 neighbours outwards, not
    pasted in."""
    key = (bool(signed), width, near)
    if key not in _ALLONES:
        L = F32(levels(signed, width))
        start = F32(float(L) / 32 if near is None else near)
        # the divisor just below a power of two, then the thresholds that divide to it
        d = np.nextafter(F32(2.0 ** np.round(np.log2(float(start) / float(L)))), F32(0))
        assert has_allones_significand(d)
        guess = F32(F32(d - O.EPS) * L)
        up = down = guess
        found = None
        for _ in range(1 << 12):
            for t in (up, down):
                if has_allones_significand(divisor(t, signed, width)):
                    found = t
                    break
            if found is not None:
                break
            up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(0))
        assert found is not None, "no threshold with an all-ones divisor near %r" % (start,)
        _ALLONES[key] = F32(found)
    return _ALLONES[key]


def saturate_rows(w, rps):
    """Rows 0 and 1 of a filter bank constant +m and -m, m the max|w| of their scale group (`rps` rows per scale): their codes
    are +L and -L at every width."""
    w = np.array(w, dtype=F32, copy=True)
    if w.shape[0] < 2:
        return w
    rows = w.shape[0]
    for r, sign in ((0, 1), (1, -1)):
        g = r // rps
        m = np.abs(w.reshape(rows, -1)[g * rps:(g + 1) * rps]).max()
        w[r] = F32(sign) * m
    return w


def saturated_input(x, signed, block=1):
    """x in {0, +8} (unsigned) or {-8, +8} (signed): seven of eight elements of the even samples at +8 (the sums of a
    constant-sign filter row go far beyond 2^24 with many distinct, odd values), one of eight in the odd samples (unsigned
    codes are stored as code - 128: there the kernel's own accumulator passes 2^24 with the OPPOSITE sign of the zoff * rowsum
    term it is re-centred with, their sum is small and exact - an epilogue that converted the two terms separately is off by
    one there, while at the large sums its double rounding happens to land on the same fp32 for every K <= 2048), pixel 0 of
    every sample all +8 (the largest sum there is; where a sample is one pixel, sample 0).  `block` = 3: the 3x3 corner of sample 0 as well - a dense 3x3 filter then meets nine taps of
    +8 at its centre."""
    x = np.asarray(x, F32)
    low = np.random.default_rng(x.size).random(x.shape) < 0.125
    low[1::2] = ~low[1::2]                          # odd samples: one of eight elements at +8
    y = np.where(low, -SATURATED_VALUE if signed else F32(0), SATURATED_VALUE).astype(F32)
    if y.ndim > 2 and y[0, 0].size > 1:
        y.reshape(y.shape[0], y.shape[1], -1)[:, :, 0] = SATURATED_VALUE
    else:
        y[0] = SATURATED_VALUE                      # planes of one pixel, rows of a matrix: sample 0 is that pixel
    if block > 1:
        y[0, :, :block, :block] = SATURATED_VALUE
    return y


def boundary_count(signed, width=8, lo_neg_max=None):
    """Rounding boundaries k + 0.5 between two codes of the clip range: L from 0 up, 2 L where the range starts at -max."""
    lo_neg = signed if lo_neg_max is None else lo_neg_max
    return (2 if lo_neg else 1) * levels(signed, width)


def boundary_table(signed, width=8, lo_neg_max=None):
    """(boundaries, 7) fp32: row k holds fp32((k + 0.5) * d), d the divisor of BOUNDARY_THRESHOLD, between its three fp32
    neighbours below and above, ascending - inputs whose quotient by d lies within a few ulp of the tie k + 0.5.  k runs over
    0 .. L-1, over -L .. L-1 where the clip range starts at -max."""
    L = levels(signed, width)
    lo_neg = signed if lo_neg_max is None else lo_neg_max
    d = np.float64(divisor(BOUNDARY_THRESHOLD, signed, width))
    mid = ((np.arange(-L if lo_neg else 0, L, dtype=np.float64) + 0.5) * d).astype(F32)
    cols = [mid]
    for _ in range(BOUNDARY_NEIGHBOURS):
        cols = [np.nextafter(cols[0], F32(-np.inf))] + cols + [np.nextafter(cols[-1], F32(np.inf))]
    table = np.stack(cols, axis=1).astype(F32)
    assert np.abs(table).max() < BOUNDARY_THRESHOLD
    return table


def reaches_half_pred(x, in_max, signed, width=8):
    """Whether an element of x has the fp32 quotient +-pred(0.5) exactly.  Every other fp32 |Q| < 2^23 has
    trunc(Q + 0.5f) == roundf(Q) (csrc/fq_common.h at round_half_away), so a quantiser that rounds that way is wrong on this
    quotient alone.  0.5 * d is exact in fp32 and its neighbours below step through the quotients in strides of
    2 / (significand of d) ulp: pred(0.5) is the first of them where that significand exceeds 4 / 3.  Under 2.75 it does
    for every level count 2^b - 1, b = 1 .. 8; under 2.5 it does for 3, 7 and 15 levels and not for 31, 63, 127 or 255."""
    q = (np.asarray(x, F32) / divisor(in_max, signed, width)).astype(F32)
    return bool((np.abs(q) == _HALF_PRED).any())


def _planted(x):
    """One element per sample - its last - carries the threshold of `boundaries`."""
    mask = np.zeros(x.shape, bool)
    mask.reshape(x.shape[0], -1)[:, -1] = True
    return mask


def boundary_input(x, signed, width=8, lo_neg_max=None):
    """x filled flat, boundary-major, by cycling through `boundary_table`; the last element of every sample is BOUNDARY_THRESHOLD
    instead (the fill passes over it), so that the per-sample maxima and their batch mean are that threshold exactly: an
    online launch divides by the very d a stored one does."""
    x = np.asarray(x, F32)
    mask = _planted(x)
    y = np.full(x.shape, BOUNDARY_THRESHOLD, F32)
    y[~mask] = np.resize(boundary_table(signed, width, lo_neg_max).reshape(-1), x.size - x.shape[0])
    return y


def apply(regime, x, signed, w=None, rps=None, thr=None, width=8, lo_neg_max=None):
    """-> (x, w, thr): the regime's input, weights and INPUT threshold.  `thr` None: the launch quantises online, and stays
    so unless the regime has a threshold of its own.  `thr` given: the launch works under a STORED threshold; a regime without
    one of its own then stores the batch mean of the per-sample maxima of its input - what a calibration run over such data
    leaves.  Output-side regimes and None leave all three alone (`output_threshold`)."""
    if regime is None or regime in OUTPUT:
        return x, w, thr
    assert regime in INPUT, regime
    x = np.asarray(x, F32)
    if thr is not None:
        thr = None if regime in ("saturated", "allones_divisor", "boundaries") else "batch mean"
    if regime == "eps_scale":
        x = (x * eps_factor(signed, width)).astype(F32)
    elif regime == "zero":
        x = np.zeros_like(x)
    elif regime == "zero_sample":
        x = x.copy()
        x[0] = 0
    elif regime in _SCALE:
        x = (x * _SCALE[regime]).astype(F32)
    elif regime == "saturated":
        dense3x3 = w is not None and np.ndim(w) == 4 and np.shape(w)[1] > 1 and np.shape(w)[2:] == (3, 3)
        x = saturated_input(x, signed, 3 if dense3x3 else 1)
        thr = SATURATED_THRESHOLD
        if w is not None:
            w = saturate_rows(w, rps)
    elif regime == "allones_divisor":
        thr = allones_threshold(signed, width)
    elif regime == "boundaries":
        x = boundary_input(x, signed, width, lo_neg_max)
        thr = BOUNDARY_THRESHOLD
    if isinstance(thr, str):
        thr = stored_threshold(x)
    return x, w, thr


def stored_threshold(x):
    return O.batch_mean(O.absmax_per_sample(x))


def stored(regime, x, signed, w=None, rps=None, thr=None, width=8, lo_neg_max=None):
    """`apply` for a launch whose input threshold is always a stored one (code tensors)."""
    assert thr is not None
    return apply(regime, x, signed, w, rps, thr, width, lo_neg_max)


def output_threshold(regime, y, signed, thr=None, width=8):
    """The OUTPUT threshold of a code-writing launch under an output-side regime; `y` is the fp32 output (the oracle's) the
    codes are taken of.  Any other regime: `thr` as given."""
    if regime not in OUTPUT:
        return thr
    if regime == "out_saturated":
        return F32(np.abs(np.asarray(y, F32)).max() / F32(64))
    if regime == "out_zero_codes":
        return F32(2.0) ** 40
    return allones_threshold(signed, width)


def max_isum(x, in_max, signed, w, rps, wt_width=8, width=8, lo_neg_max=None, taps=1):
    """Largest |integer sum| of rows 0 and 1 of `w` (the constant ones) over the oracle's codes of x.  taps = 9: dense 3x3 with
    zero padding."""
    lo_neg = signed if lo_neg_max is None else lo_neg_max
    cx = O.ste_codes(x, O.act_scale(in_max, signed, width), in_max, F32(-F32(in_max)) if lo_neg else F32(0)).astype(np.int64)
    cw = O.weight_codes(w, rps, wt_width)[0][:2].astype(np.int64)
    n, c = cx.shape[0], cx.shape[1]
    if taps == 1:
        return int(np.abs(np.einsum("oc,ncp->nop", cw, cx.reshape(n, c, -1))).max())
    h, wd = cx.shape[2:]
    pad = np.zeros((n, c, h + 2, wd + 2), np.int64)
    pad[:, :, 1:-1, 1:-1] = cx
    cw = cw.reshape(2, c, 3, 3)
    s = sum(np.einsum("oc,nchw->nohw", cw[:, :, ky, kx], pad[:, :, ky:ky + h, kx:kx + wd]) for ky in range(3) for kx in range(3))
    return int(np.abs(s).max())


def reaches_large_sums(k, signed, width=8, wt_width=8):
    """K * levels * L > 2^24: fully saturated codes on a constant filter row leave the range fp32 holds integers in."""
    return k * levels(signed, width) * (2 ** (wt_width - 1) - 1) > 2 ** 24


def check(regime, x, in_max, signed, width=8, lo_neg_max=None, w=None, rps=None, wt_width=8, taps=1):
    """The regime's condition, from the oracle's codes of `x` under the threshold `in_max` the launch quantises with.  Under
    `saturated`, wherever the shape can reach them (`reaches_large_sums`), the largest |integer sum| must pass 2^24."""
    if regime is None or regime in OUTPUT:
        return
    x = np.asarray(x, F32)
    L = levels(signed, width)
    lo_neg = signed if lo_neg_max is None else lo_neg_max
    in_max = F32(in_max)
    codes = O.ste_codes(x, O.act_scale(in_max, signed, width), in_max, F32(-in_max) if lo_neg else F32(0))
    assert np.isfinite(codes).all(), "%s: the oracle's codes are not finite" % regime
    top = np.abs(codes).max()
    if regime == "zero":
        assert not x.any() and in_max == 0 and divisor(in_max, signed, width) == O.EPS and top == 0
    elif regime == "zero_sample":
        assert not x[0].any() and (x.shape[0] == 1 or x[1:].any())
    elif regime == "eps_scale":
        assert 0.25 * L <= top <= 0.75 * L, "eps_scale: largest code %r of %d levels" % (top, L)
    elif regime in ("tiny", "subnormal"):
        assert x.any() and top == 0, "%s: a code is not 0 (largest %r)" % (regime, top)
        if regime == "subnormal":
            assert np.abs(x).max() < _MIN_NORMAL, "subnormal: a non-zero input is normal"
    elif regime == "huge":
        assert np.abs(x).max() > F32(2.0) ** 98 and top == L
    elif regime == "saturated":
        nz = x != 0
        ends = (np.abs(codes[nz]) == L) | (codes[nz] == 0) if not lo_neg else np.abs(codes[nz]) == L
        assert in_max == SATURATED_THRESHOLD and ends.mean() >= 0.95, "saturated: %.3f of the codes on a clip end" % ends.mean()
        assert (np.abs(codes[nz]) == L).any()
        if w is not None and np.asarray(w).shape[0] >= 2:
            cw = O.weight_codes(w, rps, wt_width)[0]
            Lw = 2 ** (wt_width - 1) - 1
            assert (cw[0] == Lw).all() and (cw[1] == -Lw).all(), "saturated: rows 0 and 1 are not +-%d" % Lw
            if reaches_large_sums(int(np.prod(np.asarray(w).shape[1:])), signed, width, wt_width):
                m = max_isum(x, in_max, signed, w, rps, wt_width, width, lo_neg_max, taps)
                assert m > 2 ** 24, "saturated: max|isum| = %d does not pass 2^24" % m
    elif regime == "allones_divisor":
        assert has_allones_significand(divisor(in_max, signed, width)), "allones_divisor: divisor of %r" % (in_max,)
    elif regime == "boundaries":
        assert in_max == BOUNDARY_THRESHOLD and O.batch_mean(O.absmax_per_sample(x)) == BOUNDARY_THRESHOLD
        mask = x == BOUNDARY_THRESHOLD                 # (the table's largest value lies below the threshold)
        n = int(mask.sum())
        assert n == x.shape[0] and mask.reshape(n, -1).any(axis=1).all(), "boundaries: one planted element per sample"
        nb = boundary_count(signed, width, lo_neg_max)
        groups = (x.size - n) // 7
        c = codes[~mask][:7 * groups].reshape(groups, 7)
        k = (np.arange(groups) % nb + (-L if lo_neg else 0)).reshape(groups, 1)
        straddles = ((c == k) | (c == k + 1)).all(axis=1) & (c == k).any(axis=1) & (c == k + 1).any(axis=1)
        assert straddles.all(), "boundaries: group %d (k = %d) has the codes %s" % (
            np.argmin(straddles), k[np.argmin(straddles), 0], sorted(set(c[np.argmin(straddles)].tolist())))
        seen = len(set(k[straddles, 0].tolist()))
        assert seen >= min(nb, groups), "boundaries: %d of %d boundaries straddled" % (seen, nb)
        assert seen == nb or x.size < 2 * 7 * nb + n
        # ... and where the whole table is there, the one quotient that tells roundf from trunc(Q + 0.5f)
        assert groups < nb or reaches_half_pred(x[~mask], in_max, signed, width), "boundaries: no quotient is pred(0.5)"


def check_output(regime, y, thr, signed, width=8):
    """Condition of an output-side regime, from the oracle's output codes of `y` under `thr`."""
    if regime not in OUTPUT:
        return
    L = levels(signed, width)
    thr = F32(thr)
    codes = O.ste_codes(y, O.act_scale(thr, signed, width), thr, F32(-thr) if signed else F32(0))
    if regime == "out_saturated":
        nz = np.asarray(y) != 0
        assert (np.abs(codes[nz]) == L).mean() > 0.25, "out_saturated: %.3f of the codes clipped" % (np.abs(codes[nz]) == L).mean()
    elif regime == "out_zero_codes":
        assert np.asarray(y).any() and not codes.any()
    else:
        assert has_allones_significand(divisor(thr, signed, width))
