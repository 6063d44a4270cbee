"""The host twin of the storing 1x1 with a front layer (include/fakequant_host.h: fq_pwconv_i8_front_host) IS the composition it is
documented as: fq_dwconv3x3_host (stride 1) on the depthwise layer's input, then fq_pwconv_i8_host on what it wrote, the depthwise
output's per-sample maxima as the 1x1's online statistic.  Called once through the library and compared, byte for byte, with the two
twins called one after the other; and the shape question answers as the device entry point's does.  No GPU."""
import ctypes

import numpy as np
import pytest

from oracle import host as H

F32 = np.float32


@pytest.mark.parametrize("signed", [False, True])
def test_the_twin_is_the_two_storing_twins_back_to_back(signed):
    rng = np.random.default_rng(11)
    n, c, h, w, cout = 3, 256, 5, 12, 256
    x = (rng.standard_normal((n, c, h, w)) * 1.7).astype(F32)
    if not signed:
        x = np.maximum(x, 0)
    x[-1] = 0                                               # an all-zero sample
    dww = (rng.standard_normal((c, 1, 3, 3)) * 0.4).astype(F32)
    w1 = (rng.standard_normal((cout, c)) * 0.2).astype(F32)
    bnA = ((0.5 + rng.random(c)).astype(F32), (rng.standard_normal(c) * 0.3).astype(F32))
    bnB = ((0.5 + rng.random(cout)).astype(F32), (rng.standard_normal(cout) * 0.3).astype(F32))
    actA = None if signed else "relu"
    s0 = H.absmax_per_sample(x)
    # the two twins, one after the other
    z, zstat = H.dwconv3x3(x, dww, in_stat=s0, signed=signed, bn_scale=bnA[0], bn_shift=bnA[1], act=actA, want_stat=True)
    y, ystat = H.pwconv_i8(z, w1, 1, 8, in_stat=zstat, signed=signed, bn_scale=bnB[0], bn_shift=bnB[1], act="relu", want_stat=True)
    # the one call
    codes, scales, rowsum = H.weight_codes(w1, 1, 8)
    z1, y1 = np.full_like(z, np.nan), np.full_like(y, np.nan)
    zstat1, ystat1 = np.zeros(n, F32), np.zeros(n, F32)
    cur, fcur = np.empty(1, F32), np.empty(1, F32)
    flags = H._u(H.act_flags(signed))
    H._call("fq_pwconv_i8_front_host", x, z1, zstat1, codes, scales, rowsum, None, y1, n, c, codes.shape[1], cout, h, w, None, None,
            H._i(8), flags, cur, bnB[0], bnB[1], H._i(H._ACTS["relu"]), ystat1, dww, None, bnA[0], bnA[1], H._i(H._ACTS[actA]),
            s0, None, H._i(8), flags, fcur, None)
    for a, b, what in ((z1, z, "depthwise output"), (zstat1, zstat, "its statistic"), (y1, y, "1x1 output"), (ystat1, ystat, "its statistic")):
        assert a.tobytes() == b.tobytes(), what
    assert np.abs(y).max() > 0 and fcur[0] == H.batch_mean(s0) and cur[0] == H.batch_mean(zstat)


def test_the_shape_question():
    lib = H.lib()
    q = lambda *a: int(lib.fq_pwconv_i8_front_supported_host(*(ctypes.c_int64(v) for v in a)))      # noqa: E731
    assert q(2, 256, 256, 28, 28) == 1 and q(1, 256, 256, 1, 12) == 1
    assert q(2, 256, 256, 7, 30) == 0 and q(2, 512, 256, 28, 28) == 0 and q(2, 256, 512, 28, 28) == 0 and q(2, 128, 128, 28, 28) == 0
