"""The host guards that keep a shape on the safe side of a 32-bit byte offset, a clamped buffer resource or the lane offset 2^31
("Large tensors"), asked through the C ABI at the last shape inside and the first shape outside each byte limit.

The `fq_*_supported` functions answer without a device (compute units and LDS size fall back to the MI355X's figures), so this
runs on the CPU.  The expected answers are written out from the audit table, not computed: an edit that moves or drops a guard
fails here.  No GPU."""

import pytest

P112 = 112 * 112        # MobileNet's largest planes: a sample of C channels is C * 50 176 bytes
P28 = 28 * 28


@pytest.fixture(scope="module")
def lib():
    from quantization.mxnet_amd import _lib
    return _lib.LIB


def _q(fn, *a):
    return int(fn(*(t(v) for t, v in zip(fn.argtypes, a))))


# fq_pwconv_i8_stat_supported(n, cin, cout, hw, front_h, front_wdt)
STAT = [
    # fq_pw_stat.hip, pw_stat_shape_ok: the resource spans all of x, lane offsets are 32-bit: x below 4 GiB
    # 32 channels: 1 605 632 bytes per sample; 2674 samples = 4 293 459 968 < 2^32 <= 2675 samples = 4 295 065 600
    ((2674, 32, 64, P112, 0, 0), 1), ((2675, 32, 64, P112, 0, 0), 0),
    # ... and the front mode goes through the same guard
    ((2674, 32, 64, P112, 112, 112), 1), ((2675, 32, 64, P112, 112, 112), 0),
    # a half-slab past Cin (Cin % 32 == 16) is masked with the lane offset 2^31: x at most 2 GiB
    # 16 channels: 802 816 bytes per sample; 2674 samples = 2 146 729 984 <= 2^31 < 2675 samples = 2 147 532 800
    ((2674, 16, 64, P112, 0, 0), 1), ((2675, 16, 64, P112, 0, 0), 0), ((5349, 16, 64, P112, 0, 0), 0),
    # (whole slabs have no masked lane: 64 channels up to 4 GiB - 1337 samples = 4 293 459 968)
    ((1337, 64, 128, P112, 0, 0), 1), ((1338, 64, 128, P112, 0, 0), 0),
]


@pytest.mark.parametrize("args,want", STAT, ids=["%dx%d->%d@%d-front%dx%d" % a for a, _ in STAT])
def test_statistic_pass_guards(lib, args, want):
    assert _q(lib.fq_pwconv_i8_stat_supported, *args) == want


# fq_pwdw_fused_supported(n, cin, cout, h, w, stride, stat_mode)
PWDW = [
    # fq_pwdw.hip, pwdw_plan: x below 4 GiB (the statistic pass in front reads it through one resource)
    ((2674, 32, 64, 112, 112, 2, 0), 1), ((2675, 32, 64, 112, 112, 2, 0), 0),
    # ... and fewer than 2^31 output elements: 64 channels of 112 x 112 = 802 816 per sample, 2674 samples = 2 146 729 984
    ((2674, 16, 64, 112, 112, 1, 0), 1), ((2675, 16, 64, 112, 112, 1, 0), 0),
    # 128 channels: 1 605 632 per sample, 1337 samples = 2 146 729 984 < 2^31 <= 1338 samples = 2 148 335 616 (x: 2.1 GB)
    ((1337, 32, 128, 112, 112, 1, 0), 1), ((1338, 32, 128, 112, 112, 1, 0), 0),
    # stride 2 quarters the output: the same batch is taken again
    ((1338, 32, 128, 112, 112, 2, 0), 1),
    # the statistic mode (codes of the depthwise input instead of y): fewer than 2^31 elements of the 1x1 OUTPUT, stride 1
    ((1337, 32, 128, 112, 112, 1, 1), 1), ((1338, 32, 128, 112, 112, 1, 1), 0),
]


@pytest.mark.parametrize("args,want", PWDW, ids=["%dx%d->%d@%dx%d-s%d-mode%d" % a for a, _ in PWDW])
def test_fused_pair_guards(lib, args, want):
    assert _q(lib.fq_pwdw_fused_supported, *args) == want


# fq_pwconv_i8_front_supported(n, cin, cout, h, w): the storing 1x1 with a front layer, 256 -> 256
FRONT = [
    # fq_pw_stat.hip, pw_front_store_shape_ok: the tensor the front layer stands for below 4 GiB
    # 256 channels of 28 x 28: 802 816 bytes per sample; 5349 samples = 4 294 262 784 < 2^32 <= 5350 samples = 4 295 065 600
    ((5349, 256, 256, 28, 28), 1), ((5350, 256, 256, 28, 28), 0),
]


@pytest.mark.parametrize("args,want", FRONT, ids=["%dx%d->%d@%dx%d" % a for a, _ in FRONT])
def test_front_storing_guards(lib, args, want):
    assert _q(lib.fq_pwconv_i8_front_supported, *args) == want


# fq_stem_conv7x7s2_pool_supported(h, w): one sample's three planes within 2 GiB (per-sample resources, lane offset 2^31 as mask)
STEM = [
    # w = 256: 3072 bytes per row of the three planes; 699 050 rows = 2 147 481 600 < 2^31 <= 699 051 rows = 2 147 484 672
    ((699050, 256), 1), ((699051, 256), 0),
]


@pytest.mark.parametrize("args,want", STEM, ids=["%dx%d" % a for a, _ in STEM])
def test_first_convolution_with_pooling_guards(lib, args, want):
    assert _q(lib.fq_stem_conv7x7s2_pool_supported, *args) == want
