"""fq_gconv3x3_s2_i8, the grouped 3x3 convolution with stride 2 on int8 codes.  An output at (oh, ow) is the stride-1 output at (2 oh,
2 ow), exact sums, a per-element epilogue: the subsampled dense oracle is the bit-exact expectation, an fp64 strided convolution the plain one."""
import numpy as np
import pytest
import torch

import poison
from oracle import fq_oracle as O
from test_gpu_gconv3x3 import MODES, T, _make, _up, dev, ops  # noqa: F401  (the stride-1 file's modes, fixtures and helpers)

pytestmark = pytest.mark.gpu

CASES = [  # (n, C, groups, h, w)
    (2, 32, 8, 5, 7),        # odd plane, cg 4, one slab (WC 1, four pixel tiles), last row and column taps out of the image
    (3, 64, 8, 6, 8),        # even plane (8-byte loads), cg 8, blocks that span samples
    (2, 96, 6, 9, 11),       # cg 16, slab count not a multiple of the slabs per workgroup, odd W (4-byte loads) with two slabs
    (1, 128, 4, 14, 14),     # cg 32
    (9, 32, 8, 3, 3),        # many samples per block
    (1, 64, 16, 1, 50),      # a one-row plane wider than a pixel tile
    (4, 32, 8, 1, 1),        # one-pixel outputs of one-pixel planes
    (4, 32, 8, 2, 2),        # ... and of planes whose odd row and column exist
    (1, 64, 8, 3, 70),       # Wo = 35: the even-row panels skip their first region tile
    (2, 32, 8, 28, 28),      # one slab: a band of several blocks of 128 pixels, both panel sets in use
    (2, 64, 8, 28, 28)]      # two slabs: a band of several blocks of 64 pixels


def _run(dev, ops, case, mode, want_pt=None, regime=None, width=8):
    """`regime`, `width`: as in the stride-1 file, whose device-free half makes the data and both references for this stride too."""
    n, c, groups, h, w = case
    k = _make(case, mode, regime, width, stride=2)
    codes, scales, rowsum = ops.weight_codes_g3x3(T(k["wt"], dev), groups, k["rps"], k["wt_width"])
    cur = torch.zeros(1, device=dev)
    y, stat_out = ops.gconv3x3_i8(T(k["x"], dev), codes, scales, rowsum, groups, cur_out=cur, stride=2, width=width,
                                  flags=ops.act_flags(signed=k["signed"]), **_up(k["kw"], dev, T))
    launch, got = ops.last_launch(), y.cpu().numpy()              # (family, WC, PT, NB, CG)
    assert launch[0] == "gconv3x3s2" and launch[4] == k["cg"], launch
    assert launch[1:3] == ((1, 4) if c == 32 else (2, want_pt or 2)), launch      # one slab: WC 1, four pixel tiles
    if h == 28:
        assert launch[3] >= 2 and n * 196 > 32 * launch[2], "this case is here for a band of several blocks: %s" % (launch,)
    np.testing.assert_array_equal(got, k["want"])
    np.testing.assert_array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(got))
    if "in_stat" in k["kw"]:
        np.testing.assert_array_equal(cur.cpu().numpy(), np.float32([k["okw"]["in_max"]]))
    if k["ref"] is not None:        # plain and high-precision: the fp64 strided grouped convolution of the two fake-quantised tensors
        np.testing.assert_allclose(got, k["ref"], rtol=2e-5, atol=2e-5 * np.abs(k["ref"]).max())


@pytest.mark.parametrize("case", CASES, ids=["%dx%dg%d@%dx%d" % c for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_gconv3x3_s2_i8(dev, ops, case, mode):
    _run(dev, ops, case, mode)


@pytest.mark.parametrize("mode", MODES[:2])
def test_gconv3x3_s2_i8_blocks_of_four_tiles(dev, ops, monkeypatch, mode):
    monkeypatch.setenv("FQ_GCS2_PT", "4")
    _run(dev, ops, CASES[10], mode, want_pt=4)             # the larger block, built for the table in DESIGN 3.11


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
def test_gconv3x3_s2_i8_under_poison(dev, ops, monkeypatch, pattern):
    """As the stride-1 file: guard bands intact, every owned output written."""
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setitem(globals(), "T", lambda a, d: proxy.guarded(a, d))
    for case, mode in ((CASES[2], MODES[0]), (CASES[5], MODES[3]), (CASES[10], MODES[2])):
        ops._WS.clear()
        _run(dev, ops, case, mode)
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records
        proxy.release()
    ops._WS.clear()


@pytest.mark.parametrize("c,groups,stride", [(96, 32, 2), (48, 4, 2), (64, 1, 2), (64, 8, 3)], ids=["cg3", "C48", "groups1", "stride3"])
def test_gconv3x3_s2_refuses_other_shapes(dev, ops, c, groups, stride):
    from quantization.mxnet_amd._lib import FakeQuantError
    assert not ops.gconv3x3_supported(c, c, groups, stride=stride)
    x = torch.ones((1, c, 4, 4), device=dev)
    rows_pad = (c + 63) // 64 * 64
    codes = torch.zeros((2 * rows_pad * 320,), dtype=torch.int8, device=dev)[:rows_pad * 320].view(rows_pad, 320)
    with pytest.raises(FakeQuantError, match="fq_gconv3x3_s2_i8"):
        ops.gconv3x3_i8(x, codes, torch.ones(c, device=dev), torch.zeros(c, dtype=torch.int32, device=dev), groups,
                        in_thr=torch.ones(1, device=dev), stride=stride)
