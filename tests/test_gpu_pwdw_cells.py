"""One launch per cell of the recompute pair's kernels.  The host picks an instantiation of pwdw_kernel<KT, CW, S, LZ, FAST, CODES,
NS> (csrc/fq_pwdw.hip) from run-time values; the MobileNet-shaped cases of tests/test_gpu_pwdw.py and tests/test_gpu_pair_chain.py
do not reach the statistic mode with four and eight slabs or with one channel tile per wavefront, nor stride 1 with one channel
tile per wavefront.  Here every one of the 128 cells is launched on a handful of rows:
  KT 1 2 4 8 = cin 32 64 128 256; CW 1 2 = cout 32 64; (S, LZ) = stride 1 on 5 x 28 (one strip, left zero column inside it) and
  on 5 x 32 (two strips, the second anchored), stride 2 on 6 x 32; FAST = the compile-time epilogue (`online_u8_bn_relu`) or the
  run-time one with the fast (`online_u8_bias_nobn`) and the general quantiser (`online_s8_lo_neg`); CODES = fp32 or code input;
  NS = the storing launch, and at stride 1 on code input the statistic mode.  FQ_PWDW_RB=2 makes bands of 2 + 2 + 1 / 2 + 1 rows.
Storing cells: output, per-sample maxima and both `current_input_max` against fq_pwconv_i8 then fq_dwconv3x3.  Statistic-mode
cells: per-sample maxima and `current_input_max` against the storing launch of the same case, every byte of `mid_codes_out`
against the host oracle's codes of the host twin's 1x1 output.  All bit for bit, NaN = NaN.
The front mode of pw_stat_kernel<KT, FEPI, FSIGNED, NW> (csrc/fq_pw_stat.hip): the cells that tests/test_gpu_front_dw.py,
test_gpu_front_lanes.py, test_gpu_front_layout.py and test_gpu_pair_chain.py do not reach (profiles/pair_units_one_of_each.txt
lists who reaches which) on a plane of the same size."""
import numpy as np
import pytest
import torch

from test_gpu_front_lanes import _sweep
from test_gpu_pwdw import N, _eq, _make, _run_pair, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


GEOMS = [(5, 28, 1), (5, 32, 1), (6, 32, 2)]                     # (h, w, stride)
CASES = [(2, cin, cout, h, w, s) for cin in (32, 64, 128, 256) for cout in (32, 64) for (h, w, s) in GEOMS]
MODES = ["online_u8_bn_relu", "online_u8_bias_nobn", "online_s8_lo_neg"]


def _host_mid_codes(k):
    """The low bytes of the codes the depthwise block's quantiser makes of the 1x1 output, both from the host oracle
    (tests/test_gpu_pair_chain.py's, for a pair of tests/test_gpu_pwdw.py: bias or BatchNorm)."""
    from oracle import host as H
    n, cin, cout, h, w, stride = k["case"]
    bn1 = (None, None) if k["bn1"] is None else k["bn1"]
    y, ystat = H.pwconv_i8(k["x"], k["w1"], k["rps"], k["wt_width"], in_stat=H.absmax_per_sample(k["x"]), signed=k["signed"],
                           bias=k["b1"], bn_scale=bn1[0], bn_shift=bn1[1], act=k["act1"], want_stat=True)
    codes = H.fake_quant_online_prestat(y, ystat, 8, H.act_flags(signed=k["signed"]), want_codes=True)[2]
    return (codes.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(n, cout, h * w)


def _statistic_mode(k, dev, ops):
    """fq_pwconv_i8_stat handing the codes of x over, then the fused launch in statistic mode (x itself is NaN)."""
    n, cin, cout, h, w, stride = k["case"]
    x = _t(k["x"], dev)
    flags = ops.act_flags(signed=k["signed"])
    wc = ops.weight_codes(_t(k["w1"], dev).reshape(cout, cin), k["rps"], k["wt_width"])
    w2 = ops.weight_fake_quant(_t(k["w2"], dev), cout, 8)
    bn1 = (None, None) if k["bn1"] is None else (_t(k["bn1"][0], dev), _t(k["bn1"][1], dev))
    bn2 = (None, None) if k["bn2"] is None else (_t(k["bn2"][0], dev), _t(k["bn2"][1], dev))
    b1, b2 = _t(k["b1"], dev), _t(k["b2"], dev)
    cur1, cur2 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    xstat = ops.absmax_per_sample(x)
    xcodes = torch.full(ops.pair_codes_shape(x.shape), 0x55, dtype=torch.int8, device=dev)
    ystat = ops.pwconv_i8_stat(x, *wc, b1, in_stat=xstat, width=8, flags=flags, cur_out=cur1, bn_scale=bn1[0], bn_shift=bn1[1],
                               act=k["act1"], x_codes_out=xcodes)
    ycodes = torch.full(ops.front_codes_shape((n, cout, h, w)), 0x55, dtype=torch.int8, device=dev)
    none, zstat = ops.pwdw_fused(torch.full_like(x, float("nan")), *wc, w2, pw_bias=b1, in_stat=xstat, width=8, flags=flags,
                                 pw_bn_scale=bn1[0], pw_bn_shift=bn1[1], pw_act=k["act1"], mid_stat=ystat, mid_width=8,
                                 mid_flags=flags, mid_cur_out=cur2, dw_bias=b2, stride=1, dw_bn_scale=bn2[0], dw_bn_shift=bn2[1],
                                 dw_act=k["act2"], x_codes=xcodes, store=False, mid_codes_out=ycodes)
    assert none is None
    return dict(zstat=N(zstat), cur2=N(cur2), ycodes=N(ycodes))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d->%d@%dx%ds%d" % c for c in CASES])
def test_every_cell_of_the_fused_launch(dev, ops, monkeypatch, case, mode):
    from quantization.mxnet_amd import _lib
    n, cin, cout, h, w, stride = case
    monkeypatch.setenv("FQ_PWDW_RB", "2")                        # (the library reads it at every call)
    assert _lib.LIB.fq_pwdw_fused_supported(n, cin, cout, h, w, stride, 0) == 1, "a cell's shape is refused: %s" % (case,)
    assert ops.pwdw_supported((n, cin, h, w), cout, stride), case
    k = _make(case, mode, dev, ops)
    two = _run_pair(k, dev, ops, fused=False)
    assert np.abs(two["z"]).max() > 0
    stored = {}
    for codes in (False, True):
        what = "code input" if codes else "fp32 input"
        buf = torch.full(ops.pair_codes_shape((n, cin, h, w)), 0x55, dtype=torch.int8, device=dev) if codes else None
        one = stored[codes] = _run_pair(k, dev, ops, fused=True, codes_buf=buf)
        _eq(one["ystat"], two["ystat"], "statistic-only pass vs the storing pointwise kernel, " + what)
        _eq(one["cur1"], two["cur1"], "current_input_max of the 1x1 block, " + what)
        _eq(one["cur2"], two["cur2"], "current_input_max of the depthwise block, " + what)
        _eq(one["z"], two["z"], "fused output vs the two launches, " + what)
        _eq(one["zstat"], two["zstat"], "fused per-sample statistic vs the two launches, " + what)
    if stride == 1:
        assert _lib.LIB.fq_pwdw_fused_supported(n, cin, cout, h, w, 1, 1) == 1, "statistic mode refused: %s" % (case,)
        assert ops.pwdw_chain_supported((n, cin, h, w), cout), case
        got = _statistic_mode(k, dev, ops)
        _eq(got["zstat"], stored[True]["zstat"], "per-sample maxima: statistic mode vs the storing launch")
        _eq(got["cur2"], stored[True]["cur2"], "current_input_max of the depthwise block: statistic mode vs the storing launch")
        _eq(got["ycodes"], _host_mid_codes(k), "codes of the 1x1 output vs the host oracle's quantiser (every byte)")


# pw_stat_kernel's front mode, (slabs, epilogue, signed input codes, wavefronts): 64 and 128 channels (two and four slabs, four
# and eight wavefronts each) with ReLU6, with the run-time epilogue on unsigned and on signed codes, with signed codes behind ReLU
# and ReLU6; 16 channels with signed codes behind ReLU6.  (`_make` of tests/test_gpu_front_dw.py reads the mode by its parts.)
FRONT_CELLS = [(cin, mode) for cin in (64, 128)
               for mode in ("u8_bn_relu6", "u8_bias_none", "s8_front", "s8_front_bn_relu6", "s8_both")] + [(16, "s8_front_bn_relu6")]


@pytest.mark.parametrize("cin,mode", FRONT_CELLS)
def test_the_front_cells_no_other_test_reaches(dev, ops, monkeypatch, cin, mode):
    _sweep((3, cin, 32, 9, 36), mode, (5,), 0xFF, dev, ops, monkeypatch)
