"""GPU parity of the code hand-over inside a recompute pair: fq_pwconv_i8_stat(x_codes_out) keeps the int8 codes of x it
multiplies with, fq_pwdw_fused(x_codes) loads them instead of reading and quantising the fp32 x again.  No value may change:
every comparison here is bit for bit - against the same two launches without the buffer, against fq_pwconv_i8 followed by
fq_dwconv3x3, and (the buffer itself) against the codes of the host oracle's quantiser (oracle/fq_host.cpp) in the C16 layout
of include/fakequant.h."""
import numpy as np
import pytest
import torch

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


# (n, cin, cout, h, w, stride): the smallest shapes at which each mechanism of the hand-over can break
CASES = [
    (3, 64, 64, 18, 60, 1),        # h*w = 1080 = 24 mod 32: the statistic pass's tiles straddle samples; 3*1080 = 8 mod 32: a
                                   # partial last tile whose clamped lanes rewrite the last pixel; two strips
    (2, 16, 32, 36, 32, 2),        # half a slab: the second channel block holds only codes of 0
    (3, 32, 64, 40, 36, 1),        # last strip anchored over its neighbour, partial last band, halo rows re-read from the codes
    (2, 128, 128, 30, 32, 2),      # four slabs, stride 2, two bands
    (2, 256, 256, 28, 28, 2),      # eight slabs, one strip narrower than 30 columns
]
MODES = ["online_u8_bn_relu", "online_s8_lo_neg"]      # the fast non-negative path; the general path with signed codes


def _case(case, mode, dev, ops):
    """The pair of tests/test_gpu_pwdw.py with every sample scaled differently: the threshold (batch mean of the per-sample
    maxima) then differs from every single maximum."""
    k = _make(case, mode, dev, ops)
    n = case[0]
    k["x"] = (k["x"] * (np.float32(0.55) + np.float32(0.4) * np.arange(n, dtype=np.float32)).reshape(n, 1, 1, 1)).astype(np.float32)
    return k


def _launch(k, dev, ops, codes_mode, x_for_b=None):
    """Statistic pass + fused launch.  codes_mode: None - without the buffer; "hand" - A writes it, B reads it."""
    n, cin, cout, h, w, stride = k["case"]
    x = _t(k["x"], dev)
    flags = ops.act_flags(signed=k["signed"])
    wc, scales, rowsum = ops.weight_codes(_t(k["w1"], dev).reshape(cout, cin), k["rps"], k["wt_width"])
    w2 = ops.weight_fake_quant(_t(k["w2"], dev), cout, 8)
    bn1 = (_t(k["bn1"][0], dev), _t(k["bn1"][1], dev))
    bn2 = (_t(k["bn2"][0], dev), _t(k["bn2"][1], dev))
    cur1, cur2 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    xstat = ops.absmax_per_sample(x)
    buf = None
    if codes_mode == "hand":
        # (pre-filled: a byte the pass leaves unwritten stays 0x55 and fails the comparison with the oracle's codes)
        buf = torch.full(ops.pair_codes_shape(x.shape), 0x55, dtype=torch.int8, device=dev)
    ystat = ops.pwconv_i8_stat(x, wc, scales, rowsum, None, width=8, flags=flags, cur_out=cur1, bn_scale=bn1[0],
                               bn_shift=bn1[1], act=k["act1"], in_stat=xstat, x_codes_out=buf)
    xb = x if x_for_b is None else x_for_b
    z, zstat = ops.pwdw_fused(xb, wc, scales, rowsum, w2, width=8, flags=flags, pw_bn_scale=bn1[0], pw_bn_shift=bn1[1],
                              pw_act=k["act1"], mid_stat=ystat, mid_width=8, mid_flags=flags, mid_cur_out=cur2, stride=stride,
                              dw_bn_scale=bn2[0], dw_bn_shift=bn2[1], dw_act=k["act2"], in_stat=xstat, x_codes=buf)
    return dict(z=N(z), zstat=N(zstat), ystat=N(ystat), cur1=N(cur1), cur2=N(cur2), buf=None if buf is None else N(buf))


def _host_c16(k):
    """The codes of x under the pair's input quantiser from the host oracle, as the header lays a C16 tensor out over whole
    32-channel slabs: int8 [n][2 ceil(cin / 32)][h * w][16], byte = (code + 128 - zoff) ^ 0x80, channels past cin the code 0."""
    from oracle import host as H
    n, cin, cout, h, w, stride = k["case"]
    flags = H.act_flags(signed=k["signed"])
    codes = H.fake_quant_online_prestat(k["x"], H.absmax_per_sample(k["x"]), 8, flags, want_codes=True)[2]
    cb = 2 * ((cin + 31) // 32)
    full = np.zeros((n, cb * 16, h * w), np.int64)
    full[:, :cin] = codes.reshape(n, cin, h * w)
    zoff = 0 if k["signed"] else 128
    byte = ((full + 128 - zoff) ^ 0x80) & 0xFF
    return byte.astype(np.uint8).view(np.int8).reshape(n, cb, 16, h * w).transpose(0, 1, 3, 2)


@pytest.mark.parametrize("case", CASES, ids=["%dx%d->%d@%dx%ds%d" % c for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_codes_handed_from_the_statistic_pass_change_no_value(dev, ops, case, mode):
    n, cin, cout, h, w, stride = case
    assert ops.pwdw_supported((n, cin, h, w), cout, stride), "shape refused: %s" % (case,)
    k = _case(case, mode, dev, ops)
    plain = _launch(k, dev, ops, None)
    hand = _launch(k, dev, ops, "hand")
    # (a) the statistic pass is the same pass
    _eq(hand["ystat"], plain["ystat"], "statistic with x_codes_out")
    _eq(hand["cur1"], plain["cur1"], "current_input_max of the 1x1 block with x_codes_out")
    # (b) what it wrote: the host quantiser's codes in the header's layout and encoding, every byte of the buffer
    _eq(hand["buf"], _host_c16(k), "code buffer vs the host oracle's quantiser")
    # (c) the fused launch on the codes: same values as on x, and as the two storing launches
    for name in ("z", "zstat", "cur2"):
        _eq(hand[name], plain[name], "%s with x_codes" % name)
    two = _run_pair(k, dev, ops, fused=False)
    for name in ("z", "zstat", "ystat", "cur1", "cur2"):
        _eq(hand[name], two[name], "%s vs pwconv_i8 + dwconv3x3" % name)
    assert np.abs(hand["z"]).max() > 0
    # (d) with the codes the fp32 tensor is not read at all
    nan = torch.full((n, cin, h, w), float("nan"), device=dev)
    blind = _launch(k, dev, ops, "hand", x_for_b=nan)
    _eq(blind["z"], plain["z"], "z from the codes beside an x of NaN")
    _eq(blind["zstat"], plain["zstat"], "zstat from the codes beside an x of NaN")


def test_code_buffer_arguments_are_checked(dev, ops):
    k = _case((2, 16, 32, 36, 32, 2), "online_u8_bn_relu", dev, ops)
    x = _t(k["x"], dev)
    wc, scales, rowsum = ops.weight_codes(_t(k["w1"], dev).reshape(32, 16), k["rps"], k["wt_width"])
    xstat = ops.absmax_per_sample(x)
    assert ops.pair_codes_shape(x.shape) == (2, 2, 36 * 32, 16)
    with pytest.raises(ValueError):
        ops.pwconv_i8_stat(x, wc, scales, rowsum, None, in_stat=xstat, x_codes_out=torch.empty((2, 1, 36 * 32, 16), dtype=torch.int8,
                                                                                              device=dev))
    with pytest.raises(TypeError):
        ops.pwconv_i8_stat(x, wc, scales, rowsum, None, in_stat=xstat, x_codes_out=torch.empty((2, 2, 36 * 32, 16), device=dev))
    with pytest.raises(Exception):
        ops.pwconv_i8_stat(x, wc, scales, rowsum, None, in_stat=xstat, x_codes_out=torch.empty((2, 2, 36 * 32, 16), dtype=torch.int8))


# ---- net level ------------------------------------------------------------------------------------------------------------
def _net(model, gpu):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    from test_gpu_net import _build as build
    net = build(model, 1000, gpu)
    net.fix_params()
    net.quantize_input(enable=True, online=True)
    net(mx.nd.array(np.random.default_rng(1).standard_normal((2, 3, 224, 224)).astype(np.float32), ctx=gpu))
    fuse.fuse_inference(net)
    return net


class _Spy(object):
    """Records, per `ops.pwdw_fused` launch, the code buffer it was handed."""

    def __init__(self, ops):
        self.ops, self.real, self.seen = ops, ops.pwdw_fused, []

    def __enter__(self):
        def spy(*a, **k):
            c = k.get("x_codes")
            self.seen.append(None if c is None else (c.data_ptr(), tuple(c.shape), tuple(a[0].shape)))
            return self.real(*a, **k)
        self.ops.pwdw_fused = spy
        return self

    def __exit__(self, *exc):
        self.ops.pwdw_fused = self.real
        return False


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(23)
    return [(rng.standard_normal((6, 3, 224, 224)) * (1.0 + 0.5 * i)).astype(np.float32) for i in range(3)]


@pytest.mark.parametrize("model", ["mobilenet1.0", "mobilenet0.5"])
def test_a_net_with_the_hand_over_equals_the_same_net_without(dev, ops, model, inputs):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    X = mx.nd.array(inputs[0], ctx=mx.gpu(0))
    outs = {}
    for on in (False, True):
        net = _net(model, mx.gpu(0))
        old = fuse.PAIR_CODES
        fuse.PAIR_CODES = on
        try:
            with _Spy(ops) as spy:
                out = net(X)
            cur = np.asarray([float(b.current_input_max) for b in net.collect_quantized_blocks()], np.float32)
            net.update_ema()
            thr = np.asarray([b.input_max.data().asscalar() for b in net.collect_quantized_blocks()], np.float32)
        finally:
            fuse.PAIR_CODES = old
        outs[on] = (N(out._t), cur, thr, spy.seen)
    assert len(outs[True][3]) >= 2 and len(outs[True][3]) == len(outs[False][3])
    assert all(s is None for s in outs[False][3]), outs[False][3]
    for s in outs[True][3]:                                          # every pair's launch received its input's codes
        assert s is not None and s[1] == ops.pair_codes_shape(s[2]), s
    _eq(outs[True][0], outs[False][0], "logits")
    _eq(outs[True][1], outs[False][1], "current_input_max of every block")
    _eq(outs[True][2], outs[False][2], "thresholds after one naive-EMA step")


@pytest.mark.parametrize("model", ["mobilenet1.0", "mobilenet0.5"])
def test_two_lanes_keep_their_own_code_buffers(dev, ops, model, inputs):
    from quantization.mxnet_amd import mx
    net = _net(model, mx.gpu(0))
    xs = [mx.nd.array(a, ctx=mx.gpu(0)) for a in inputs[:2]]
    ref = [net(x)._t.clone() for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in xs]
    outs, seen = [], []
    for x, s in zip(xs, streams):                                    # issued back to back: nothing waits in between
        with torch.cuda.stream(s), ops.batches_in_flight(), _Spy(ops) as spy:
            outs.append(net(x)._t)
        seen.append(spy.seen)
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert torch.equal(o, r)
    assert len(seen[0]) >= 2 and len(seen[0]) == len(seen[1])
    for a, b in zip(*seen):
        assert a is not None and b is not None and a[0] != b[0], (a, b)


@pytest.mark.parametrize("model", ["mobilenet1.0", "mobilenet0.5"])
def test_a_captured_forward_replays_with_the_hand_over(dev, ops, model, inputs):
    from quantization.mxnet_amd import mx
    net = _net(model, mx.gpu(0))
    want = [net(mx.nd.array(a, ctx=mx.gpu(0)))._t.clone() for a in inputs[1:]]
    static = mx.nd.array(inputs[0], ctx=mx.gpu(0))
    net(static)                                                      # eager warm-up on the static input
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _Spy(ops) as spy:
        with torch.cuda.graph(g):
            out = net(static)._t
    assert len(spy.seen) >= 2 and all(s is not None for s in spy.seen)
    for a, w in zip(inputs[1:], want):
        static._t.copy_(torch.from_numpy(a).to(dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, w)
