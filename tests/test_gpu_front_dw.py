"""GPU parity of the depthwise layer in FRONT of a recompute pair: fq_dwconv3x3 without y (the statistic pass that keeps its
input's codes) followed by fq_pwconv_i8_stat with a front layer (which recomputes the depthwise values from those codes) against
the two launches they replace - fq_dwconv3x3 storing z, fq_pwconv_i8_stat(x_codes_out) reading it.  No value may change: every
comparison is bit for bit (both statistics, both `current_input_max`, every byte of the code buffer), also from poisoned,
guard-banded memory (tests/poison.py), and at net level against the switch FQ_PWDW_FRONT=0."""
import numpy as np
import pytest
import torch

import poison
import regimes as R
from test_gpu_pwdw import N, _eq, _t

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


# (n, cin, cout, h, w).  Rows of 112 floats are MobileNet's; a band of the front layer is 2 rows on the 3-row plane (bands of 2
# and 1 rows, the second a short tile of 112 pixels = 3.5 tiles), 4 rows on the 5-row plane and 8 on the 17-row one (8 + 8 + 1);
# 64- and 32-wide rows put 4 and 8 channels into a wavefront.  Tiles of the reference pass straddle samples (336 = 16 mod 32).
TAKEN = [
    (3, 16, 32, 3, 112),
    (3, 32, 64, 5, 112),
    (3, 32, 96, 3, 112),
    (3, 16, 96, 17, 112),
    (3, 32, 32, 12, 64),
    (3, 16, 64, 9, 32),
]
# rows that are no multiple of four floats: the form refuses, the caller keeps the two storing launches
REFUSED = [(3, 32, 64, 7, 61), (3, 16, 32, 9, 33), (3, 32, 96, 4, 30)]
# quantisers: the unsigned fast path on both layers; signed codes with FQ_ACT_LO_NEG_MAX on the depthwise input / on the 1x1
# input / on both; a stored 1x1 threshold whose divisor make_fast_quot declines (significand all ones)
MODES = ["u8_bn_relu", "u8_bn_relu6", "u8_bias_none", "s8_front", "s8_pw", "s8_both", "u8_no_fast_quot"]


def _declined_threshold():
    """A threshold t with fp32(t / 255) + 1e-10 == a divisor whose significand is all ones (fq_common.h: make_fast_quot
    declines it and the kernel divides through the fp64 reciprocal)."""
    d = np.float32(np.uint32(0x3C7FFFFF).view(np.float32))
    t0 = np.float32(d * np.float32(255))
    for k in range(-64, 65):
        t = np.float32(np.uint32(t0.view(np.uint32) + np.uint32(k)).view(np.float32)) if k >= 0 else \
            np.float32(np.uint32(t0.view(np.uint32) - np.uint32(-k)).view(np.float32))
        den = np.float32(np.float32(t / np.float32(255)) + np.float32(1e-10))
        if (den.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF:
            return float(t)
    raise AssertionError("no threshold found whose divisor has an all-ones significand")


def _make(case, mode, seed=0, regime=None, front_width=8, width=8):
    """`regime`: a value regime of tests/regimes.py on the depthwise layer's input as drawn (both quantisers in front of the
    stored 1x1 threshold work online: `saturated` has no threshold to be stored in); `allones_divisor` is stored as the 1x1's
    threshold.  `front_width`, `width`: the activation widths of the depthwise layer's and of the 1x1's input."""
    n, cin, cout, h, w = case
    rng = np.random.default_rng(seed + 31 * cin + 7 * h + w)
    k = dict(case=case, mode=mode, s_front="s8_front" in mode or "s8_both" in mode, s_pw="s8_pw" in mode or "s8_both" in mode,
             front_width=front_width, width=width)
    y0 = rng.standard_normal((n, cin, h, w)).astype(np.float32) * np.float32(1.9)
    if not k["s_front"]:
        y0 = np.maximum(y0, 0)
    y0 = y0 * (np.float32(0.6) + np.float32(0.45) * np.arange(n, dtype=np.float32)).reshape(n, 1, 1, 1)
    y0[n - 1] = 0                                           # one all-zero sample
    y0[0, 0, 0, 0] = np.float32(6.25)
    k["y0"] = y0.astype(np.float32)
    k["dww"] = (rng.standard_normal((cin, 1, 3, 3)) * 0.4).astype(np.float32)
    k["w1"] = (rng.standard_normal((cout, cin)) * 0.2).astype(np.float32)

    def bn(c):
        s = (0.5 + rng.random(c)).astype(np.float32) * np.where(rng.random(c) < 0.25, -1, 1).astype(np.float32)
        s[1] = 0                                            # a zero scale, negative ones
        s[2] = -np.abs(s[2])
        return s, (rng.standard_normal(c) * 0.3).astype(np.float32)
    k["bnA"], k["bnB"] = bn(cin), bn(cout)
    k["biasA"] = None
    k["actA"] = "relu6" if "relu6" in mode else "relu"
    k["actB"] = "relu"
    if "bias_none" in mode:                                 # depthwise bias, no BatchNorm, no activation: the run-time epilogue
        k["bnA"], k["biasA"], k["actA"] = (None, None), (rng.standard_normal(cin) * 0.2).astype(np.float32), None
    if k["s_pw"]:
        k["actA"] = None                                    # signed values reach the 1x1: its clip range is [-max, max]
    k["thrB"] = _declined_threshold() if "no_fast_quot" in mode else None
    if regime is not None:
        assert regime != "saturated"
        k["y0"], _, rthr = R.apply(regime, k["y0"], k["s_front"], width=front_width)
        if regime == "allones_divisor":
            k["thrB"] = float(R.allones_threshold(k["s_pw"], width))
            assert R.has_allones_significand(R.divisor(k["thrB"], k["s_pw"], width))
        else:
            R.check(regime, k["y0"], R.stored_threshold(k["y0"]), k["s_front"], width=front_width)
    return k


def _operands(k, dev, ops, put):
    n, cin, cout, h, w = k["case"]
    o = dict(y0=put(k["y0"]), dww=put(k["dww"]), biasA=None if k["biasA"] is None else put(k["biasA"]),
             bnA=tuple(None if a is None else put(a) for a in k["bnA"]), bnB=tuple(put(a) for a in k["bnB"]))
    o["wc"], o["scales"], o["rowsum"] = ops.weight_codes(_t(k["w1"], dev), cout, 8)
    o["fA"], o["fB"] = ops.act_flags(signed=k["s_front"]), ops.act_flags(signed=k["s_pw"])
    o["thrB"] = None if k["thrB"] is None else put(np.float32([k["thrB"]]))
    return o


def _two_launches(k, dev, ops):
    """The reference: the storing depthwise launch, then the statistic pass reading what it stored."""
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    s0 = ops.absmax_per_sample(o["y0"])
    z, zstat = ops.dwconv3x3(o["y0"], o["dww"], o["biasA"], stride=1, in_stat=s0, width=k["front_width"], flags=o["fA"], cur_out=curA,
                             bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"])
    buf = torch.full(ops.pair_codes_shape(z.shape), 0x55, dtype=torch.int8, device=dev)
    pstat = ops.pwconv_i8_stat(z, o["wc"], o["scales"], o["rowsum"], None, in_stat=zstat, in_thr=o["thrB"], width=k["width"],
                               flags=o["fB"], cur_out=curB, bn_scale=o["bnB"][0], bn_shift=o["bnB"][1], act=k["actB"],
                               x_codes_out=buf)
    return dict(zstat=N(zstat), curA=N(curA), pstat=N(pstat), curB=N(curB), buf=N(buf), z=N(z))


def _front(k, dev, ops, put=None, empty=None):
    """The statistic pass of the depthwise layer, then the 1x1 statistic pass that recomputes it - handed an x of NaN."""
    put = put or (lambda a: _t(a, dev))
    empty = empty or (lambda shape, dtype: torch.full(shape, 0x55, dtype=dtype, device=dev))
    o = _operands(k, dev, ops, put)
    n, cin, cout, h, w = k["case"]
    curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    s0 = ops.absmax_per_sample(o["y0"])
    ycodes = empty(ops.front_codes_shape(o["y0"].shape), torch.int8)
    none, zstat = ops.dwconv3x3(o["y0"], o["dww"], o["biasA"], stride=1, in_stat=s0, width=k["front_width"], flags=o["fA"], cur_out=curA,
                                bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"], store=False, x_codes_out=ycodes)
    assert none is None
    buf = empty(ops.pair_codes_shape((n, cin, h, w)), torch.int8)
    nan = torch.full((n, cin, h, w), float("nan"), device=dev)
    front = dict(x_codes=ycodes, w=o["dww"], bias=o["biasA"], bn_scale=o["bnA"][0], bn_shift=o["bnA"][1], act=k["actA"],
                 in_stat=s0, width=k["front_width"], flags=o["fA"])
    pstat = ops.pwconv_i8_stat(nan, o["wc"], o["scales"], o["rowsum"], None, in_stat=zstat, in_thr=o["thrB"], width=k["width"],
                               flags=o["fB"], cur_out=curB, bn_scale=o["bnB"][0], bn_shift=o["bnB"][1], act=k["actB"],
                               x_codes_out=buf, front=front)
    return dict(zstat=N(zstat), curA=N(curA), pstat=N(pstat), curB=N(curB), buf=N(buf), ycodes=N(ycodes), y0=N(o["y0"]))


_REFERENCE = {}


def _reference(case, mode, dev, ops):
    """(inputs, results of the two existing launches): computed once per case and mode, shared, never changed."""
    key = (case, mode)
    if key not in _REFERENCE:
        k = _make(case, mode)
        _REFERENCE[key] = (k, _two_launches(k, dev, ops))
    return _REFERENCE[key]


def _compare(got, want, k, regime=None):
    _eq(got["zstat"], want["zstat"], "per-sample statistic of the depthwise output")
    _eq(got["curA"], want["curA"], "current_input_max of the depthwise block")
    _eq(got["pstat"], want["pstat"], "statistic of the 1x1 output")
    _eq(got["curB"], want["curB"], "current_input_max of the 1x1 block")
    _eq(got["buf"], want["buf"], "code buffer of the depthwise output (every byte, the half-slab past Cin included)")
    # (`boundaries` fills every sample: there the all-zero one is gone)
    assert (regime == "boundaries" or not k["y0"][-1].any()) and (regime is not None or (np.abs(want["z"]).max() > 0 and want["pstat"].max() > 0))


def _input_codes(k):
    """The codes fq_dwconv3x3's quantise-on-load makes of y0, from the host oracle, as their low bytes."""
    from oracle import host as H
    flags = H.act_flags(signed=k["s_front"])
    codes = H.fake_quant_online_prestat(k["y0"], H.absmax_per_sample(k["y0"]), k["front_width"], flags, want_codes=True)[2]
    n, cin, h, w = k["y0"].shape
    return (codes.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(n, cin, h * w)


@pytest.mark.parametrize("case", TAKEN, ids=["%dx%d->%d@%dx%d" % c for c in TAKEN])
@pytest.mark.parametrize("mode", MODES)
def test_the_recomputed_depthwise_layer_changes_no_value(dev, ops, case, mode):
    n, cin, cout, h, w = case
    assert ops.pwconv_front_supported((n, cin, h, w), cout), "shape refused: %s" % (case,)
    k, want = _reference(case, mode, dev, ops)
    got = _front(k, dev, ops)
    _compare(got, want, k)
    _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input vs the host oracle's quantiser")
    if "no_fast_quot" in mode:
        den = np.float32(np.float32(np.float32(k["thrB"]) / np.float32(255)) + np.float32(1e-10))
        assert (den.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("case,mode", [(TAKEN[0], "u8_bn_relu"), (TAKEN[1], "s8_both"), (TAKEN[2], "u8_bias_none"),
                                       (TAKEN[3], "u8_bn_relu6"), (TAKEN[4], "s8_front"), (TAKEN[5], "u8_no_fast_quot")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d->%d@%dx%d" % v)
def test_both_passes_from_poisoned_guarded_memory(dev, ops, monkeypatch, case, mode, pattern):
    """Inputs between guard bands, every output and statistic target poisoned: the statistic pass of the depthwise layer writes
    its statistic, its `current_input_max` and the code buffer and nothing else; no result carries poison."""
    k, want = _reference(case, mode, dev, ops)
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        got = _front(k, dev, ops, put=lambda a: proxy.guarded(a, dev),
                     empty=lambda shape, dtype: proxy.empty(shape, dtype=dtype, device=dev))
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert len(proxy.records) >= 8
        _compare(got, want, k)
        _eq(got["y0"], k["y0"], "the depthwise input after both passes")
        _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input")
    finally:
        proxy.release()
        ops._WS.clear()


@pytest.mark.parametrize("case", REFUSED, ids=["%dx%d->%d@%dx%d" % c for c in REFUSED])
def test_refused_planes_are_reported_and_the_two_launches_remain(dev, ops, case):
    n, cin, cout, h, w = case
    assert not ops.pwconv_front_supported((n, cin, h, w), cout)
    k = _make(case, "u8_bn_relu")
    with pytest.raises(Exception):
        _front(k, dev, ops)
    want = _two_launches(k, dev, ops)                       # the fall-back: what the caller runs instead
    assert want["pstat"].max() > 0 and np.isfinite(want["z"]).all()


def test_arguments_are_checked(dev, ops):
    k = _make(TAKEN[0], "u8_bn_relu")
    n, cin, cout, h, w = k["case"]
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    s0 = ops.absmax_per_sample(o["y0"])
    assert ops.front_codes_shape(o["y0"].shape) == (n, cin, h * w)
    good = torch.empty((n, cin, h * w), dtype=torch.int8, device=dev)
    with pytest.raises(ValueError):                         # the codes belong to the statistic pass
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, x_codes_out=good)
    with pytest.raises(ValueError):
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, store=False, x_codes_out=torch.empty((n, cin, h, w), dtype=torch.int8, device=dev))
    with pytest.raises(TypeError):
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, store=False, x_codes_out=torch.empty((n, cin, h * w), device=dev))
    with pytest.raises(Exception):
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, store=False, x_codes_out=torch.empty((n, cin, h * w), dtype=torch.int8))
    with pytest.raises(ValueError):                         # 16-byte alignment
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, store=False,
                      x_codes_out=torch.empty(n * cin * h * w + 16, dtype=torch.int8, device=dev)[4:4 + n * cin * h * w].view(n, cin, h * w))
    with pytest.raises(Exception):                          # a statistic pass of a form that has none: stride 2
        ops.dwconv3x3(o["y0"], o["dww"], stride=2, in_stat=s0, store=False)
    with pytest.raises(ValueError):
        ops.dwconv3x3(o["y0"], o["dww"], in_stat=s0, store=False, want_stat=False)


# ---- net level ------------------------------------------------------------------------------------------------------------
def _net(model, gpu):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    from test_gpu_net import _build as build
    import unit_reference
    net = build(model, 1000, gpu)
    unit_reference.randomise_batchnorm(net, seed=5)
    net.fix_params()
    net.quantize_input(enable=True, online=True)
    net(mx.nd.array(np.random.default_rng(1).standard_normal((2, 3, 128, 128)).astype(np.float32), ctx=gpu))
    fuse.fuse_inference(net)
    return net


class _Spy(object):
    """Counts the launches of the two passes at `ops` level: depthwise statistic passes, 1x1 passes with a front layer."""

    def __init__(self, ops):
        self.ops, self.dw, self.pw = ops, ops.dwconv3x3, ops.pwconv_i8_stat
        self.stat_passes, self.fronts, self.plain = [], [], 0

    def __enter__(self):
        def dw(*a, **k):
            if k.get("store", True) is False:
                self.stat_passes.append(k["x_codes_out"].data_ptr())
            return self.dw(*a, **k)

        def pw(*a, **k):
            if k.get("front") is not None:
                self.fronts.append(k["front"]["x_codes"].data_ptr())
            else:
                self.plain += 1
            return self.pw(*a, **k)
        self.ops.dwconv3x3, self.ops.pwconv_i8_stat = dw, pw
        return self

    def __exit__(self, *exc):
        self.ops.dwconv3x3, self.ops.pwconv_i8_stat = self.dw, self.pw
        return False


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(29)
    return [(rng.standard_normal((3, 3, 128, 128)) * (1.0 + 0.5 * i)).astype(np.float32) for i in range(3)]


def _forward(net, X, ops, declared=True):
    """One forward on the default stream - `declared`: as one of several batches in flight (`ops.batches_in_flight()`), which is
    where the front layer is taken by default; on the default stream such a forward still writes every `current_input_max`."""
    import contextlib
    with _Spy(ops) as spy, (ops.batches_in_flight() if declared else contextlib.nullcontext()):
        out = net(X)
    cur = np.asarray([float(b.current_input_max) for b in net.collect_quantized_blocks()], np.float32)
    net.update_ema()
    thr = np.asarray([b.input_max.data().asscalar() for b in net.collect_quantized_blocks()], np.float32)
    return N(out._t), cur, thr, spy


@pytest.mark.parametrize("model", ["mobilenet1.0", "mobilenet0.5"])
def test_a_net_with_the_front_layer_equals_the_same_net_without(dev, ops, model, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    X = mx.nd.array(inputs[0], ctx=mx.gpu(0))
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(fuse, "PAIR_FRONT", on)
        outs[on] = _forward(_net(model, mx.gpu(0)), X, ops)
    off, on = outs[False], outs[True]
    assert off[3].stat_passes == [] and off[3].fronts == [] and off[3].plain >= 1
    assert len(on[3].stat_passes) == 1 and on[3].fronts == on[3].stat_passes, (on[3].stat_passes, on[3].fronts)
    assert on[3].plain == off[3].plain - 1
    _eq(on[0], off[0], "logits")
    _eq(on[1], off[1], "current_input_max of every block")
    _eq(on[2], off[2], "thresholds after one naive-EMA step")
    assert np.isfinite(on[0]).all() and np.abs(on[0]).max() > 0

    # an ordinary forward (one batch at a time: calibration, a single evaluation) keeps the stored tensor unless FQ_PWDW_FRONT=2
    # asks for the front layer everywhere; the results are the same
    for level, taken in ((1, 0), (2, 1)):
        monkeypatch.setattr(fuse, "PAIR_FRONT", level)
        plain = _forward(_net(model, mx.gpu(0)), X, ops, declared=False)
        assert len(plain[3].stat_passes) == taken and len(plain[3].fronts) == taken, (level, plain[3].stat_passes)
        _eq(plain[0], off[0], "logits of an ordinary forward, FQ_PWDW_FRONT=%d" % level)
        _eq(plain[1], off[1], "current_input_max of an ordinary forward")
        _eq(plain[2], off[2], "thresholds after one naive-EMA step, ordinary forward")
    monkeypatch.setattr(fuse, "PAIR_FRONT", 1)

    # a forward hook on the depthwise block: something observes its output, the two storing launches run, same results
    net = _net(model, mx.gpu(0))
    dw = next(b for b in net.collect_quantized_blocks() if getattr(b, "_fq_dw_fused", None) is not None
              and b._fq_dw_fused.get("front_pw") is not None)
    seen = []
    dw.register_forward_hook(lambda blk, i, o: seen.append(tuple(o.shape)))
    hooked = _forward(net, X, ops)
    assert seen and hooked[3].stat_passes == [] and hooked[3].fronts == []
    _eq(hooked[0], off[0], "logits under a forward hook on the depthwise block")
    _eq(hooked[1], off[1], "current_input_max under the hook")


@pytest.mark.parametrize("model", ["mobilenet1.0", "mobilenet0.5"])
def test_two_lanes_and_a_captured_forward(dev, ops, model, inputs):
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
        seen.append(spy.fronts)
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert torch.equal(o, r)
    assert len(seen[0]) == 1 and len(seen[1]) == 1 and seen[0][0] != seen[1][0], seen      # each lane its own code buffer

    static = mx.nd.array(inputs[2], ctx=mx.gpu(0))
    net(static)                                                      # eager warm-up on the static input
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _Spy(ops) as spy, ops.batches_in_flight():
        with torch.cuda.graph(g):
            out = net(static)._t
    assert len(spy.fronts) == 1 and spy.fronts == spy.stat_passes
    for a, w in zip(inputs[:2], ref):
        static._t.copy_(torch.from_numpy(a).to(dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, w)
