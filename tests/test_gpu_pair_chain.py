"""GPU parity of a CHAIN of two recompute pairs: the stride-1 depthwise 3x3 that closes the first pair feeds the 1x1 of the
second, and its output is not stored.
  * fq_pwdw_fused with `mid_codes_out` (`ops.pwdw_fused(store=False, mid_codes_out=)`), the fused launch in statistic mode,
    against the storing fused launch: equal per-sample maxima and `current_input_max`, and the code buffer it keeps - the codes of the 1x1 output it
    has just quantised for the stencil - against the codes the host oracle's quantiser (oracle/fq_host.cpp) makes of the host
    twin's 1x1 output, every byte;
  * fq_pwconv_i8_stat with a front layer of 64 and 128 channels, which recomputes the depthwise values from those codes and is
    handed an x of NaN, against the plain statistic pass fed with the stored fp32 tensor: equal statistic and
    `current_input_max`, byte-equal `x_codes_out`.
Every comparison is bit for bit, every case runs from poisoned, guard-banded memory (tests/poison.py) under both patterns, with
the band lengths of both kernels forced so that they do not coincide and the last band of each is short.  At net level: the
switch FQ_PWDW_CHAIN at 0 / 1 / 2, a hook on the tensor, two lanes, a captured forward."""
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


# (n, cin, cmid, cout, h, w): 1x1 cin -> cmid, depthwise 3x3 on cmid channels (the front layer: 64 and 128 channels, two and four
# slabs), 1x1 cmid -> cout.  Widths: 28 is one strip with the left zero column inside it, 32 two strips with the second anchored
# over the first, 56 MobileNet's, 60 exactly two strips (the only dword two strips share the halves of).  Rows per band: the
# fused launch 2 of 5 (2 + 2 + 1) and 4 of 9 (4 + 4 + 1), the front layer 3 of 5 (3 + 2) and 5 of 9 (5 + 4).
CASES = [(3, cin, cmid, cout, h, w) for (cin, cmid) in ((32, 64), (64, 128)) for cout in (64, 128) for h in (5, 9)
         for w in (28, 32, 56, 60)]
BANDS = {5: (2, 3), 9: (4, 5)}
# without ReLU anywhere in front of the second 1x1: signed codes (two's complement bytes) and the general quantisers
SIGNED_CASES = [(3, 64, 128, 64, 9, 60), (3, 32, 64, 128, 5, 28)]


def _id(c):
    return "%dx%d->%d->%d@%dx%d" % c


def _make(case, signed, regime=None, width=8, mid_width=8):
    """`regime`: a value regime of tests/regimes.py on the input as drawn (every quantiser of the chain works online: the
    regimes with a threshold of their own have none to be stored in).  `width`: the activation width of both 1x1 inputs;
    `mid_width`: that of the depthwise layer's input, the tensor in the middle of the first pair."""
    n, cin, cmid, cout, h, w = case
    rng = np.random.default_rng(1000 * cin + 37 * h + w + cout + (7 if signed else 0))
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32) * np.float32(1.7)
    if not signed:
        x = np.maximum(x, 0)
    x = x * (np.float32(0.55) + np.float32(0.4) * np.arange(n, dtype=np.float32)).reshape(n, 1, 1, 1)
    x[0, 0, 0, 0] = np.float32(5.5)
    k = dict(case=case, signed=signed, x=x.astype(np.float32), width=width, mid_width=mid_width)
    k["w1"] = (rng.standard_normal((cmid, cin)) * 0.2).astype(np.float32)
    k["dww"] = (rng.standard_normal((cmid, 1, 3, 3)) * 0.3).astype(np.float32)
    k["w2"] = (rng.standard_normal((cout, cmid)) * 0.2).astype(np.float32)

    def bn(c):
        s = (0.5 + rng.random(c)).astype(np.float32) * np.where(rng.random(c) < 0.15, -1, 1).astype(np.float32)
        return s, (rng.standard_normal(c) * 0.3).astype(np.float32)
    k["bn1"], k["bn2"], k["bn3"] = bn(cmid), bn(cmid), bn(cout)
    k["act1"] = k["act2"] = None if signed else "relu"
    k["act3"] = "relu"
    if regime is not None:
        assert regime not in ("saturated", "allones_divisor")
        k["x"], k["w1"], _ = R.apply(regime, k["x"], signed, k["w1"], cmid, width=width)
        R.check(regime, k["x"], R.stored_threshold(k["x"]), signed, width=width)
    return k


def _operands(k, dev, ops, put):
    n, cin, cmid, cout, h, w = k["case"]
    o = dict(x=put(k["x"]), dww=ops.weight_fake_quant(_t(k["dww"], dev), cmid, 8))
    o["dww"] = put(N(o["dww"]))
    for name in ("bn1", "bn2", "bn3"):
        o[name] = tuple(put(a) for a in k[name])
    o["w1"] = ops.weight_codes(_t(k["w1"], dev), cmid, 8)
    o["w2"] = ops.weight_codes(_t(k["w2"], dev), cout, 8)
    o["flags"] = ops.act_flags(signed=k["signed"])
    return o


def _first_half(k, o, dev, ops, empty):
    """The statistic pass of the first pair, which hands the codes of x over: common to both ways."""
    cur1 = torch.zeros(1, device=dev)
    xstat = ops.absmax_per_sample(o["x"])
    xcodes = empty(ops.pair_codes_shape(o["x"].shape), torch.int8)
    ystat = ops.pwconv_i8_stat(o["x"], *o["w1"], None, in_stat=xstat, width=k["width"], flags=o["flags"], cur_out=cur1,
                               bn_scale=o["bn1"][0], bn_shift=o["bn1"][1], act=k["act1"], x_codes_out=xcodes)
    return xstat, xcodes, ystat


def _fused(k, o, dev, ops, xstat, xcodes, ystat, cur2, x=None, **more):
    return ops.pwdw_fused(o["x"] if x is None else x, *o["w1"], o["dww"], in_stat=xstat, width=k["width"], flags=o["flags"],
                          pw_bn_scale=o["bn1"][0], pw_bn_shift=o["bn1"][1], pw_act=k["act1"], mid_stat=ystat, mid_width=k["mid_width"],
                          mid_flags=o["flags"], mid_cur_out=cur2, stride=1, dw_bn_scale=o["bn2"][0], dw_bn_shift=o["bn2"][1],
                          dw_act=k["act2"], x_codes=xcodes, **more)


def _stored(k, dev, ops):
    """The reference: the storing fused launch, then the plain statistic pass reading the fp32 tensor it stored."""
    n, cin, cmid, cout, h, w = k["case"]
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    fill = lambda shape, dtype: torch.full(shape, 0x55, dtype=dtype, device=dev)      # noqa: E731
    xstat, xcodes, ystat = _first_half(k, o, dev, ops, fill)
    cur2, cur3 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    z, zstat = _fused(k, o, dev, ops, xstat, xcodes, ystat, cur2)
    buf = fill(ops.pair_codes_shape(z.shape), torch.int8)
    pstat = ops.pwconv_i8_stat(z, *o["w2"], None, in_stat=zstat, width=k["width"], flags=o["flags"], cur_out=cur3, bn_scale=o["bn3"][0],
                               bn_shift=o["bn3"][1], act=k["act3"], x_codes_out=buf)
    return dict(ystat=N(ystat), zstat=N(zstat), cur2=N(cur2), pstat=N(pstat), cur3=N(cur3), buf=N(buf), z=N(z))


def _chained(k, dev, ops, put=None, empty=None):
    """The fused launch in statistic mode and the statistic pass that recomputes the depthwise layer - neither is handed a
    readable fp32 tensor: both get NaN."""
    n, cin, cmid, cout, h, w = k["case"]
    put = put or (lambda a: _t(a, dev))
    empty = empty or (lambda shape, dtype: torch.full(shape, 0x55, dtype=dtype, device=dev))
    o = _operands(k, dev, ops, put)
    xstat, xcodes, ystat = _first_half(k, o, dev, ops, empty)
    cur2, cur3 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ycodes = empty(ops.front_codes_shape((n, cmid, h, w)), torch.int8)
    nan_x = torch.full((n, cin, h, w), float("nan"), device=dev)
    none, zstat = _fused(k, o, dev, ops, xstat, xcodes, ystat, cur2, x=nan_x, store=False, mid_codes_out=ycodes)
    assert none is None
    buf = empty(ops.pair_codes_shape((n, cmid, h, w)), torch.int8)
    nan_z = torch.full((n, cmid, h, w), float("nan"), device=dev)
    front = dict(x_codes=ycodes, w=o["dww"], bias=None, bn_scale=o["bn2"][0], bn_shift=o["bn2"][1], act=k["act2"],
                 in_stat=ystat, width=k["mid_width"], flags=o["flags"])
    pstat = ops.pwconv_i8_stat(nan_z, *o["w2"], None, in_stat=zstat, width=k["width"], flags=o["flags"], cur_out=cur3,
                               bn_scale=o["bn3"][0], bn_shift=o["bn3"][1], act=k["act3"], x_codes_out=buf, front=front)
    return dict(ystat=N(ystat), zstat=N(zstat), cur2=N(cur2), pstat=N(pstat), cur3=N(cur3), buf=N(buf), ycodes=N(ycodes),
                x=N(o["x"]))


def _host_mid_codes(k, ops, dev):
    """The low bytes of the codes the depthwise block's quantiser makes of the 1x1 output, both from the host oracle."""
    from oracle import host as H
    n, cin, cmid, cout, h, w = k["case"]
    y, ystat = H.pwconv_i8(k["x"], k["w1"].reshape(cmid, cin, 1, 1), cmid, 8, in_stat=H.absmax_per_sample(k["x"]),
                           signed=k["signed"], bias=None, bn_scale=k["bn1"][0], bn_shift=k["bn1"][1], act=k["act1"], want_stat=True,
                           width=k["width"])
    codes = H.fake_quant_online_prestat(y, ystat, k["mid_width"], H.act_flags(signed=k["signed"]), want_codes=True)[2]
    return (codes.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8).reshape(n, cmid, h * w), ystat


_REFERENCE = {}


def _reference(case, signed, dev, ops, monkeypatch):
    """(inputs, results of the two stored launches, the host's codes): computed once per case, shared, never changed."""
    key = (case, signed)
    if key not in _REFERENCE:
        k = _make(case, signed)
        _set_bands(monkeypatch, case)
        _REFERENCE[key] = (k, _stored(k, dev, ops), _host_mid_codes(k, ops, dev))
    return _REFERENCE[key]


def _set_bands(monkeypatch, case):
    rb, fr = BANDS[case[4]]
    monkeypatch.setenv("FQ_PWDW_RB", str(rb))
    monkeypatch.setenv("FQ_PWSTAT_FRONT_ROWS", str(fr))


def _compare(got, want, host, regime=None):
    _eq(got["ystat"], want["ystat"], "statistic of the first 1x1 output")
    _eq(got["ystat"], host[1], "statistic of the first 1x1 output vs the host twin")
    _eq(got["zstat"], want["zstat"], "per-sample maxima of the depthwise output: statistic mode vs the storing fused launch")
    _eq(got["cur2"], want["cur2"], "current_input_max of the depthwise block")
    _eq(got["ycodes"], host[0], "codes of the 1x1 output vs the host oracle's quantiser (every byte of the buffer)")
    _eq(got["pstat"], want["pstat"], "statistic of the second 1x1 output: front layer vs the stored tensor")
    _eq(got["cur3"], want["cur3"], "current_input_max of the second 1x1 block")
    _eq(got["buf"], want["buf"], "x_codes_out of the second statistic pass (every byte)")
    assert np.isfinite(want["z"]).all() and (regime is not None or (np.abs(want["z"]).max() > 0 and want["pstat"].max() > 0))


def _poisoned(k, want, host, dev, ops, monkeypatch, pattern):
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        got = _chained(k, dev, ops, put=lambda a: proxy.guarded(a, dev),
                       empty=lambda shape, dtype: proxy.empty(shape, dtype=dtype, device=dev))
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert len(proxy.records) >= 10
        _compare(got, want, host)
        _eq(got["x"], k["x"], "the input after all launches")
    finally:
        proxy.release()
        ops._WS.clear()


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_chained_pair_changes_no_value(dev, ops, monkeypatch, case, pattern):
    n, cin, cmid, cout, h, w = case
    assert ops.pwdw_chain_supported((n, cin, h, w), cmid) and ops.pwconv_front_supported((n, cmid, h, w), cout), case
    k, want, host = _reference(case, False, dev, ops, monkeypatch)
    _set_bands(monkeypatch, case)
    _poisoned(k, want, host, dev, ops, monkeypatch, pattern)
    assert (host[0].view(np.uint8) > 127).any()              # (unsigned codes above 127: the byte is not a clamped int8)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("case", SIGNED_CASES, ids=_id)
def test_signed_codes_and_the_general_quantisers(dev, ops, monkeypatch, case, pattern):
    k, want, host = _reference(case, True, dev, ops, monkeypatch)
    _set_bands(monkeypatch, case)
    _poisoned(k, want, host, dev, ops, monkeypatch, pattern)
    assert (host[0] < 0).any() and (want["z"] < 0).any()


def test_band_lengths_chosen_by_the_launches_themselves(dev, ops, monkeypatch):
    """Without the two knobs: the bands `pwdw_plan` and `front_rows_pick` choose."""
    monkeypatch.delenv("FQ_PWDW_RB", raising=False)
    monkeypatch.delenv("FQ_PWSTAT_FRONT_ROWS", raising=False)
    k = _make((3, 64, 128, 128, 9, 56), False)
    want, host = _stored(k, dev, ops), _host_mid_codes(k, ops, dev)
    _compare(_chained(k, dev, ops), want, host)


# W % 4 != 0 (30 is a plane the storing fused launch takes), a front layer of 48 channels
def test_refused_shapes_fail_with_a_message_and_do_not_launch(dev, ops):
    assert ops.pwdw_supported((3, 32, 9, 30), 64, 1) and not ops.pwdw_chain_supported((3, 32, 9, 30), 64)
    k = _make((3, 32, 64, 64, 9, 30), False)
    o = _operands(k, dev, ops, lambda a: _t(a, dev))
    xstat, xcodes, ystat = _first_half(k, o, dev, ops, lambda s, d: torch.zeros(s, dtype=d, device=dev))
    ycodes = torch.full((3, 64, 9 * 30), 0x55, dtype=torch.int8, device=dev)
    with pytest.raises(ValueError, match="does not take"):
        _fused(k, o, dev, ops, xstat, xcodes, ystat, torch.zeros(1, device=dev), store=False, mid_codes_out=ycodes)
    from quantization.mxnet_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    stat = torch.zeros(3, device=dev)
    rc = _lib.LIB.fq_pwdw_fused(p(o["x"]), p(o["w1"][0]), p(o["w1"][1]), p(o["w1"][2]), None, 3, 32, 64, o["w1"][0].shape[0],
                                64, 9, 30, p(xstat), None, 8, 0, p(o["bn1"][0]), p(o["bn1"][1]), 1, p(ystat), None, 8, 0, None,
                                p(o["dww"]), None, 1, p(o["bn2"][0]), p(o["bn2"][1]), 1, None, p(stat), p(xcodes), None, p(ycodes))
    assert rc != 0 and b"not taken" in _lib.LIB.fq_last_error()
    torch.cuda.synchronize()
    assert (ycodes == 0x55).all()
    for kw in (dict(store=False), dict(mid_codes_out=ycodes)):      # the two go together
        with pytest.raises(ValueError, match="go together"):
            _fused(k, o, dev, ops, xstat, xcodes, ystat, torch.zeros(1, device=dev), **kw)

    assert not ops.pwconv_front_supported((3, 48, 9, 32), 64) and ops.pwconv_front_supported((3, 64, 9, 32), 64)
    wc = ops.weight_codes(torch.zeros(64, 48, device=dev), 64, 8)
    front = dict(x_codes=torch.zeros((3, 48, 9 * 32), dtype=torch.int8, device=dev), w=torch.zeros((48, 1, 3, 3), device=dev),
                 in_stat=torch.ones(3, device=dev), width=8, flags=0)
    with pytest.raises(ValueError, match="does not take"):
        ops.pwconv_i8_stat(torch.zeros((3, 48, 9, 32), device=dev), *wc, None, in_stat=torch.ones(3, device=dev), front=front)


# ---- net level ------------------------------------------------------------------------------------------------------------
def _net(gpu):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    from test_gpu_net import _build as build
    import unit_reference
    net = build("mobilenet1.0", 1000, gpu)
    unit_reference.randomise_batchnorm(net, seed=5)
    net.fix_params()
    net.quantize_input(enable=True, online=True)
    net(mx.nd.array(np.random.default_rng(1).standard_normal((2, 3, 224, 224)).astype(np.float32), ctx=gpu))
    fuse.fuse_inference(net)
    return net


class _Spy(object):
    """Records the fused launches in statistic mode (their code buffers) and the statistic passes with a front layer."""

    def __init__(self, ops):
        self.ops, self.fused, self.pw = ops, ops.pwdw_fused, ops.pwconv_i8_stat
        self.stat_modes, self.stored, self.fronts = [], 0, []

    def __enter__(self):
        def fused(*a, **k):
            if k.get("store", True) is False:
                self.stat_modes.append((k["mid_codes_out"].data_ptr(), tuple(k["mid_codes_out"].shape)))
            else:
                self.stored += 1
            return self.fused(*a, **k)

        def pw(*a, **k):
            if k.get("front") is not None:
                self.fronts.append(k["front"]["x_codes"].data_ptr())
            return self.pw(*a, **k)
        self.ops.pwdw_fused, self.ops.pwconv_i8_stat = fused, pw
        return self

    def __exit__(self, *exc):
        self.ops.pwdw_fused, self.ops.pwconv_i8_stat = self.fused, self.pw
        return False


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(31)
    return [(rng.standard_normal((3, 3, 224, 224)) * (1.0 + 0.5 * i)).astype(np.float32) for i in range(3)]


def _forward(net, X, ops, declared):
    import contextlib
    with _Spy(ops) as spy, (ops.batches_in_flight() if declared else contextlib.nullcontext()):
        out = net(X)
    cur = np.asarray([float(b.current_input_max) for b in net.collect_quantized_blocks()], np.float32)
    net.update_ema()
    thr = np.asarray([b.input_max.data().asscalar() for b in net.collect_quantized_blocks()], np.float32)
    return N(out._t), cur, thr, spy


def test_a_net_with_the_chain_equals_the_same_net_without(dev, ops, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    X = mx.nd.array(inputs[0], ctx=mx.gpu(0))
    monkeypatch.setattr(fuse, "PAIR_CHAIN", 0)
    off = _forward(_net(mx.gpu(0)), X, ops, True)
    assert off[3].stat_modes == [] and off[3].stored == 3
    assert np.isfinite(off[0]).all() and np.abs(off[0]).max() > 0
    # exactly one link qualifies: pair 2 -> pair 3, the 128-channel tensor at 56 x 56; level 1 takes it among batches in flight
    # only, level 2 in every forward
    for level, declared, taken in ((1, True, 1), (1, False, 0), (2, True, 1), (2, False, 1)):
        monkeypatch.setattr(fuse, "PAIR_CHAIN", level)
        on = _forward(_net(mx.gpu(0)), X, ops, declared)
        what = "FQ_PWDW_CHAIN=%d, %s forward" % (level, "declared" if declared else "ordinary")
        assert len(on[3].stat_modes) == taken and on[3].stored == 3 - taken, (what, on[3].stat_modes, on[3].stored)
        if taken:
            assert on[3].stat_modes[0][1] == (3, 128, 56 * 56) and on[3].stat_modes[0][0] in on[3].fronts, what
        _eq(on[0], off[0], "logits, " + what)
        _eq(on[1], off[1], "current_input_max of every block, " + what)
        _eq(on[2], off[2], "thresholds after one naive-EMA step, " + what)


def test_a_hook_on_the_tensor_gets_the_stored_values(dev, ops, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    X = mx.nd.array(inputs[1], ctx=mx.gpu(0))
    seen = {}
    for level in (0, 2):
        monkeypatch.setattr(fuse, "PAIR_CHAIN", level)
        net = _net(mx.gpu(0))
        plain = _forward(net, X, ops, True)
        assert len(plain[3].stat_modes) == (1 if level else 0)
        dw = [b for b in net.collect_quantized_blocks() if getattr(b, "_fq_dw_fused", None) is not None
              and b._kwargs["num_group"] == 128 and b._kwargs["stride"] == (1, 1)]
        assert len(dw) == 1
        got = []
        dw[0].register_forward_hook(lambda blk, i, o: got.append(N(o._t)))
        hooked = _forward(net, X, ops, True)
        assert hooked[3].stat_modes == [] and len(got) == 1 and got[0].shape == (3, 128, 56, 56) and got[0].dtype == np.float32
        _eq(hooked[0], plain[0], "logits under the hook, FQ_PWDW_CHAIN=%d" % level)
        seen[level] = (got[0], plain[0])
    _eq(seen[2][0], seen[0][0], "the tensor the hook was handed")
    _eq(seen[2][1], seen[0][1], "logits")
    assert np.abs(seen[0][0]).max() > 0


def test_two_lanes_and_a_captured_forward(dev, ops, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    monkeypatch.setattr(fuse, "PAIR_CHAIN", 0)
    net = _net(mx.gpu(0))
    xs = [mx.nd.array(a, ctx=mx.gpu(0)) for a in inputs[:2]]
    ref = [net(x)._t.clone() for x in xs]
    torch.cuda.synchronize()
    monkeypatch.setattr(fuse, "PAIR_CHAIN", 1)
    streams = [torch.cuda.Stream(dev) for _ in xs]
    outs, seen = [], []
    for x, s in zip(xs, streams):                                    # issued back to back: nothing waits in between
        with torch.cuda.stream(s), ops.batches_in_flight(), _Spy(ops) as spy:
            outs.append(net(x)._t)
        seen.append(spy.stat_modes)
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert torch.equal(o, r)
    assert len(seen[0]) == 1 and len(seen[1]) == 1 and seen[0][0][0] != seen[1][0][0], seen      # each lane its own code buffer

    static = mx.nd.array(inputs[2], ctx=mx.gpu(0))
    with ops.batches_in_flight():
        net(static)                                                  # eager warm-up on the static input
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _Spy(ops) as spy, ops.batches_in_flight():
        with torch.cuda.graph(g):
            out = net(static)._t
    assert len(spy.stat_modes) == 1 and spy.stat_modes[0][0] in spy.fronts
    for a, w in zip(inputs[:2], ref):
        static._t.copy_(torch.from_numpy(a).to(dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, w)
