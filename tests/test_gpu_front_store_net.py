"""Net level: MobileNet1.0 with the 28 x 28 depthwise layer dw5 folded into the storing 1x1 behind it (FQ_PW_FRONT_STORE; the
statistic pass of fq_dwconv3x3 + fq_pwconv_i8_front, `ops.pwconv_i8(front=)`) against the same net with the two storing launches.  Batch 2 at 224 x 224,
declared as one of several batches in flight; logits and every quantised block's `current_input_max` byte for byte."""
import contextlib

import numpy as np
import pytest
import torch

from test_gpu_pwdw import N, _eq

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


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(41)
    return [(rng.standard_normal((2, 3, 224, 224)) * (1.0 + 0.5 * i)).astype(np.float32) for i in range(3)]


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
    """Counts, at `ops` level, the storing 1x1 launches with a front layer and the depthwise statistic passes on 256 channels."""

    def __init__(self, ops):
        self.ops, self.dw, self.pw = ops, ops.dwconv3x3, ops.pwconv_i8
        self.stat_passes, self.fronts = [], []

    def __enter__(self):
        def dw(*a, **k):
            if k.get("store", True) is False and a[0].shape[1] == 256:
                self.stat_passes.append(k["x_codes_out"].data_ptr())
            return self.dw(*a, **k)

        def pw(*a, **k):
            if k.get("front") is not None:
                self.fronts.append(k["front"]["x_codes"].data_ptr())
            return self.pw(*a, **k)
        self.ops.dwconv3x3, self.ops.pwconv_i8 = dw, pw
        return self

    def __exit__(self, *exc):
        self.ops.dwconv3x3, self.ops.pwconv_i8 = self.dw, self.pw
        return False


def _forward(net, X, ops, declared=True):
    with _Spy(ops) as spy, (ops.batches_in_flight() if declared else contextlib.nullcontext()):
        out = net(X)
    cur = np.asarray([float(b.current_input_max) for b in net.collect_quantized_blocks()], np.float32)
    return N(out._t), cur, spy


def test_the_fold_changes_no_value_at_any_level_of_the_knob(dev, ops, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    X = mx.nd.array(inputs[0], ctx=mx.gpu(0))
    outs = {}
    for level in (0, 1, 2):
        monkeypatch.setattr(fuse, "PW_FRONT_STORE", level)
        outs[level] = _forward(_net(mx.gpu(0)), X, ops)
    off = outs[0]
    assert off[2].fronts == [] and off[2].stat_passes == []
    assert np.isfinite(off[0]).all() and np.abs(off[0]).max() > 0
    for level in (1, 2):                                     # exactly one link qualifies: dw5 -> pw5
        assert len(outs[level][2].fronts) == 1 and outs[level][2].fronts == outs[level][2].stat_passes, outs[level][2].fronts
        _eq(outs[level][0], off[0], "logits, FQ_PW_FRONT_STORE=%d" % level)
        _eq(outs[level][1], off[1], "current_input_max of every block, FQ_PW_FRONT_STORE=%d" % level)

    # an ordinary forward (one batch at a time) keeps the stored tensor unless the knob is 2; the results are the same
    for level, taken in ((1, 0), (2, 1)):
        monkeypatch.setattr(fuse, "PW_FRONT_STORE", level)
        plain = _forward(_net(mx.gpu(0)), X, ops, declared=False)
        assert len(plain[2].fronts) == taken and len(plain[2].stat_passes) == taken, (level, plain[2].fronts)
        _eq(plain[0], off[0], "logits of an ordinary forward, FQ_PW_FRONT_STORE=%d" % level)
        _eq(plain[1], off[1], "current_input_max of an ordinary forward")
    monkeypatch.setattr(fuse, "PW_FRONT_STORE", 1)

    # a forward hook on dw5: something observes its output, the fold steps aside, same results
    net = _net(mx.gpu(0))
    dw5 = next(b for b in net.collect_quantized_blocks() if getattr(b, "_fq_dw_fused", None) is not None
               and b._fq_dw_fused.get("front_pw") is not None and b._kwargs["num_filter"] == 256)
    seen = []
    dw5.register_forward_hook(lambda blk, i, o: seen.append(tuple(o.shape)))
    hooked = _forward(net, X, ops)
    assert seen == [(2, 256, 28, 28)] and hooked[2].fronts == [] and hooked[2].stat_passes == []
    _eq(hooked[0], off[0], "logits under a forward hook on dw5")
    _eq(hooked[1], off[1], "current_input_max under the hook")


def test_two_lanes_and_a_captured_forward(dev, ops, inputs, monkeypatch):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    monkeypatch.setattr(fuse, "PW_FRONT_STORE", 0)
    net = _net(mx.gpu(0))
    xs = [mx.nd.array(a, ctx=mx.gpu(0)) for a in inputs[:2]]
    ref = [net(x)._t.clone() for x in xs]
    torch.cuda.synchronize()
    monkeypatch.setattr(fuse, "PW_FRONT_STORE", 1)
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
