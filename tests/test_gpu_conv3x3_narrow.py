"""fq_conv3x3_i8_narrow: the dense 3x3 convolution on int8 codes for 16 and 32 input channels, reached through ops.conv3x3_i8.
Bit for bit against the oracle stand-in on the same weight codes (exact integer sums, the same fp32 chain), once against an fp64
convolution of the dequantised operands, once under guard-banded buffers, and in a fused CIFAR ResNet-20 with the route on and off."""
import numpy as np
import pytest
import torch

import poison
import regimes as R
from oracle import fq_oracle as O
from oracle import patch as OP
from test_gpu_gconv3x3 import T, _input_side, dev, ops  # noqa: F401  (fixtures, the upload helper, the regime's threshold)

pytestmark = pytest.mark.gpu

CASES = [  # (n, cin, cout, h, w)
    (2, 16, 16, 5, 7),       # two taps per K slab, odd plane
    (3, 32, 32, 9, 11),      # one tap per K slab
    (5, 16, 40, 3, 3),       # partial channel tile, blocks that span samples
    (4, 32, 8, 1, 1),        # one-pixel planes: every tap but the centre is padding
    (2, 16, 16, 32, 32),     # the real planes: several blocks per band, the second panel in use
    (2, 32, 64, 16, 16),
    (1, 16, 16, 2, 37)]      # a plane wider than a pixel tile
MODES = ["online_u8_bn_relu", "offline_s8_channel_w4_bias", "both_u8_bn", "online_s8_plain"]


def _make(case, mode, regime=None, width=8):
    """What needs no device: the data as drawn, turned into `regime` (tests/regimes.py) and checked against its condition, the
    launch keywords as host arrays, the oracle's output on the fp32 filter and the dequantised input at `width`."""
    n, cin, cout, h, w = case
    signed, rng = "s8" in mode, np.random.default_rng(sum(case) + 13)
    x = (rng.standard_normal((n, cin, h, w)) * 2).astype(np.float32)
    x = x if signed else np.maximum(x, 0)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    rps, wt_width = 1 if "channel" in mode else cout, 4 if "w4" in mode else 8
    stored = not mode.startswith("online")
    x, wt, rthr = R.apply(regime, x, signed, wt, rps, np.float32(2.3) if stored else None, width=width)
    kw, in_max = _input_side(regime, rthr, x, stored, both=mode.startswith("both"))
    R.check(regime, x, in_max, signed, w=wt, rps=rps, wt_width=wt_width, taps=9, width=width)
    if "bn" in mode:
        kw.update(bn_scale=rng.uniform(0.3, 1.5, cout).astype(np.float32), bn_shift=rng.standard_normal(cout).astype(np.float32),
                  act="relu" if "relu" in mode else None)
    if "bias" in mode:
        kw["bias"] = rng.standard_normal(cout).astype(np.float32)
    want = O.conv3x3_i8(x, wt, rps, wt_width, in_max, signed=signed, width=width,
                        **{k: v for k, v in kw.items() if k in ("bias", "bn_scale", "bn_shift", "act")})
    assert np.isfinite(want).all()
    xq = O.ste_forward(x, O.act_scale(in_max, signed, width), in_max, -in_max if signed else 0.0)
    return dict(x=x, wt=wt, rps=rps, wt_width=wt_width, signed=signed, kw=kw, want=want, xq=xq)


def _run(dev, ops, case, mode, monkeypatch, fp64=False, regime=None, width=8):
    """`regime`: a value regime of tests/regimes.py, applied to the data as drawn (tests/test_gpu_value_regimes.py).
    `width`: the activation width of the launch and of the references (tests/test_gpu_act_widths.py)."""
    n, cin, cout, h, w = case
    if h * w >= 256:                                              # (at this batch the launch rule would take one block per band)
        monkeypatch.setenv("FQ_C3N_NB", "2")
    mk = _make(case, mode, regime, width)
    codes, scales, rowsum = ops.weight_codes_3x3(T(mk["wt"], dev), mk["rps"], mk["wt_width"])
    kw = dict(mk["kw"], width=width, flags=ops.act_flags(signed=mk["signed"]))
    up = lambda d, f: {k: (f(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}      # noqa: E731
    cur, ocur = torch.zeros(1, device=dev), torch.zeros(1)
    y, stat_out = ops.conv3x3_i8(T(mk["x"], dev), codes, scales, rowsum, cur_out=cur, **up(kw, lambda a: T(a, dev)))
    launch = ops.last_launch()                                    # (family, CIN, WC, PTW, NB)
    assert launch[:3] == ("conv3x3narrow", cin, 2 if cout > 32 else 1), launch
    if h * w >= 256:
        assert launch[4] >= 2 and n * h * w > 128 * launch[4], "this case is here for a band of several blocks: %s" % (launch,)
    want, want_stat = OP.conv3x3_i8(torch.from_numpy(mk["x"]), codes.cpu(), scales.cpu(), rowsum.cpu(), cur_out=ocur,
                                    **up(kw, torch.from_numpy))
    got = y.cpu().numpy()
    np.testing.assert_array_equal(got, want.numpy())
    np.testing.assert_array_equal(got, mk["want"])                 # ... and the oracle on the fp32 filter, weight codes of its own
    np.testing.assert_array_equal(stat_out.cpu().numpy(), want_stat.numpy())
    np.testing.assert_array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(got))
    if "in_stat" in kw:
        np.testing.assert_array_equal(cur.cpu().numpy(), np.float32([O.batch_mean(kw["in_stat"])]))
        np.testing.assert_array_equal(cur.cpu().numpy(), ocur.numpy())
    if fp64:                 # plain and high-precision: the fp64 convolution of the two dequantised tensors
        wq = (codes.cpu().numpy()[:cout, :9 * cin].astype(np.float32) * scales.cpu().numpy()[:, None]).reshape(cout, 3, 3, cin)
        ref = torch.nn.functional.conv2d(torch.from_numpy(mk["xq"].astype(np.float64)),
                                         torch.from_numpy(wq.transpose(0, 3, 1, 2).astype(np.float64)), padding=1).numpy()
        if "bias" in kw:
            ref = ref + kw["bias"].astype(np.float64).reshape(1, -1, 1, 1)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())


@pytest.mark.parametrize("case", CASES, ids=["%dx%d->%d@%dx%d" % c for c in CASES])
@pytest.mark.parametrize("mode", MODES)
def test_conv3x3_narrow_vs_oracle(dev, ops, monkeypatch, case, mode):
    _run(dev, ops, case, mode, monkeypatch)


@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=["cin16", "cin32"])
def test_conv3x3_narrow_vs_fp64(dev, ops, monkeypatch, case):
    _run(dev, ops, case, MODES[3], monkeypatch, fp64=True)


def test_conv3x3_narrow_under_poison(dev, ops, monkeypatch):
    """Guard bands intact around every buffer, every owned output written: a partial channel tile, and a band of several blocks."""
    proxy = poison.Proxy(poison.PATTERNS[0])
    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setitem(globals(), "T", lambda a, d: proxy.guarded(a, d))
    for case, mode in ((CASES[2], MODES[1]), (CASES[5], MODES[0])):
        ops._WS.clear()
        _run(dev, ops, case, mode, monkeypatch)
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records
        proxy.release()
    ops._WS.clear()


def test_fused_cifar_resnet_with_the_route_on_and_off(gpu, monkeypatch):
    """A fused cifar_resnet20_v1 gives the same logits whether its 16- and 32-channel 3x3 layers run on fq_conv3x3_i8_narrow or on
    the generic route, to the bound test_gpu_net.py holds a fused net to against the unfused one."""
    from quantization.mxnet_amd import mx, ops
    from quantization.mxnet_amd.quantize import fuse
    from test_gpu_net import _build
    X = mx.nd.array(np.random.default_rng(7).standard_normal((8, 3, 32, 32)).astype(np.float32), ctx=gpu)
    seen, real = [], ops.conv3x3_i8
    monkeypatch.setattr(ops, "conv3x3_i8", lambda x, *a, **k: (seen.append(x.shape[1]), real(x, *a, **k))[1])
    outs = {}
    for on in (True, False):
        monkeypatch.setattr(fuse, "C3_NARROW", on)
        net = _build("cifar_resnet20_v1", 10, gpu)
        net.fix_params()
        net.quantize_input(enable=True, online=True)
        assert fuse.fuse_inference(net) > 0
        del seen[:]
        outs[on] = net(X).asnumpy()
        assert ({16, 32} <= set(seen)) == on and 64 in seen, seen
    assert np.abs(outs[True] - outs[False]).max() <= 5e-2 * np.abs(outs[False]).max()
