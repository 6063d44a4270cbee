"""One ResNeXt bottleneck unit under stored thresholds: the grouped 3x3 takes the opening 1x1's codes and writes the closing 1x1's
(fq_gconv3x3_i8_c16) - logits bit-equal to the fp32 hand-over, and no codes online, with the switch off or past a hook."""
import numpy as np
import pytest

import unit_reference as U

pytestmark = pytest.mark.gpu


def _unit(gpu, offline):
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.mx.gluon import nn
    from quantization.mxnet_amd.mx.gluon.model_zoo import ResNextBlock
    from quantization.mxnet_amd.quantize import convert
    from quantization.mxnet_amd.quantize.initialize import qparams_init
    np.random.seed(7)
    net = nn.HybridSequential(prefix="")
    net.add(ResNextBlock(64, 16, 4, 1, False, in_channels=256, prefix=""))
    net.initialize(mx.init.MSRAPrelu(factor_type="in", slope=0.0))
    convert.convert_model(net, convert_fn={nn.Conv2D: convert.gen_conv2d_converter(quantize_input=True, quant_type="group"),
                                           nn.Activation: None, nn.BatchNorm: None})
    qparams_init(net)
    net.collect_params().reset_ctx(gpu)
    U.randomise_batchnorm(net, 3)
    rng = np.random.default_rng(5)
    X = mx.nd.array(np.maximum(rng.standard_normal((3, 256, 9, 9)), 0).astype(np.float32), ctx=gpu)
    net.quantize_input(enable=True, online=True)
    net(mx.nd.array(np.maximum(rng.standard_normal((3, 256, 9, 9)), 0).astype(np.float32) * 1.3, ctx=gpu))
    net.update_ema()                                    # one naive calibration batch
    net.fix_params()
    net.quantize_input(enable=True, online=not offline)
    return net, X


@pytest.mark.parametrize("mode", ["offline", "online", "switch_off", "hooked"])
def test_resnext_unit_hands_codes_through_the_grouped_3x3(gpu, monkeypatch, mode):
    from quantization.mxnet_amd import ops
    from quantization.mxnet_amd.quantize import fuse
    net, X = _unit(gpu, offline=mode != "online")
    assert fuse.fuse_inference(net) > 0
    g3, first = net[0].body[3], net[0].body[0]
    assert g3._fq_pw_fused["kind"] == "g3x3" and g3._fq_pw_fused["g_next"] is net[0].body[6]
    assert first._fq_pw_fused["g_next"] is g3 and first._fq_pw_fused.get("next") is None and g3._fq_pw_fused.get("next") is None
    seen = []
    real = ops.gconv3x3_i8
    monkeypatch.setattr(ops, "gconv3x3_i8", lambda x, *a, **k: (seen.append((isinstance(x, ops.Codes16), k.get("out_codes") is not None)),
                                                                real(x, *a, **k))[1])
    if mode == "switch_off":
        monkeypatch.setattr(fuse, "GCONV_C16", False)
    hook = g3.register_forward_hook(lambda m, a, out: None) if mode == "hooked" else None
    got = net(X)._t.cpu().numpy()
    assert seen == [(mode == "offline", mode == "offline")], seen
    if hook is not None:
        hook.detach()
    monkeypatch.setattr(fuse, "HANDOVER", False)
    want = net(X)._t.cpu().numpy()
    assert seen[1] == (False, False)
    assert np.array_equal(got, want), "logits with the grouped 3x3 between code tensors differ from the fp32 hand-over"
    fuse.unfuse(net)
