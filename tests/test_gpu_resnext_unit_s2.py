"""The first ResNeXt unit of a stage (stride 2, 64 channels in 16 groups at 9x9): fq_gconv3x3_s2_i8 in the fused net against the generic route."""
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
    net.add(ResNextBlock(64, 16, 4, 2, True, in_channels=128, prefix=""))
    net.initialize(mx.init.MSRAPrelu(factor_type="in", slope=0.0))
    convert.convert_model(net, convert_fn={nn.Conv2D: convert.gen_conv2d_converter(quantize_input=True, quant_type="group"),
                                           nn.Activation: None, nn.BatchNorm: None})
    qparams_init(net)
    net.collect_params().reset_ctx(gpu)
    U.randomise_batchnorm(net, 3)
    rng = np.random.default_rng(5)
    X = mx.nd.array(np.maximum(rng.standard_normal((3, 128, 9, 9)), 0).astype(np.float32), ctx=gpu)
    net.quantize_input(enable=True, online=True)
    if offline:                                         # naive calibration, as the CLI runs it
        net(mx.nd.array(np.maximum(rng.standard_normal((3, 128, 9, 9)), 0).astype(np.float32) * 1.3, ctx=gpu))
        net.update_ema()
    net.fix_params()
    net.quantize_input(enable=True, online=not offline)
    return net, X


@pytest.mark.parametrize("offline", [False, True], ids=["online", "offline"])
def test_resnext_stride2_unit_fused_vs_generic_route(gpu, offline):
    from quantization.mxnet_amd.quantize import fuse
    net, X = _unit(gpu, offline)
    ref = net(X)._t.double().cpu().numpy()              # the generic route
    assert fuse.fuse_inference(net) > 0
    fz = net[0].body[3]._fq_pw_fused
    assert fz["kind"] == "g3x3" and fz["stride"] == 2 and fz.get("next") is None
    got = net(X)._t.cpu().numpy()
    print("max |fused - generic| = %.3g of max|ref| = %.3g" % (np.abs(got - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
    fuse.unfuse(net)


def test_resnext_stride2_unit_switch_off(gpu, monkeypatch):
    from quantization.mxnet_amd.quantize import fuse
    monkeypatch.setattr(fuse, "GCONV_S2", False)
    net, _ = _unit(gpu, False)
    assert fuse.fuse_inference(net) > 0
    assert fuse._is_grouped3x3_s2(net[0].body[3]) and not hasattr(net[0].body[3], "_fq_pw_fused")
    fuse.unfuse(net)
