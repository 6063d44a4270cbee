"""Which layers of resnext50_32x4d the fuser links for the int8 hand-over through the grouped 3x3 (fq_gconv3x3_i8_c16)."""
from quantization.mxnet_amd.mx.gluon import nn
from quantization.mxnet_amd.mx.gluon.model_zoo import get_model


def test_stride1_grouped_layers_of_resnext50_are_linked_on_both_sides():
    from quantization.mxnet_amd.quantize import convert, fuse
    net = get_model("resnext50_32x4d")
    convert.convert_model(net, exclude=[net.features[0], net.features[1]],
                          convert_fn={nn.Conv2D: convert.gen_conv2d_converter(quant_type="group"), nn.Dense: None,
                                      nn.Activation: None, nn.BatchNorm: None})
    assert fuse.fuse_inference(net) > 0
    units = []
    net.apply(lambda b: units.append(b) if hasattr(b, "body") and hasattr(b, "downsample") else None)
    linked = 0
    for u in units:
        body = list(u.body._children.values())
        first, g3, last = body[0], body[3], body[6]
        assert g3._fq_pw_fused["kind"] == "g3x3" and last._fq_pw_fused["kind"] == "1x1"
        assert first._fq_pw_fused.get("next") is None and g3._fq_pw_fused.get("next") is None
        if g3._kwargs["stride"] == (1, 1):
            assert first._fq_pw_fused.get("g_next") is g3 and g3._fq_pw_fused.get("g_next") is last
            linked += 1
        else:
            assert first._fq_pw_fused.get("g_next") is None and g3._fq_pw_fused.get("g_next") is None
    assert len(units) == 16 and linked == 13
