"""The ResNeXt nets of the model zoo: parameter counts that follow from gluoncv's structure, and which of their grouped 3x3
layers the fuser would hand to fq_gconv3x3_i8."""
import numpy as np
import pytest

from quantization.mxnet_amd.mx.gluon import nn
from quantization.mxnet_amd.mx.gluon.model_zoo import get_model, get_model_list

COUNTS = {"resnext50_32x4d": 25028904, "resnext101_32x4d": 44177704, "resnext101_64x4d": 83455272}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_resnext_trainable_values(name):
    assert name in get_model_list()
    net = get_model(name)
    assert sum(int(np.prod(p.shape)) for p in net.collect_params().values() if p.grad_req != "null") == COUNTS[name]


def test_stride1_grouped_layers_of_resnext50_qualify():
    from quantization.mxnet_amd.quantize import convert, fuse
    net = get_model("resnext50_32x4d")
    convert.convert_model(net, exclude=[net.features[0], net.features[1]],
                          convert_fn={nn.Conv2D: convert.gen_conv2d_converter(quant_type="group"), nn.Dense: None,
                                      nn.Activation: None, nn.BatchNorm: None})
    grouped = []
    net.apply(lambda b: grouped.append(b) if type(b) is nn.Conv2D and b._kwargs["num_group"] > 1 else None)
    assert len(grouped) == 16
    taken = [b for b in grouped if fuse._is_grouped3x3(b)]
    assert len(taken) == 13 and all(b._kwargs["stride"] == (1, 1) for b in taken)
    assert all(b._kwargs["stride"] == (2, 2) for b in grouped if b not in taken)
