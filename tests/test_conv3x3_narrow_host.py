"""fq_conv3x3_i8_narrow without a GPU: its host twin against the oracle stand-in on the device's weight buffer, the shape rule, and
which blocks of a CIFAR ResNet-20 the fuser hands to it."""
import numpy as np
import pytest
import torch

from oracle import host as H
from oracle import patch as OP
from oracle.patch import oracle_ops
from quantization.mxnet_amd import mx, ops
from quantization.mxnet_amd.mx.gluon import nn
from quantization.mxnet_amd.mx.gluon.model_zoo import get_model
from quantization.mxnet_amd.quantize import convert, fuse
from quantization.mxnet_amd.quantize.initialize import qparams_init


@pytest.mark.parametrize("case,signed", [((2, 16, 16, 5, 7), False), ((5, 16, 40, 3, 3), True), ((3, 32, 32, 9, 11), False)],
                         ids=["2x16->16@5x7", "5x16->40@3x3", "3x32->32@9x11"])
def test_host_twin_equals_the_oracle_stand_in(case, signed):
    n, cin, cout, h, w = case
    rng = np.random.default_rng(sum(case))
    x = (rng.standard_normal((n, cin, h, w)) * 2).astype(np.float32)
    x = x if signed else np.maximum(x, 0)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(0.05, 1.0, (cout, 1, 1, 1))).astype(np.float32)
    codes, scales, rowsum = H.weight_codes(np.ascontiguousarray(wt.transpose(0, 2, 3, 1)), 1, 8)     # rows of 192 / 320
    assert codes.shape[1] == (9 * cin + 63) // 64 * 64
    stat = np.abs(x).reshape(n, -1).max(axis=1)
    sc, sh = rng.uniform(0.3, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    flags = H.act_flags(signed=signed)
    y, cur, stat_out = np.empty((n, cout, h, w), np.float32), np.zeros(1, np.float32), np.zeros(n, np.float32)
    H._call("fq_conv3x3_i8_narrow_host", x, codes, scales, rowsum, None, y, n, cin, cout, h, w, stat, None, H._i(8), H._u(flags),
            cur, sc, sh, H._i(1), stat_out, None)
    ocur = torch.zeros(1)
    want, want_stat = OP.conv3x3_i8(torch.from_numpy(x), torch.from_numpy(codes), torch.from_numpy(scales), torch.from_numpy(rowsum),
                                    in_stat=torch.from_numpy(stat), width=8, flags=flags, cur_out=ocur,
                                    bn_scale=torch.from_numpy(sc), bn_shift=torch.from_numpy(sh), act="relu")
    np.testing.assert_array_equal(y, want.numpy())
    np.testing.assert_array_equal(stat_out, want_stat.numpy())
    np.testing.assert_array_equal(cur, ocur.numpy())


@pytest.mark.parametrize("cin,cout,ok", [(16, 16, True), (32, 64, True), (16, 1, True), (8, 16, False), (48, 48, False),
                                         (64, 64, False)])
def test_shape_rule(cin, cout, ok):
    assert ops.conv3x3_narrow_supported(cin, cout) == ok


@pytest.mark.parametrize("on", [True, False], ids=["FQ_C3_NARROW=1", "FQ_C3_NARROW=0"])
def test_fuser_hands_the_stride_1_layers_of_the_first_two_stages_over(monkeypatch, on):
    monkeypatch.setattr(fuse, "C3_NARROW", on)
    net = get_model("cifar_resnet20_v1", classes=10)
    fn = {nn.Conv2D: convert.gen_conv2d_converter(quantize_input=True), nn.Dense: convert.gen_dense_converter(quantize_input=True),
          nn.Activation: None, nn.BatchNorm: None}
    convert.convert_model(net, exclude=[net.features[0], net.features[1], net.features[2][0].body[0], net.features[2][0].body[1]],
                          convert_fn=fn)
    net.initialize(mx.init.Xavier())
    qparams_init(net)
    with oracle_ops():
        net(mx.nd.array(np.zeros((1, 3, 16, 16), np.float32)))
        fuse.fuse_inference(net)
    convs = [b for b in net.collect_quantized_blocks() if type(b) is nn.Conv2D and b._kwargs["kernel"] == (3, 3)]
    narrow = [b for b in convs if b.weight.shape[1] in (16, 32)]
    want = [b for b in narrow if b._kwargs["stride"] == (1, 1)]
    assert len(want) == 10 and len(narrow) == 12          # (the excluded first convolution of the first unit is not counted)
    for b in narrow:
        fz = getattr(b, "_fq_pw_fused", None)
        assert (fz is not None and fz["kind"] == "3x3") == (on and b in want), b.name
        assert fz is None or (fz.get("narrow") and fz.get("next") is None)
    for b in convs:                                        # no hand-over link into a narrow block either; the wide ones stay
        fz = getattr(b, "_fq_pw_fused", None)
        assert fz is None or fz.get("next") is None or not fz["next"]._fq_pw_fused.get("narrow")
        assert b.weight.shape[1] != 64 or b._kwargs["stride"] != (1, 1) or fz["kind"] == "3x3"
