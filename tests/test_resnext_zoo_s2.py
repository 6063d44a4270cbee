"""The stride-2 grouped 3x3 layers of the ResNeXt nets: which the fuser hands to fq_gconv3x3_s2_i8, and that entry point's host twin."""
import ctypes

import numpy as np
import pytest

from oracle import fq_oracle as O
from quantization.mxnet_amd.mx.gluon import nn
from quantization.mxnet_amd.mx.gluon.model_zoo import get_model
from test_gpu_gconv3x3 import _dense


def test_stride2_grouped_layers_of_resnext50_qualify():
    from quantization.mxnet_amd.quantize import convert, fuse
    net = get_model("resnext50_32x4d")
    convert.convert_model(net, exclude=[net.features[0], net.features[1]],
                          convert_fn={nn.Conv2D: convert.gen_conv2d_converter(quant_type="group"), nn.Dense: None,
                                      nn.Activation: None, nn.BatchNorm: None})
    grouped = []
    net.apply(lambda b: grouped.append(b) if type(b) is nn.Conv2D and b._kwargs["num_group"] > 1 else None)
    s2 = [b for b in grouped if fuse._is_grouped3x3_s2(b)]
    s1 = [b for b in grouped if fuse._is_grouped3x3(b)]
    assert len(s2) == 3 and all(b._kwargs["stride"] == (2, 2) for b in s2)
    assert len(s1) == 13 and not set(map(id, s1)) & set(map(id, s2))


@pytest.mark.parametrize("c,groups,h,w", [(32, 8, 5, 7), (64, 2, 4, 6)], ids=["cg4_odd", "cg32_even"])
def test_host_twin_against_subsampled_dense_oracle(c, groups, h, w):
    from oracle import host
    lib = ctypes.CDLL(host.build())
    n, cg, thr = 2, c // groups, np.float32(1.7)
    rng = np.random.default_rng(c + h)
    x = (rng.standard_normal((n, c, h, w)) * 2).astype(np.float32)
    wt = rng.standard_normal((c, cg, 3, 3)).astype(np.float32)
    # rows of 320 bytes: tap t's cg codes at 32 t + (the group's position in its slab of 32 channels)
    wc, ws = O.weight_codes(wt, cg, 8)
    rows = np.zeros((c, 10, 32), np.int8)
    for co in range(c):
        p0 = (co % 32) // cg * cg
        rows[co, :9, p0:p0 + cg] = wc[co].reshape(cg, 9).T
    rows, ws = np.ascontiguousarray(rows.reshape(c, 320)), np.ascontiguousarray(ws, np.float32)
    y, stat = np.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), np.float32), np.empty(n, np.float32)
    p, i64 = (lambda a: ctypes.c_void_p(a.ctypes.data)), ctypes.c_int64
    assert lib.fq_gconv3x3_s2_i8_supported_host(i64(c), i64(c), i64(groups)) == 1
    rc = lib.fq_gconv3x3_s2_i8_host(p(x), p(rows), p(ws), None, None, p(y), i64(n), i64(c), i64(groups), i64(h), i64(w), None,
                                    p(np.float32([thr])), ctypes.c_int(8), ctypes.c_uint(3), None, None, None, ctypes.c_int(0),
                                    p(stat), None)
    assert rc == 0
    want = O.conv3x3_i8(x, _dense(wt, groups), cg, 8, in_max=thr, signed=True, width=8)[:, :, ::2, ::2]
    np.testing.assert_array_equal(y, want)
    np.testing.assert_array_equal(stat, O.absmax_per_sample(y))
