"""Which layers of resnext50_32x4d the fuser links for the int8 hand-over through the STRIDE-2 grouped 3x3 (`g2_next`,
fq_gconv3x3_s2_i8_c16), and that entry point's host twin."""
import ctypes

import numpy as np
import pytest

from oracle import fq_oracle as O
from quantization.mxnet_amd.mx.gluon import nn
from quantization.mxnet_amd.mx.gluon.model_zoo import get_model
from test_gpu_gconv3x3 import _dense


def test_stride2_grouped_layers_of_resnext50_are_linked_on_both_sides():
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
        s2 = g3._kwargs["stride"] == (2, 2)
        assert first._fq_pw_fused.get("g2_next") is (g3 if s2 else None) and g3._fq_pw_fused.get("g2_next") is (last if s2 else None)
        assert first._fq_pw_fused.get("g_next") is (None if s2 else g3) and g3._fq_pw_fused.get("g_next") is (None if s2 else last)
        assert last._fq_pw_fused.get("g2_next") is None
        linked += s2
    assert len(units) == 16 and linked == 3


@pytest.mark.parametrize("c,groups,h,w", [(32, 8, 5, 7), (64, 2, 4, 6)], ids=["cg4_odd", "cg32_even"])
@pytest.mark.parametrize("io", ["codes-codes", "codes-fp32", "fp32-codes"])
def test_host_twin_against_subsampled_dense_oracle_and_quantiser(c, groups, h, w, io):
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
    want = np.ascontiguousarray(O.conv3x3_i8(x, _dense(wt, groups), cg, 8, in_max=thr, signed=True, width=8)[:, :, ::2, ::2])
    thr2 = np.float32(0.6) * np.abs(want).max()
    in16, out16 = io.startswith("codes"), io.endswith("codes")
    xin = O.to_c16(O.ste_codes(x, O.act_scale(thr, True, 8), thr, -thr).astype(np.int64), 0) if in16 else x
    y = np.empty(O.to_c16(want.astype(np.int64), 0).shape, np.int8) if out16 else np.empty_like(want)
    stat, thr_a, thr2_a = np.empty(n, np.float32), np.float32([thr]), np.float32([thr2])      # (alive across the call)
    p, i64 = (lambda a: ctypes.c_void_p(a.ctypes.data)), ctypes.c_int64
    rc = lib.fq_gconv3x3_s2_i8_c16_host(p(xin), ctypes.c_int(in16), p(rows), p(ws), None, None, p(y), i64(n), i64(c), i64(groups),
                                        i64(h), i64(w), None, p(thr_a), ctypes.c_int(8), ctypes.c_uint(3), None, None,
                                        None, ctypes.c_int(0), p(stat), p(thr2_a) if out16 else None, ctypes.c_int(8),
                                        ctypes.c_uint(3), None)
    assert rc == 0
    np.testing.assert_array_equal(stat, O.absmax_per_sample(want))
    np.testing.assert_array_equal(y, O.to_c16(O.ste_codes(want, O.act_scale(thr2, True, 8), thr2, -thr2).astype(np.int64), 0)
                                  if out16 else want)
