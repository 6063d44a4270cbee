"""The first ResNeXt unit of a stage (stride 2) under stored thresholds: its grouped 3x3 takes the opening 1x1's codes and writes the
closing 1x1's (fq_gconv3x3_s2_i8_c16, the `g2_next` links) - logits bit-equal to the fp32 hand-over, and no codes online, with the
switch off or past a hook."""
import numpy as np
import pytest

from test_gpu_resnext_unit_s2 import _unit              # (ResNextBlock(64, 16, 4, 2, True) on 128 channels at 9x9)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["offline", "online", "switch_off", "hooked"])
def test_resnext_stride2_unit_hands_codes_through_the_grouped_3x3(gpu, monkeypatch, mode):
    from quantization.mxnet_amd import ops
    from quantization.mxnet_amd.quantize import fuse
    net, X = _unit(gpu, offline=mode != "online")
    assert fuse.fuse_inference(net) > 0
    g3, first = net[0].body[3], net[0].body[0]
    assert g3._fq_pw_fused["stride"] == 2 and g3._fq_pw_fused["g2_next"] is net[0].body[6] and first._fq_pw_fused["g2_next"] is g3
    assert all(b._fq_pw_fused.get("next") is None and b._fq_pw_fused.get("g_next") is None for b in (first, g3))
    seen, plain = [], []
    real, real_i8 = ops.gconv3x3_s2_c16, ops.gconv3x3_i8
    monkeypatch.setattr(ops, "gconv3x3_s2_c16", lambda x, *a, **k: (seen.append((isinstance(x, ops.Codes16), k.get("out_codes") is not None)),
                                                                    real(x, *a, **k))[1])
    monkeypatch.setattr(ops, "gconv3x3_i8", lambda *a, **k: (plain.append(k.get("stride")), real_i8(*a, **k))[1])
    if mode == "switch_off":
        monkeypatch.setattr(fuse, "GCONV_S2_C16", False)
    hook = g3.register_forward_hook(lambda m, a, out: None) if mode == "hooked" else None
    got = net(X)._t.cpu().numpy()
    assert (seen, plain) == (([(True, True)], []) if mode == "offline" else ([], [2])), (seen, plain)
    if hook is not None:
        hook.detach()
    monkeypatch.setattr(fuse, "HANDOVER", False)
    want = net(X)._t.cpu().numpy()
    assert len(seen) == (mode == "offline") and plain[-1] == 2
    assert np.array_equal(got, want), "logits with the stride-2 grouped 3x3 between code tensors differ from the fp32 hand-over"
    fuse.unfuse(net)
