"""Every fused unit on the device against the fp64 composition of the reference (tests/unit_reference.py), with randomised
BatchNorm statistics and at sizes at which the special forms are really chosen.

Run A - the plain fused forms: recompute pairs, subsampled trunk, pooled producer, folded shortcut, int8 hand-over and the pooling
first convolution switched off, so every unit is ONE storing launch whose input and output exist in memory; the per-unit gate
(4 * max(e_fp32, 2^-23), see unit_reference) on every launch, every per-sample statistic and `current_input_max` bit-exact.
Run B - the same net object and input with every switch back on: logits and every block's `current_input_max` bit-equal to run A,
and the forms counted, so that they were really taken.  The special forms are thereby tied to the fp64 reference through the
bit-equality bar the suite already holds them to; no unit needs a tensor that never exists in memory."""
import numpy as np
import pytest
import torch

import unit_reference as U

pytestmark = pytest.mark.gpu

PLAIN = dict(RECOMPUTE=False, SUBSAMPLE=False, GAP_FUSE=False, SHORTCUT_FUSE=False, HANDOVER=False, STEM_POOL=False)
R50 = dict(sub=3, shortcut=4, gap=1)

# (id, model, build arguments, EMA steps before the stored thresholds are used (0: online), batch, what run B must have taken)
CASES = [
    ("mobilenet1.0-layer-online", "mobilenet1.0", dict(), 0, 8, dict(pairs=2, gap=1)),
    ("resnet50_v1-channel-online", "resnet50_v1", dict(quant_type="channel"), 0, 4, R50),
    # (stored thresholds: the closing 1x1 of the last unit reads codes, and the pooling epilogue is built for fp32 inputs)
    ("resnet50_v1-channel-offline", "resnet50_v1", dict(quant_type="channel"), 1, 4, dict(sub=3, shortcut=4, gap=0, codes=1)),
    ("resnet50_v1-wino-F43-online", "resnet50_v1", dict(quant_type="channel", wino="F43"), 0, 4, R50),
    ("mobilenetv2_1.0-w4a8-offline", "mobilenetv2_1.0", dict(quant_type="channel", wt=4), 2, 8, dict(codes=1)),
    ("mobilenet0.75-channel-online", "mobilenet0.75", dict(quant_type="channel"), 0, 4, dict()),
    ("mobilenet0.25-channel-online", "mobilenet0.25", dict(quant_type="channel"), 0, 4, dict()),
    ("mobilenetv2_0.75-channel-online", "mobilenetv2_0.75", dict(quant_type="channel"), 0, 4, dict()),
    ("mobilenetv2_0.5-channel-online", "mobilenetv2_0.5", dict(quant_type="channel"), 0, 4, dict()),
    ("resnet18_v1-channel-online", "resnet18_v1", dict(quant_type="channel"), 0, 4, dict()),
    ("resnet34_v1-channel-online", "resnet34_v1", dict(quant_type="channel"), 0, 4, dict()),
    ("resnet101_v1-channel-online", "resnet101_v1", dict(quant_type="channel"), 0, 4, R50),
    ("resnet50_v1-last_gamma-online", "resnet50_v1", dict(quant_type="channel", last_gamma=True), 0, 4, R50),
    # four bits on both sides (the reference's published c10_r56_uint4_int4 configurations): the gate is measured against the
    # fp32 composition at that width and follows it by itself
    ("mobilenet1.0-w4a4-online", "mobilenet1.0", dict(wt=4, in_w=4), 0, 8, dict(pairs=2, gap=1)),
    ("mobilenetv2_1.0-w4a4-offline", "mobilenetv2_1.0", dict(quant_type="channel", wt=4, in_w=4), 2, 8, dict(codes=1)),
    ("resnet18_v1-channel-w4a4-offline", "resnet18_v1", dict(quant_type="channel", wt=4, in_w=4), 1, 4, dict(codes=1)),
]


def _forms(rec):
    return dict(pairs=rec.count("pwdw_fused"), stat_only=rec.count("pwconv_i8_stat"),
                sub=rec.count("pwconv_i8", subsample=True), shortcut=rec.count("pwconv_i8_shortcut"),
                gap=rec.count("pwconv_i8_gap"), codes=rec.count(codes_out=True) + rec.count("dwconv3x3_c16"))


@pytest.fixture
def deterministic_library():
    """(MobileNetV2's classifier convolution stays with the tensor library, which may pick another algorithm once its database is
    warm: pinned to its deterministic one while two forwards are compared bit for bit, as tests/test_gpu_c16.py does)"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


@pytest.mark.parametrize("name,model,kw,ema_steps,batch,expect", CASES, ids=[c[0] for c in CASES])
def test_every_unit_on_the_device_is_the_reference_composition(gpu, monkeypatch, deterministic_library, name, model, kw, ema_steps, batch, expect):
    """(mobilenetv2_0.75 is the case that found a bug: its 432 -> 72 and 720 -> 120 projections were handed the unit's shortcut as
    a residual operand no form of fq_pwconv_i8 adds for those channel counts, and the fused net's forward raised.)"""
    from quantization.mxnet_amd import mx
    from quantization.mxnet_amd.quantize import fuse
    last_gamma = bool(kw.get("last_gamma"))
    net = U.build(model, 1000, gpu, rand_bn=3, **kw)
    rng = np.random.default_rng(5)
    X = mx.nd.array(rng.standard_normal((batch, 3, 224, 224)).astype(np.float32), ctx=gpu)
    units = U.describe(net)
    net.quantize_input(enable=True, online=True)
    for step in range(ema_steps):                      # naive calibration, as the CLI runs it
        net(mx.nd.array(rng.standard_normal((batch, 3, 224, 224)).astype(np.float32) * (1 + 0.3 * step), ctx=gpu))
        net.update_ema()
    offline = ema_steps > 0
    net.fix_params()
    net.quantize_input(enable=True, online=not offline)
    assert fuse.fuse_inference(net) > 0
    blocks = net.collect_quantized_blocks()
    # run A: every unit one storing launch
    with monkeypatch.context() as m:
        for switch, value in PLAIN.items():
            m.setattr(fuse, switch, value)
        with U.Recorder() as rec_a:
            out_a = net(X)._t.clone()
        cur_a = [float(b.current_input_max) for b in blocks]
    plain = _forms(rec_a)
    assert not any(plain.values()), plain
    bound = U.bind(units, rec_a.launches, out_a)
    assert sum(1 for b in bound if b.unit.quantised) == len(blocks)
    report = []
    try:
        worst = U.check_units(bound, offline, report, last_gamma=last_gamma, library="launch")
    finally:
        print("\n".join(["== %s" % name] + report))
    print("%s: %d units, worst ratio %.2f" % (name, len(bound), worst))
    assert U.check_statistics(rec_a.launches) > 0
    # run B: the forms the net really runs with
    with U.Recorder() as rec_b:
        out_b = net(X)._t.clone()
    cur_b = [float(b.current_input_max) for b in blocks]
    taken = _forms(rec_b)
    print("%s: forms taken %s" % (name, taken))
    assert torch.equal(out_b, out_a), "logits with the special forms differ from the plain fused forms"
    assert cur_b == cur_a, "current_input_max with the special forms differs from the plain fused forms"
    assert taken["pairs"] == taken["stat_only"]
    for form, least in expect.items():
        if form in ("pairs", "codes"):
            assert taken[form] >= least, (form, taken)
        else:
            assert taken[form] == least, (form, taken)
    fuse.unfuse(net)
