"""The depthwise 3x3 dispatcher under its A/B switches: every kernel form forced by FQ_DW_FORM (the four-column form also with
its nontemporal loads, FQ_DW_NT_MB=0), the run-time epilogue forced by FQ_DW_EPI=0 and one column per lane forced by
FQ_DW_PLANES_CPL=1, each against the CPU oracle with the assertions of test_gpu_parity.test_dwconv3x3_vs_oracle.  Every
environment runs the nine cells of a form's template arguments: input unquantised / quantised online / offline, times the
run-time epilogue (bias) / BatchNorm + ReLU / BatchNorm + ReLU6 fixed at compile time.  The library reads these variables once
per process, so every case runs in a fresh child process (this file, run as a script)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ENVS = [{"FQ_DW_FORM": str(k)} for k in (1, 2, 3, 4, 5)] + [{"FQ_DW_EPI": "0"}, {"FQ_DW_PLANES_CPL": "1"}] + [
    {"FQ_DW_FORM": "3", "FQ_DW_NT_MB": "0"}]
SHAPES = [(2, 8, 7, 7), (3, 16, 14, 14), (2, 32, 28, 28), (1, 3, 9, 11), (2, 6, 14, 20),
          (1, 2, 30, 70),       # one column per lane
          (1, 2, 20, 72),       # four columns per lane, two segments per row
          (1, 2, 130, 64),      # LDS tiles in strip mode: WS = 67, 120 / 60 rows per strip against Ho = 130 / 65: two strips
          # one channel: a plane is a sample, and one workgroup step covers more than the 16 samples of its statistic table -
          # the straight-to-memory path.  From the launch geometry (4 wavefronts): 14x14 flat 36 (stride 2: 32) planes, whole
          # planes 36, one column per lane 32 at stride 2; 8x8 four columns per lane 64 (stride 2: 84), one column 24 (48)
          (40, 1, 14, 14), (40, 1, 8, 8)]
MODES = [(quant, epi) for quant in ("none", "online", "offline") for epi in ("bias_relu6", "bn_relu", "bn_relu6")]

_stopped = []       # why no further child is started (a child that died may have left the GPU in a bad state)


@pytest.mark.parametrize("env", ENVS, ids=[",".join("%s=%s" % kv for kv in e.items()) for e in ENVS])
def test_forced_form_vs_oracle(env):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    assert not _stopped, "not started: " + _stopped[0]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        _stopped.append("the child for %r ran into its time limit" % (env,))
        raise
    if r.returncode != 0:
        _stopped.append("the child for %r ended with status %d" % (env, r.returncode))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _child():
    sys.path.insert(0, ROOT)
    import torch
    from oracle import fq_oracle as O
    from quantization.mxnet_amd import ops
    dev = torch.device("cuda", 0)

    def T(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    for shape in SHAPES:
        for stride in (1, 2):
            rng = np.random.default_rng(sum(shape) * 7 + stride)
            c = shape[1]
            x = np.maximum((rng.standard_normal(shape) * 2).astype(np.float32), 0)
            wt = (rng.standard_normal((c, 1, 3, 3)) * 0.5).astype(np.float32)
            sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
            sh = rng.standard_normal(c).astype(np.float32)
            b = rng.standard_normal(c).astype(np.float32)
            stat = O.absmax_per_sample(x)
            thr = np.float32(2.3)
            for quant, epi in MODES:
                what = "%r stride %d %s %s" % (shape, stride, quant, epi)
                kw, okw = {}, {}
                if quant == "online":
                    kw.update(in_stat=T(stat), width=8, flags=0)
                    okw.update(in_max=O.batch_mean(stat), signed=False, width=8)
                elif quant == "offline":
                    kw.update(in_thr=T(np.float32([thr])), width=8, flags=0)
                    okw.update(in_max=thr, signed=False, width=8)
                if epi == "bias_relu6":
                    kw.update(bias=T(b), act="relu6")
                    okw.update(bias=b, act="relu6")
                else:
                    act = epi[3:]
                    kw.update(bn_scale=T(sc), bn_shift=T(sh), act=act)
                    okw.update(bn_scale=sc, bn_shift=sh, act=act)
                cur = torch.zeros(1, device=dev)
                y, stat_out = ops.dwconv3x3(T(x), T(wt), stride=stride, cur_out=cur, **kw)
                want = O.dwconv3x3(x, wt, stride=stride, **okw)
                got = y.cpu().numpy()
                assert got.shape == want.shape, what
                np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6, err_msg=what)
                assert (got != want).mean() < 1e-3, what           # fmaf emulation differs only at double-rounding ties
                assert np.array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(got)), what + ": statistic"
                if quant == "online":
                    assert cur.cpu().numpy()[0] == okw["in_max"], what + ": current_input_max"
                # the layer's statistic pass (y == NULL: the four-column form without its stores, with FQ_DW_NT_MB=0 its
                # nontemporal instantiations): the same maxima, nothing stored
                if quant != "none" and stride == 1 and shape[3] % 4 == 0:
                    codes = torch.zeros(ops.front_codes_shape(shape), dtype=torch.int8, device=dev)
                    none, stat_only = ops.dwconv3x3(T(x), T(wt), stride=1, store=False, x_codes_out=codes, **kw)
                    assert none is None and torch.equal(stat_only, stat_out), what + ": statistic pass"
    print("OK")


if __name__ == "__main__":
    _child()
