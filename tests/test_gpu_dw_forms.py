"""The depthwise 3x3 dispatcher under its A/B switches: every kernel form forced by FQ_DW_FORM, the run-time epilogue forced
by FQ_DW_EPI=0 and one column per lane forced by FQ_DW_PLANES_CPL=1, each against the CPU oracle with the assertions of
test_gpu_parity.test_dwconv3x3_vs_oracle.  The library reads these variables once per process, so every case runs in a fresh
child process (this file, run as a script)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ENVS = [{"FQ_DW_FORM": str(k)} for k in (1, 2, 3, 4, 5)] + [{"FQ_DW_EPI": "0"}, {"FQ_DW_PLANES_CPL": "1"}]
SHAPES = [(2, 8, 7, 7), (3, 16, 14, 14), (2, 32, 28, 28), (1, 3, 9, 11), (2, 6, 14, 20),
          (1, 2, 30, 70),       # one column per lane
          (1, 2, 20, 72),       # four columns per lane, two segments per row
          (1, 2, 130, 64)]      # LDS tiles in strip mode: WS = 67, 120 / 60 rows per strip against Ho = 130 / 65: two strips
MODES = ["bn_relu_online", "bias_relu6"]

_stopped = []       # why no further child is started (a child that died may have left the GPU in a bad state)


@pytest.mark.parametrize("env", ENVS, ids=["%s=%s" % kv for e in ENVS for kv in e.items()])
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
            for mode in MODES:
                what = "%r stride %d %s" % (shape, stride, mode)
                rng = np.random.default_rng(sum(shape) * 7 + stride)
                c = shape[1]
                x = np.maximum((rng.standard_normal(shape) * 2).astype(np.float32), 0)
                wt = (rng.standard_normal((c, 1, 3, 3)) * 0.5).astype(np.float32)
                kw, okw = {}, {}
                if mode == "bn_relu_online":
                    stat = O.absmax_per_sample(x)
                    sc = rng.uniform(0.3, 1.5, c).astype(np.float32)
                    sh = rng.standard_normal(c).astype(np.float32)
                    kw.update(in_stat=T(stat), width=8, flags=0, bn_scale=T(sc), bn_shift=T(sh), act="relu")
                    okw.update(in_max=O.batch_mean(stat), signed=False, width=8, bn_scale=sc, bn_shift=sh, act="relu")
                else:
                    b = rng.standard_normal(c).astype(np.float32)
                    kw.update(bias=T(b), act="relu6")
                    okw.update(bias=b, act="relu6")
                cur = torch.zeros(1, device=dev)
                y, stat_out = ops.dwconv3x3(T(x), T(wt), stride=stride, cur_out=cur, **kw)
                want = O.dwconv3x3(x, wt, stride=stride, **okw)
                got = y.cpu().numpy()
                assert got.shape == want.shape, what
                np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6, err_msg=what)
                assert (got != want).mean() < 1e-3, what           # fmaf emulation differs only at double-rounding ties
                assert np.array_equal(stat_out.cpu().numpy(), O.absmax_per_sample(got)), what + ": statistic"
                if "online" in mode:
                    assert cur.cpu().numpy()[0] == okw["in_max"], what + ": current_input_max"
    print("OK")


if __name__ == "__main__":
    _child()
