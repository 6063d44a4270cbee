"""bench.py on one GPU as the driver types it: a plain run times exactly --steps steps in one block and measures nothing
else; --dump-outputs writes what the last timed step computed, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(args, timeout=900):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        out[f[:-4]] = np.load(os.path.join(d, f))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    return out


def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_the_same_logits_twice(gpu, tmp_path):
    recs, dumps = [], []
    for tag in ("a", "b"):
        recs.append(_bench(["--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / tag)]))
        dumps.append(_load(str(tmp_path / tag)))
    for rec in recs:
        assert rec["steps"] == 5 and rec["warmup"] == 2 and rec["repeats"] == 1 and rec["consistency"]["blocks"] == 1
        assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert abs(rec["value"] - 128 * 5 / (rec["ms_per_step"] * 5e-3)) / rec["value"] < 1e-3
        assert rec["roofline"] is None and "cpu_baseline" not in rec and "headline_tensor" not in rec
        assert "single_stream" not in rec and "box" not in rec
        # every forward the process ran: the set-up forward of each of the 3 streams, the 2 warm-up steps, the first replay
        # of every captured graph (3 streams x 4 resident batches) and the 5 timed steps - no other block
        assert rec["config"]["streams"] == 3 and rec["config"]["hipgraph"] is True
        assert rec["eval_counters"]["images"] == 128 * (3 + 2 + 3 * 4 + 5)
    assert set(dumps[0]) == {"logits"}
    logits = dumps[0]["logits"]
    assert logits.dtype == np.float32 and logits.shape == (128, 1000) and np.isfinite(logits).all()
    assert np.array_equal(logits, dumps[1]["logits"])


@pytest.mark.parametrize("phase,names", [("calib-naive", {"logits", "thresholds"}), ("calib-kl", {"histograms", "ranges"})])
def test_calibration_phases_dump_what_their_last_step_produced(gpu, tmp_path, phase, names):
    rec = _bench(["--steps", "3", "--warmup", "1", "--phase", phase, "--model", "cifar_resnet20_v1", "--batch-size", "16",
                  "--dump-outputs", str(tmp_path)])
    assert rec["steps"] == 3 and rec["repeats"] == 1 and rec["roofline"] is None and "kl_search" not in rec
    got = _load(str(tmp_path))
    assert set(got) == names
    for a in got.values():
        assert a.dtype == np.float32 and a.size and np.isfinite(a).all()
    if phase == "calib-kl":
        assert got["histograms"].shape == (got["ranges"].size, 2048) and (got["ranges"] > 0).all()
        assert (got["histograms"].sum(axis=1) > 0).all()
    else:
        assert got["logits"].shape == (16, 10) and (got["thresholds"] >= 0).all()
