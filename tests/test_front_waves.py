"""Workgroup size and rows per band of the front-layer statistic pass (csrc/fq_front_layout.h: front_waves_pick,
front_rows_pick), on the host: tests/front_waves_main.cpp is compiled with the host compiler, AddressSanitizer and UBSan
against the very header the launch includes, and run as a program of its own.

The rule's own arithmetic (rows the busiest CU dequantises = rounds x workgroups per CU x (R + 2), times 1.2 / 1.1 / 1.0 at
two / three / four wavefronts per SIMD - among the bands of a workgroup of eight and between the two workgroup sizes; the bands of
a workgroup of four are chosen by the plain rule, as before there were workgroups of eight; 1.1 is an interpolation), 256 CUs,
batch 128:
  * 128 channels at 56 x 56, 128 outputs: four wavefronts - 5 rows, two workgroups per CU (two wavefronts per SIMD),
    3 x 2 x 7 x 1.2 = 50.4; eight wavefronts - 5 rows, two workgroups of eight (four per SIMD), 3 x 2 x 7 = 42 (7 rows: one
    workgroup, 4 x 1 x 9 x 1.2 = 43.2): eight on 5 rows;
  * 64 channels at 56 x 56, 64 outputs: four - 4 rows, 2 x 4 x 6 = 48; eight - 7 rows, 2 x 2 x 9 = 36: eight on 7 rows;
  * 32 and 16 channels at 112 x 112: four workgroups of four fit, 7 rows as before, and eight wavefronts are not instantiated.
No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quantization", "mxnet_amd", "csrc")
# (n, cin, cout, h, w, compute units) -> (wavefronts per workgroup, rows per band, wavefronts per SIMD)
PICKS = {(128, 128, 128, 56, 56, 256): (8, 5, 4), (128, 64, 64, 56, 56, 256): (8, 7, 4),
         (128, 32, 64, 112, 112, 256): (4, 7, 4), (128, 16, 32, 112, 112, 256): (4, 7, 4),
         (3, 128, 32, 13, 36, 256): (4, 1, 4), (3, 64, 32, 9, 112, 256): (4, 1, 4)}
# what four wavefronts alone would get: the picks of tests/test_front_layout.py and tests/test_front_layout_wide.py, unchanged
ROWS4 = {(128, 128, 128, 56, 56, 256): 5, (128, 64, 64, 56, 56, 256): 4, (128, 32, 64, 112, 112, 256): 7,
         (128, 16, 32, 112, 112, 256): 7}
# more shapes for the walk of the turns: odd channel counts per turn, short planes, every row width of tests/test_gpu_front_lanes.py
MORE = [(3, cin, 32, h, w, 256) for cin in (16, 32, 64, 128) for h in (9, 13) for w in (12, 16, 28, 36, 56, 60, 64, 112, 256)]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("front_waves") / "front_waves_main")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "front_waves_main.cpp"),
                           "-o", exe])
    args = [str(v) for key in sorted(set(PICKS) | set(MORE)) for v in key]
    res = subprocess.run([exe] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    picks, turns, forced = {}, {}, {}
    for line in res.stdout.splitlines():
        f = line.split()
        key = tuple(int(v) for v in f[1:7])
        if f[0] == "pick":
            picks[key] = dict(waves=int(f[7]), rows=int(f[8]), lds=int(f[9]), wps=int(f[10]), r4=int(f[11]), c4=float(f[12]),
                              r8=int(f[13]), c8=float(f[14]))
        elif f[0] == "forced":
            forced[key + (int(f[7]), int(f[8]))] = dict(waves=int(f[9]), rows=int(f[10]), lds=int(f[11]))
        else:
            turns[key] = (int(f[7]), int(f[8]))
    return picks, turns, forced


def test_workgroup_size_and_rows_by_the_cost_rule(walk):
    picks, _, _ = walk
    assert {k: (picks[k]["waves"], picks[k]["rows"], picks[k]["wps"]) for k in PICKS} == PICKS
    assert {k: picks[k]["r4"] for k in ROWS4} == ROWS4
    p = picks[(128, 128, 128, 56, 56, 256)]
    assert (p["c4"], p["c8"]) == (50.4, 42.0)
    p = picks[(128, 64, 64, 56, 56, 256)]
    assert (p["c4"], p["c8"]) == (48.0, 36.0)


def test_every_launch_fits_the_lds_and_small_inputs_stay_with_four_wavefronts(walk):
    picks, _, _ = walk
    assert all(1 <= p["rows"] <= 8 and 0 < p["lds"] <= 120 * 1024 for p in picks.values()), picks
    assert all(p["waves"] == 4 for k, p in picks.items() if k[1] < 64)


def test_every_channel_and_every_tile_of_a_band_has_one_owner(walk):
    _, turns, _ = walk
    assert set(turns) == set(PICKS) | set(MORE)
    bad = [k for k, v in turns.items() if v != (1, 1)]
    assert not bad, bad[:8]


def test_the_knobs_get_the_workgroup_size_they_ask_for(walk):
    """tests/test_gpu_front_lanes.py forces FQ_PWSTAT_FRONT_WAVES = 8 on these very shapes: the plan the launch calls gives it
    eight wavefronts on every one of 64 and 128 channels - no fall-back to four for want of LDS - and four on 16 and 32; the
    rows are at most those asked for (the plane, the band buffer and the LDS clamp them); the LDS carries eight tables then."""
    _, _, forced = walk
    assert len(forced) == 8 * len(set(PICKS) | set(MORE))
    for (n, cin, cout, h, w, cus, fr, fw), p in forced.items():
        assert p["waves"] == (fw if cin >= 64 else 4), ((n, cin, cout, h, w), fr, fw, p)
        assert 1 <= p["rows"] <= min(fr, h, 8, 32768 // (32 * w)) and 0 < p["lds"] <= 120 * 1024, ((n, cin, cout, h, w), fr, fw, p)
    for (n, cin, cout, h, w, cus, fr, fw), p in forced.items():
        if cin >= 64 and fw == 8:
            four = forced[(n, cin, cout, h, w, cus, fr, 4)]
            assert p["rows"] <= four["rows"]
            assert p["rows"] < four["rows"] or p["lds"] - four["lds"] == 4 * ((cout + 31) // 32) * 128 * 4
