"""The band buffer of the front-layer statistic pass (csrc/fq_front_layout.h), walked on the host: tests/front_layout_main.cpp is
compiled with the host compiler against the very header the kernel includes and plays both phases lane by lane.  For every row
width the shape check admits (Q = W / 4 = 4 .. 64 lanes per row), every R = 1 .. 8 rows per band, 16 and 32 channels, full and
short bands:
  * the pixel -> slot map is a bijection onto the band, every byte inside the buffer pw_stat_launch allocates;
  * under the LDS bank rule ((address / 4) mod 32, lanes 0-31 and 32-63 apart) no byte store of phase 1 puts more than two
    distinct dwords on a bank, and no fragment read of phase 2 more than one;
and the rows per band the cost rule chooses.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quantization", "mxnet_amd", "csrc")
# (n, cin, cout, h, w, compute units) -> rows per band: MobileNet1.0 and MobileNet0.5's first pair on 256 CUs.  The cost is the
# rows the busiest CU dequantises.  Batch 128: 16 bands of 7 rows are 2048 = exactly two per workgroup, 8 per CU x 9 rows = 72
# (8 rows: 1792 bands on 1024 workgroups, two rounds on four workgroups per CU x 10 = 80); batch 64: 1024 bands, 4 per CU x 9 = 36
# (8 rows: 896 bands, 4 x 10); batch 32: 512 bands, 2 per CU x 9 = 18 (8 rows: 2 x 10; 4 rows: 896 bands, 4 x 6 = 24); batch 8: 224
# bands of 4 rows, one per CU x 6.  Planes of a few rows on an empty chip: one row per band.
PICKS = {(128, 32, 64, 112, 112, 256): 7, (64, 32, 64, 112, 112, 256): 7, (32, 32, 64, 112, 112, 256): 7,
         (128, 16, 32, 112, 112, 256): 7, (64, 16, 32, 112, 112, 256): 7, (32, 16, 32, 112, 112, 256): 7,
         (8, 32, 64, 112, 112, 256): 4, (2, 32, 64, 3, 256, 256): 1, (3, 32, 64, 17, 112, 256): 1}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("front_layout") / "front_layout_main")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "front_layout_main.cpp"), "-o", exe])
    args = [str(v) for key in PICKS for v in key]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
    maps, rows = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "map":
            maps[tuple(int(v) for v in f[1:5])] = tuple(int(v) for v in f[5:9])
        elif f[0] == "rows":
            rows[tuple(int(v) for v in f[1:7])] = int(f[7])
    return maps, rows


def _cases():
    for q in range(4, 65):
        for r in range(1, 9):
            for cin in (16, 32):
                for rb in sorted({r, 1, max(1, r - 1)}):
                    yield q, r, cin, rb


def test_every_admitted_band_was_walked(walk):
    maps, _ = walk
    assert sorted(maps) == sorted(_cases())


def test_the_slot_map_is_a_bijection_onto_the_band(walk):
    maps, _ = walk
    bad = [k for k, (bij, inside, _, _) in maps.items() if not (bij == 1 and inside == 1)]
    assert not bad, "(Q, R, Cin, rows of the band): %s" % bad[:8]


def test_no_store_of_phase_1_is_worse_than_two_way(walk):
    maps, _ = walk
    bad = {k: v[2] for k, v in maps.items() if v[2] > 2}
    assert not bad, "(Q, R, Cin, rows of the band) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]
    # MobileNet's row (Q = 28): two segments of ONE four-channel plane per half-wave - no conflict at all
    assert all(maps[(28, r, cin, r)][2] == 1 for r in range(1, 9) for cin in (16, 32))


def test_the_fragment_read_of_phase_2_is_conflict_free(walk):
    maps, _ = walk
    bad = {k: v[3] for k, v in maps.items() if v[3] != 1}
    assert not bad, "(Q, R, Cin, rows of the band) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]


def test_rows_per_band_by_the_cost_rule(walk):
    _, rows = walk
    assert rows == PICKS
