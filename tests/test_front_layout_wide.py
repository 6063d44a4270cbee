"""The band buffer of the front-layer statistic pass (csrc/fq_front_layout.h) for 64 and 128 input channels - two and four
32-channel slabs, the depthwise layer that closes one recompute pair recomputed in front of the next pair's 1x1 - walked on the
host: tests/front_layout_wide_main.cpp is compiled with the host compiler against the very header the kernel includes and plays
both phases lane by lane.  For Q = W / 4 = 7 .. 16 lanes per row (planes 28 to 64 wide), every R = 1 .. 8 rows per band, full
and short bands:
  * the (channel, pixel) -> byte map is a bijection onto the band, every byte inside the buffer pw_stat_launch allocates, every
    byte stored exactly once by phase 1, and the sixteen bytes a lane gathers for slab kt in phase 2 are the channels
    32 kt + 16 h .. + 15 of its pixel;
  * under the LDS bank rule ((address / 4) mod 32, lanes 0-31 and 32-63 apart) no byte store of phase 1 puts more than two
    distinct dwords on a bank, and no fragment read of phase 2 more than one;
and the rows per band the cost rule chooses for the two links of the model zoo.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quantization", "mxnet_amd", "csrc")
# (n, cin, cout, h, w, compute units) -> rows per band, by the rule's own arithmetic (rounds x workgroups per CU x (R + 2)):
# MobileNet1.0's pair 2 -> pair 3 (128 channels at 56 x 56, 33 280 bytes beside the band): bands of 7 and 8 rows (55 296 and
#   63 488 bytes) leave room for one workgroup per CU only - a single wavefront per SIMD - and are not considered; of the others
#   5 rows (38 912 bytes, two per CU) are 1536 bands in 3 rounds x 2 x 7 = 42 (6 rows: 3 x 2 x 8 = 48; 4 rows: 4 x 2 x 6 = 48;
#   3 rows: 5 x 2 x 5 = 50);
# MobileNet0.5's (64 channels, 12 544 bytes): 4 rows are 15 360 bytes, four workgroups per CU, 1792 bands in 2 rounds x 4 x 6 = 48
#   (7 rows: three per CU, 2 x 3 x 9 = 54; 5 rows: 2 x 4 x 7 = 56).
PICKS = {(128, 128, 128, 56, 56, 256): 5, (128, 64, 64, 56, 56, 256): 4}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("front_layout_wide") / "front_layout_wide_main")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "front_layout_wide_main.cpp"), "-o", exe])
    args = [str(v) for key in PICKS for v in key]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
    maps, rows = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "map":
            maps[tuple(int(v) for v in f[1:5])] = tuple(int(v) for v in f[5:9])
        elif f[0] == "rows":
            rows[tuple(int(v) for v in f[1:7])] = (int(f[7]), int(f[8]))
    return maps, rows


def _cases():
    for q in range(7, 17):
        for r in range(1, 9):
            for cin in (64, 128):
                for rb in sorted({r, 1, max(1, r - 1)}):
                    yield q, r, cin, rb


def test_every_band_was_walked(walk):
    maps, _ = walk
    assert sorted(maps) == sorted(_cases())


def test_the_map_is_a_bijection_inside_the_buffer_and_a_fragment_is_its_slab(walk):
    maps, _ = walk
    bad = [k for k, (bij, inside, _, _) in maps.items() if not (bij == 1 and inside == 1)]
    assert not bad, "(Q, R, Cin, rows of the band): %s" % bad[:8]


def test_no_store_of_phase_1_is_worse_than_two_way(walk):
    maps, _ = walk
    bad = {k: v[2] for k, v in maps.items() if v[2] > 2}
    assert not bad, "(Q, R, Cin, rows of the band) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]


def test_the_fragment_reads_of_phase_2_are_conflict_free(walk):
    maps, _ = walk
    bad = {k: v[3] for k, v in maps.items() if v[3] != 1}
    assert not bad, "(Q, R, Cin, rows of the band) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]


def test_rows_per_band_by_the_cost_rule_and_the_launch_fits_the_lds(walk):
    _, rows = walk
    assert {k: v[0] for k, v in rows.items()} == PICKS
    assert all(0 < v[1] <= 120 * 1024 for v in rows.values()), rows
