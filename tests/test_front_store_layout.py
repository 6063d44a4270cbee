"""The band buffer of the storing 1x1 with a front layer (csrc/fq_front_layout.h; fq_pw_stat.hip: pw_front_store_kernel) for 256
input channels - eight 32-channel slabs - walked on the host: tests/front_store_layout_main.cpp is compiled with the host compiler
against the very header the kernel includes and plays both phases lane by lane, phase 2 with lane = pixel as the storing kernel
reads it.  For Q = W / 4 = 3 .. 16 lanes per row, every R = 1 .. 8 rows per band, full and short bands, workgroups of four and of
eight wavefronts:
  * the (channel, pixel) -> byte map is a bijection onto the band, every byte inside the buffer the launch allocates, every byte
    stored exactly once by phase 1, and the sixteen bytes a lane gathers for slab kt in phase 2 are the channels
    32 kt + 16 h .. + 15 of its pixel;
  * under the LDS bank rule ((address / 4) mod 32, lanes 0-31 and 32-63 apart) no byte store of phase 1 puts more than two
    distinct dwords on a bank, and no fragment read of phase 2 more than one;
  * the dynamic LDS front_store_plan counts is what the kernel carves up, and fits - for every (Q, R) of the walk and for the
    shapes of the GPU tests.
No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quantization", "mxnet_amd", "csrc")
# (n, cin, cout, h, w, compute units, forced rows, forced wavefronts) -> (wavefronts, rows per band).
# MobileNet1.0's dw5 -> pw5 at batch 128 on 256 CUs: 17 408 bytes beside the band, a band of 7 or 8 rows is 61 440 bytes - two
# workgroups per CU either way; 7 rows are 512 bands in one round x 2 x 9 = 18 (8 rows: 2 x 10 = 20; 4 rows: 896 bands, 2 rounds x
# 2 x 6 = 24), and eight wavefronts hold four per SIMD where four hold two (18 against 18 x 1.2).
PLANS = {
    (128, 256, 256, 28, 28, 256, 0, 0): (8, 7),
    (128, 256, 256, 28, 28, 256, 4, 0): (8, 4),
    (128, 256, 256, 28, 28, 256, 0, 4): (4, 7),
    (32, 256, 256, 28, 28, 256, 0, 0): None,
    (3, 256, 256, 9, 28, 256, 4, 8): (8, 4),
    (2, 256, 256, 5, 36, 256, 0, 0): None,
    (2, 256, 256, 6, 12, 256, 0, 0): None,
    (1, 256, 256, 1, 28, 256, 0, 0): None,
    (2, 256, 256, 64, 256, 256, 0, 0): None,
}
# ... and every (Q, R) of the walk as a forced plan: W = 4 Q, eight rows, R rows per band asked for (clamped where the band does
# not fit the LDS: the count must still be the declared one)
GRID = [(2, 256, 256, 8, 4 * q, 256, r, 0) for q in range(3, 17) for r in range(1, 9)]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("front_store_layout") / "front_store_layout_main")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "front_store_layout_main.cpp"), "-o", exe])
    args = [str(v) for key in list(PLANS) + GRID for v in key]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
    maps, plans = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "map":
            maps[tuple(int(v) for v in f[1:5])] = tuple(int(v) for v in f[5:9])
        elif f[0] == "plan":
            plans[tuple(int(v) for v in f[1:9])] = tuple(int(v) for v in f[9:13])
    return maps, plans


def _cases():
    for q in range(3, 17):
        for r in range(1, 9):
            for rb in sorted({r, 1, max(1, r - 1)}):
                for nw in (4, 8):
                    yield q, r, rb, nw


def test_every_band_was_walked(walk):
    maps, plans = walk
    assert sorted(maps) == sorted(_cases()) and sorted(plans) == sorted(list(PLANS) + GRID)


def test_the_map_is_a_bijection_inside_the_buffer_and_a_fragment_is_its_slab(walk):
    maps, _ = walk
    bad = [k for k, (bij, inside, _, _) in maps.items() if not (bij == 1 and inside == 1)]
    assert not bad, "(Q, R, rows of the band, wavefronts): %s" % bad[:8]


def test_no_store_of_phase_1_is_worse_than_two_way(walk):
    maps, _ = walk
    bad = {k: v[2] for k, v in maps.items() if v[2] > 2}
    assert not bad, "(Q, R, rows of the band, wavefronts) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]


def test_the_fragment_reads_of_phase_2_are_conflict_free(walk):
    maps, _ = walk
    bad = {k: v[3] for k, v in maps.items() if v[3] != 1}
    assert not bad, "(Q, R, rows of the band, wavefronts) -> distinct dwords on one bank: %s" % sorted(bad.items())[:8]


def test_the_plan_counts_the_lds_the_kernel_declares(walk):
    _, plans = walk
    for key, (waves, rows, lds, declared) in plans.items():
        assert waves in (4, 8) and 1 <= rows <= min(8, key[3]), (key, waves, rows)
        assert lds == declared and 0 < lds <= 120 * 1024, (key, lds, declared)
        if PLANS.get(key) is not None:
            assert (waves, rows) == PLANS[key], (key, waves, rows)
        if key[6]:                                 # (forced rows: those, or fewer where the band does not fit beside the rest)
            assert rows <= min(key[6], key[3], 8) and (rows == min(key[6], key[3], 8) or key in GRID)
        if key[7]:
            assert waves == key[7]
