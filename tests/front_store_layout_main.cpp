// Stand-alone walk over the band buffer of the STORING 1x1 with a front layer (csrc/fq_front_layout.h, fq_pw_stat.hip:
// pw_front_store_kernel) for 256 input channels - eight 32-channel slabs - compiled and run by tests/test_front_store_layout.py.
// Plays both phases of the kernel on the host, lane by lane, with the functions the kernel itself calls, for workgroups of four
// and of eight wavefronts, and prints per (Q, R, rows of the band, wavefronts):
//   map   Q R RB NW  bijection(0/1)  inside(0/1)  store_ways  read_ways
// store_ways / read_ways: the most DISTINCT dwords any wave-instruction of phase 1 / phase 2 puts on one of the 32 LDS banks
// ((address / 4) mod 32), lanes 0-31 and 32-63 taken separately.  Phase 2 here has lane = pixel: lane (i32, h) reads pixel
// 32 tile + i32 (the statistic pass reads pixel 32 tile + mfma_row_pixel(i32): the same 32 pixels in another order).
//   plan  N CIN COUT H W CUS FORCED_ROWS FORCED_WAVES  waves rows lds declared
// front_store_plan's choice for a shape, and `declared`: the dynamic LDS as the kernel carves it up - Cout ints and 4 x Cout floats
// of constants, 12 floats per input channel, Cin / 4 planes of lay.pl dwords.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "fq_front_layout.h"

using namespace fqi;

static int worst_bank(const std::vector<int>& dwords) {
  std::set<int> per_bank[32];
  for (int d : dwords) per_bank[d & 31].insert(d);
  size_t w = 0;
  for (const auto& s : per_bank) w = std::max(w, s.size());
  return (int)w;
}

static void walk(int q, int rows, int rb, int nw) {
  const int cin = 256, kts = cin / 32;
  const FrontLayout lay = front_layout(q, rows);
  const int segs = 64 / q, npix = rb * 4 * q;
  const size_t bytes = front_band_bytes(q, rows, cin);
  std::vector<int> hits(bytes, 0);
  bool inside = true;
  int store_ways = 0, read_ways = 0;
  // phase 1: per channel turn (nw * segs channels), wavefront, output row and column j one byte store of all lanes
  for (int c0 = 0; c0 < cin; c0 += nw * segs)
    for (int wave = 0; wave < nw; ++wave)
      for (int row = 0; row < rb; ++row)
        for (int j = 0; j < 4; ++j)
          for (int half = 0; half < 2; ++half) {
            std::vector<int> dwords;
            for (int lane = 32 * half; lane < 32 * half + 32; ++lane) {
              const int seg = lane / q, pos = lane - seg * q;
              const int c = front_channel(c0, wave, segs, seg);
              if (!(seg < segs && c < cin)) continue;
              const int a = front_byte(lay, c, 4 * (row * q + pos) + j);
              if (a < 0 || (size_t)a >= bytes) {
                inside = false;
                continue;
              }
              ++hits[a];
              dwords.push_back(a >> 2);
            }
            store_ways = std::max(store_ways, worst_bank(dwords));
          }
  // every (channel, pixel) of the band exactly one byte: a bijection onto cin * npix bytes, each stored exactly once
  bool bij = true;
  std::set<int> seen;
  for (int c = 0; c < cin; ++c)
    for (int p = 0; p < npix; ++p) {
      const int a = front_byte(lay, c, p);
      if (a < 0 || (size_t)a >= bytes || hits[a] != 1 || !seen.insert(a).second) bij = false;
    }
  long total = 0;
  for (int v : hits) total += v;
  if (total != (long)cin * npix || seen.size() != (size_t)cin * npix) bij = false;
  // phase 2: per tile, slab kt and plane u one dword read of all lanes; lane (i32, h) reads plane 8 kt + 4 h + u of pixel
  // 32 tile + i32 - and the sixteen bytes it gathers must be the channels 32 kt + 16 h .. + 15 of that pixel
  for (int tl = 0; tl < (npix + 31) / 32; ++tl)
    for (int kt = 0; kt < kts; ++kt)
      for (int u = 0; u < 4; ++u)
        for (int h = 0; h < 2; ++h) {
          std::vector<int> dwords;
          for (int i32 = 0; i32 < 32; ++i32) {
            const int pp = std::min(tl * 32 + i32, npix - 1);
            const int a = front_byte(lay, 16 * h, pp) + 4 * (8 * kt + u) * lay.pl;
            if (a < 0 || (size_t)a + 4 > bytes) inside = false;
            for (int b = 0; b < 4; ++b)
              if (a + b != front_byte(lay, 32 * kt + 16 * h + 4 * u + b, pp)) bij = false;
            dwords.push_back(a >> 2);
          }
          read_ways = std::max(read_ways, worst_bank(dwords));
        }
  printf("map %d %d %d %d %d %d %d %d\n", q, rows, rb, nw, bij ? 1 : 0, inside ? 1 : 0, store_ways, read_ways);
}

int main(int argc, char** argv) {
  for (int q = 3; q <= 16; ++q)
    for (int rows = 1; rows <= kFrontRows; ++rows)
      for (int nw = kFrontWaves; nw <= kFrontWavesWide; nw += kFrontWavesWide - kFrontWaves) {
        walk(q, rows, rows, nw);
        if (rows > 1) walk(q, rows, 1, nw);                   // the short last band of a plane
        if (rows > 2) walk(q, rows, rows - 1, nw);
      }
  for (int i = 1; i + 7 < argc; i += 8) {
    const long n = atol(argv[i]), cin = atol(argv[i + 1]), cout = atol(argv[i + 2]), h = atol(argv[i + 3]), w = atol(argv[i + 4]);
    const int cus = atoi(argv[i + 5]), fr = atoi(argv[i + 6]), fw = atoi(argv[i + 7]);
    const FrontPlan p = front_store_plan(n, cin, cout, h, w, cus, kFrontWgCap, fr, fw);
    size_t declared = 0;
    if (p.rows >= 1)
      declared = (size_t)cout * sizeof(int) + 4 * (size_t)cout * sizeof(float) + (size_t)cin * 12 * sizeof(float) +
                 (size_t)(cin / 4) * front_layout((int)(w / 4), p.rows).pl * 4;
    printf("plan %ld %ld %ld %ld %ld %d %d %d %d %d %zu %zu\n", n, cin, cout, h, w, cus, fr, fw, p.waves, p.rows, p.lds, declared);
  }
  return 0;
}
