// Stand-alone walk over the workgroup size and the rows per band of the front-layer statistic pass (csrc/fq_front_layout.h:
// front_waves_pick, front_rows_pick), compiled and run by tests/test_front_waves.py.  Arguments: N CIN COUT H W CUS, repeated.
// Per shape it prints what front_plan - the function pw_stat_launch takes its workgroup size, rows and LDS from - answers,
//   pick N CIN COUT H W CUS  WAVES  ROWS  LDS  WAVES_PER_SIMD   ROWS4 COST4 ROWS8 COST8
// and what it answers to the knobs FQ_PWSTAT_FRONT_ROWS = 1, 5, 7, 8 with FQ_PWSTAT_FRONT_WAVES = 4 and 8,
//   forced N CIN COUT H W CUS  ROWS_ASKED WAVES_ASKED  WAVES ROWS LDS
// and it plays phase 1 and phase 2 of a band for that workgroup size with the functions the kernel calls:
//   turn N CIN COUT H W CUS  channels_once(0/1)  tiles_once(0/1)
// - every channel of the band is owned by exactly one (turn, wavefront, segment), every 32-pixel tile by exactly one wavefront.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fq_front_layout.h"

using namespace fqi;

int main(int argc, char** argv) {
  for (int i = 1; i + 5 < argc; i += 6) {
    const long n = atol(argv[i]), cin = atol(argv[i + 1]), cout = atol(argv[i + 2]), h = atol(argv[i + 3]), w = atol(argv[i + 4]);
    const int cus = atoi(argv[i + 5]), q = (int)(w / 4), cap = kFrontWgCap;
    const size_t f4 = front_fixed_lds(cin, cout, kFrontWaves), f8 = front_fixed_lds(cin, cout, kFrontWavesWide);
    double c4 = 0.0, c8 = 0.0;
    const int r4 = front_rows_pick(n, h, w, (int)cin, f4, cus, cap, 0, kFrontWaves, &c4);
    const int r8 = front_rows_pick(n, h, w, (int)cin, f8, cus, cap, 0, kFrontWavesWide, &c8);
    const FrontPlan plan = front_plan(n, cin, cout, h, w, cus);
    const int waves = plan.waves, rows = plan.rows;
    const size_t lds = plan.lds;
    const int wps = stat_wg_per_cu(lds, stat_wg_cap(cap, waves)) * waves / 4;
    printf("pick %ld %ld %ld %ld %ld %d %d %d %zu %d %d %.2f %d %.2f\n", n, cin, cout, h, w, cus, waves, rows, lds, wps, r4, c4, r8, c8);
    for (int fr : {1, 5, 7, 8})
      for (int fw : {kFrontWaves, kFrontWavesWide}) {
        const FrontPlan f = front_plan(n, cin, cout, h, w, cus, kFrontWgCap, fr, fw);
        printf("forced %ld %ld %ld %ld %ld %d %d %d %d %d %zu\n", n, cin, cout, h, w, cus, fr, fw, f.waves, f.rows, f.lds);
      }
    // phase 1: the channels of a band over turns, wavefronts and segments; phase 2: its tiles over the wavefronts
    const int segs = 64 / q;
    std::vector<int> owners((size_t)cin, 0);
    for (int c0 = 0; c0 < cin; c0 += waves * segs)
      for (int wave = 0; wave < waves; ++wave)
        for (int seg = 0; seg < segs; ++seg) {
          const int c = front_channel(c0, wave, segs, seg);
          if (c < cin) ++owners[(size_t)c];
        }
    bool channels_once = true;
    for (int v : owners) channels_once = channels_once && v == 1;
    const int ntile = (int)((rows * w + 31) / 32);
    std::vector<int> tiles((size_t)ntile, 0);
    for (int wave = 0; wave < waves; ++wave)
      for (int tl = wave; tl < ntile; tl += waves) ++tiles[(size_t)tl];
    bool tiles_once = true;
    for (int v : tiles) tiles_once = tiles_once && v == 1;
    printf("turn %ld %ld %ld %ld %ld %d %d %d\n", n, cin, cout, h, w, cus, channels_once ? 1 : 0, tiles_once ? 1 : 0);
  }
  return 0;
}
