// libfakequant - the band buffer of the front-layer statistic pass (fq_pw_stat.hip: pw_stat_kernel with FEPI >= 0) and the rows
// a band gets.  Plain C++ as well as HIP: tests/front_layout_main.cpp compiles this file alone and walks every admitted shape.
//
// The buffer holds the codes of one band - R rows of W = 4 Q pixels, Cin channels - between the two phases of the kernel:
//   1  lane (seg, pos) of a wavefront owns channel front_channel(c0, wave, segs, seg) and the four columns 4 pos .. 4 pos + 3 of
//      a row; per row it writes four bytes, column j of all lanes in one wave-instruction;
//   2  lane (i32, h) reads the 16 channels 32 kt + 16 h .. + 15 of pixel 32 tile + mfma_row_pixel(i32): its MFMA A fragment of
//      slab kt (Cin / 32 slabs: one for 16 and 32 channels, two and four for 64 and 128).
// LDS has 32 banks of 4 bytes, a wave-instruction is served as lanes 0-31 and 32-63, and two lanes conflict when they touch
// DIFFERENT dwords of one bank.  In C16 order ([16-channel block][pixel][16 bytes]) the lanes of phase 1 are 64 bytes apart:
// two banks for up to 32 lanes.  Here instead
//   byte(c, p) = 4 * ((c >> 2) * pl + front_slot(p)) + (c & 3),      front_slot(p) = (p & 3) * js + (p >> 2)
// - four-channel planes of dwords, inside a plane the four columns j = p & 3 de-interleaved:
//   phase 1: the lanes of a row segment write CONSECUTIVE dwords (p >> 2 = row * Q + pos), four neighbouring channels the four
//            bytes of one dword; a half-wave meets at most three planes, each a run of at most 32 dwords: never more than two
//            dwords on a bank (pl = 16 mod 32 keeps two planes of short rows apart);
//   phase 2: the 32 pixels of a tile are 8 consecutive p >> 2 for each of the four j: four runs of 8 dwords, js apart - with
//            js = 8 mod 16 they fall on 32 different banks.  The fragment is four dword reads, one per plane 8 kt + 4 h .. + 3
//            (a plane further on moves every lane by the same pl dwords: what holds for one plane holds for all).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FQ_FL_FN __host__ __device__ __forceinline__
#else
#define FQ_FL_FN inline
#endif

namespace fqi {

constexpr int kFrontRows = 8;                  // most rows of a band (the kernel keeps kFrontRows + 2 input rows in registers)
constexpr int kFrontBandBytes = 32768;         // most codes of a band PER 32-CHANNEL SLAB: rows * W * 32 (64 and 128 channels:
                                               // two and four times as much, and the LDS limit below decides)
constexpr int kStatLdsPerCU = 160 * 1024, kStatLdsMax = 120 * 1024;

struct FrontLayout {
  int js;                                      // dwords between the column planes j = 0 .. 3 (>= rows * Q, = 8 mod 16)
  int pl;                                      // dwords between the four-channel planes (= 16 mod 32)
};

FQ_FL_FN FrontLayout front_layout(int q, int rows) {
  FrontLayout l;
  l.js = rows * q + ((8 - rows * q) & 15);
  l.pl = 4 * l.js + 16;
  return l;
}

// pixel p of the band (row-major, rows of 4 Q pixels) -> its dword inside a four-channel plane.  THE map: both phases call it.
FQ_FL_FN int front_slot(FrontLayout l, int p) { return (p & 3) * l.js + (p >> 2); }

FQ_FL_FN int front_byte(FrontLayout l, int c, int p) { return (((c >> 2) * l.pl + front_slot(l, p)) << 2) + (c & 3); }

inline size_t front_band_bytes(int q, int rows, int cin) { return (size_t)((cin + 3) / 4) * front_layout(q, rows).pl * 4; }

// phase 1: the channel of segment `seg` of wavefront `wave` in the turn that starts at channel c0 (waves * segs channels per
// turn: a workgroup has kFrontWaves = 4 wavefronts, or kFrontWavesWide = 8 - front_waves_pick below)
FQ_FL_FN int front_channel(int c0, int wave, int segs, int seg) { return c0 + wave * segs + seg; }

constexpr int kFrontWaves = 4, kFrontWavesWide = 8;

// the tile pixel of MFMA row i32 (row 8 g + 4 h + i holds pixel 16 h + 4 g + i: a lane's 16 registers are 16 consecutive pixels)
FQ_FL_FN int mfma_row_pixel(int i32) { return 16 * ((i32 >> 2) & 1) + 4 * (i32 >> 3) + (i32 & 3); }

// persistent workgroups of the statistic pass per CU: by LDS, at most `cap` (registers)
inline int stat_wg_per_cu(size_t lds, int cap) {
  const int by_lds = (int)((size_t)kStatLdsPerCU / (lds + 1024));
  return by_lds > cap ? cap : (by_lds < 1 ? 1 : by_lds);
}

// the cap on workgroups per CU for workgroups of `waves` wavefronts, from the cap for workgroups of four
inline int stat_wg_cap(int cap4, int waves) {
  const int cap = cap4 * kFrontWaves / waves;
  return cap < 1 ? 1 : cap;
}

// Rows per band.  A band of R rows dequantises R + 2 input rows, and the n * ceil(h / R) bands go round by round over the
// workgroups launched (stat_wg_per_cu of them per CU, fewer when there are fewer bands).  The kernel is bound by its vector
// instructions, which the workgroups of a CU share: the cost of a choice is the rows the busiest CU dequantises,
// rounds * ceil(workgroups / CUs) * (R + 2).  On a full chip that is pwdw_plan's rounds * (R + 2); on a chip that the bands
// do not fill it does NOT divide by the fill as pwdw_plan does - that prefers many short bands, and measured at batch 32 four
// rows per band lose to eight (49.8 against 47.3 us, 44.1 against 39.9 on 16 channels: profiles/front_stat_alone.txt).  Among
// equal costs a band of whole 32-pixel tiles wins, then the longer one.  MobileNet's 112 x 112 plane at batch 128 on 256 CUs:
// R = 8 is 1792 bands on 1024 workgroups - two rounds of 10 rows where the mean is 1.75 - and R = 7 is 2048 bands, two rounds of 9.
// The rule takes the vector instructions for the bound, which holds while something hides a latency: a band so large that only
// ONE workgroup fits a CU leaves each SIMD a single wavefront, and every load of phase 1 and every fragment read of phase 2 is
// waited for in full (128 channels at 56 x 56, batch 128: 7 rows - one workgroup per CU, 36 by the rule - take 125 us, 5 rows -
// two per CU, 42 by the rule - 102 us: profiles/pair_chain_alone.txt).  So where some band leaves room for two workgroups, no
// longer band is considered.
// `lds_fixed`: what the launch needs beside the band buffer; `forced` > 0: that many rows (clamped), the tuning knob.
// 0 when no band fits (the caller refuses the shape).
// `waves`: wavefronts per workgroup.  What hides a latency is the wavefronts on a SIMD, workgroups * waves / 4, not the workgroups
// on the CU: `wg_cap` counts workgroups of FOUR wavefronts (= wavefronts per SIMD the registers admit), a workgroup of eight
// counts twice against it, and "room for two workgroups" above reads "two wavefronts per SIMD" - which ONE workgroup of eight is.
// `lds_fixed` is the caller's figure for that many wavefronts (each has a max / min table).
// Below four wavefronts per SIMD a row costs more: forced rows 1 .. 8 at both workgroup sizes (128 channels at 56 x 56, batch 128,
// profiles/front_waves_sweep.txt) give 1.84-2.0 us per row of the rule at four wavefronts per SIMD and 2.2-2.4 us at two - eight
// wavefronts on 5 rows (42 by the rule) take 84 us, on 7 rows (36, one workgroup per CU) 87 us.  Hence front_occupancy_cost: 1.2
// at two wavefronts per SIMD and 1.0 at four are MEASURED; 1.1 at three is an interpolation that no sweep has covered.
// Where the factor counts: among the bands of a workgroup of EIGHT, which holds two or four wavefronts per SIMD and nothing
// else (the two measured points), and in front_waves_pick's comparison of the two workgroup sizes.  Among the bands of a
// workgroup of four the rule is the plain one, so every pick of four wavefronts - 16 and 32 channels, odd shapes - is what it
// was before there were workgroups of eight; the unmeasured 1.1 can tip the choice between four and eight wavefronts only.
// `cost_out`: the cost of the choice with its factor, for front_waves_pick.
inline double front_occupancy_cost(int waves_per_simd) { return waves_per_simd >= 4 ? 1.0 : (waves_per_simd == 3 ? 1.1 : 1.2); }

inline int front_rows_pick(int64_t n, int64_t h, int64_t w, int cin, size_t lds_fixed, int num_cu, int wg_cap, int forced = 0,
                           int waves = kFrontWaves, double* cost_out = nullptr) {
  const int q = (int)(w / 4);
  wg_cap = stat_wg_cap(wg_cap, waves);
  int rmax = (int)(kFrontBandBytes / (32 * w));
  rmax = rmax > kFrontRows ? kFrontRows : rmax;
  rmax = rmax > h ? (int)h : rmax;
  while (rmax >= 1 && lds_fixed + front_band_bytes(q, rmax, cin) > (size_t)kStatLdsMax) --rmax;
  if (rmax < 1) return 0;
  if (forced > 0) return forced < rmax ? forced : rmax;
  {
    int r2 = rmax;
    while (r2 >= 1 && stat_wg_per_cu(lds_fixed + front_band_bytes(q, r2, cin), wg_cap) * waves < 2 * 4) --r2;
    if (r2 >= 1) rmax = r2;
  }
  double best = 1e30, best_with_occ = 1e30;
  int best_r = rmax;
  bool best_whole = false;
  for (int r = rmax; r >= 1; --r) {
    const int64_t wgs = n * ((h + r - 1) / r);
    const int per_cu = stat_wg_per_cu(lds_fixed + front_band_bytes(q, r, cin), wg_cap);
    const int64_t slots = (int64_t)num_cu * per_cu;
    const int64_t grid = wgs < slots ? wgs : slots, rounds = (wgs + grid - 1) / grid;
    const double plain = (double)(rounds * ((grid + num_cu - 1) / num_cu) * (r + 2)), occ = front_occupancy_cost(per_cu * waves / 4);
    const double cost = waves > kFrontWaves ? plain * occ : plain;
    const bool whole = (r * w) % 32 == 0;
    if (cost < best - 1e-9 || (cost < best + 1e-9 && whole && !best_whole)) {
      best = cost;
      best_with_occ = plain * occ;
      best_r = r;
      best_whole = whole;
    }
  }
  if (cost_out != nullptr) *cost_out = best_with_occ;
  return best_r;
}

// Wavefronts per workgroup.  The band buffer, the weights and the tables decide how many workgroups a CU holds, and with four
// wavefronts each that is also the wavefronts per SIMD: two for 128 channels at 56 x 56 (5 rows), three or four for 64.  Eight
// wavefronts on the same band fill the SIMDs without a shorter band's halo rows, and what a wavefront waits for - the loads of
// phase 1, the fragment reads of phase 2, the barrier between them - is hidden by three others instead of one.  The choice is the
// cheaper of the two by the rule above, each with its own rows: 128 channels - eight wavefronts on 5 rows (42 against 42 x 1.2),
// 84 us where four took 96; 64 channels - eight on 7 rows (36 against 48 for four on 4 rows), 54.5 us against 60.5; 16 and 32
// channels fit four workgroups of four anyway and have no instantiation of eight (profiles/front_waves_sweep.txt).
// `lds_fixed4`, `lds_fixed8`: the fixed LDS of a launch with four and with eight wavefronts.
inline int front_waves_pick(int64_t n, int64_t h, int64_t w, int cin, size_t lds_fixed4, size_t lds_fixed8, int num_cu, int wg_cap) {
  double c4 = 0.0, c8 = 0.0;
  const int r4 = front_rows_pick(n, h, w, cin, lds_fixed4, num_cu, wg_cap, 0, kFrontWaves, &c4);
  const int r8 = front_rows_pick(n, h, w, cin, lds_fixed8, num_cu, wg_cap, 0, kFrontWavesWide, &c8);
  return r8 >= 1 && (r4 < 1 || c8 < c4) ? kFrontWavesWide : kFrontWaves;
}

// LDS of the statistic pass beside a front layer's band: weight fragments, per-channel constants, one max / min table per
// wavefront (kt, ct: 32-channel slabs of the input and of the output)
inline size_t stat_fixed_lds(int kt, int ct, int waves = kFrontWaves) {
  return (size_t)ct * kt * 1024 + 5 * (size_t)ct * 32 * 4 + (size_t)waves * ct * 128 * 4;
}

// ... and with a front layer: its weights, bias and BatchNorm constants, 12 floats per channel
inline size_t front_fixed_lds(int64_t cin, int64_t cout, int waves) {
  return stat_fixed_lds((int)((cin + 31) / 32), (int)((cout + 31) / 32), waves) + (size_t)cin * 12 * 4;
}

constexpr int kFrontWgCap = 4;          // (by registers: the front-layer instantiations fit four wavefronts per SIMD)

// What a launch of the front-layer mode runs with: wavefronts per workgroup, rows per band (0: no band fits, the shape is
// refused), its dynamic LDS.  Eight wavefronts are instantiated for 64 and 128 channels (16 and 32 leave a CU four workgroups of
// four anyway); a shape whose band fits with four tables only stays with four, forced or not.
// `forced_rows`, `forced_waves`: the tuning knobs (0: the rules above); `wg_cap`: kFrontWgCap unless a knob says otherwise.
struct FrontPlan {
  int waves, rows;
  size_t lds;
};
inline FrontPlan front_plan(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, int num_cu, int wg_cap = kFrontWgCap,
                            int forced_rows = 0, int forced_waves = 0) {
  FrontPlan p;
  p.waves = kFrontWaves;
  if (cin >= 64) {
    if (forced_waves == kFrontWaves || forced_waves == kFrontWavesWide) p.waves = forced_waves;
    else p.waves = front_waves_pick(n, h, w, (int)cin, front_fixed_lds(cin, cout, kFrontWaves),
                                    front_fixed_lds(cin, cout, kFrontWavesWide), num_cu, wg_cap);
  }
  p.rows = front_rows_pick(n, h, w, (int)cin, front_fixed_lds(cin, cout, p.waves), num_cu, wg_cap, forced_rows, p.waves);
  if (p.rows < 1 && p.waves != kFrontWaves) {
    p.waves = kFrontWaves;
    p.rows = front_rows_pick(n, h, w, (int)cin, front_fixed_lds(cin, cout, p.waves), num_cu, wg_cap, forced_rows, p.waves);
  }
  p.lds = p.rows >= 1 ? front_fixed_lds(cin, cout, p.waves) + front_band_bytes((int)(w / 4), p.rows, (int)cin) : 0;
  return p;
}

// ---- the STORING 1x1 with a front layer (fq_pw_stat.hip: pw_front_store_kernel, fq_pwconv_i8_front) ------------------------------
// The same band buffer and the same phase 1; phase 2 takes the band's pixels as the B operand (lane = pixel: a channel's 32
// pixels leave as one 128-byte run) and keeps the weight fragments in registers, so beside the band the launch holds only the
// epilogue's per-channel constants (five words per output channel) and the front layer's 12 floats per input channel - no weight
// fragments, no max / min tables, whatever the workgroup size.
inline size_t front_store_fixed_lds(int64_t cin, int64_t cout) { return (size_t)cout * 5 * 4 + (size_t)cin * 12 * 4; }

// front_plan's rules with that fixed part: eight wavefronts against four by front_waves_pick, rows by front_rows_pick.
inline FrontPlan front_store_plan(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, int num_cu, int wg_cap = kFrontWgCap,
                                  int forced_rows = 0, int forced_waves = 0) {
  const size_t fixed = front_store_fixed_lds(cin, cout);
  FrontPlan p;
  if (forced_waves == kFrontWaves || forced_waves == kFrontWavesWide) p.waves = forced_waves;
  else p.waves = front_waves_pick(n, h, w, (int)cin, fixed, fixed, num_cu, wg_cap);
  p.rows = front_rows_pick(n, h, w, (int)cin, fixed, num_cu, wg_cap, forced_rows, p.waves);
  p.lds = p.rows >= 1 ? fixed + front_band_bytes((int)(w / 4), p.rows, (int)cin) : 0;
  return p;
}

}  // namespace fqi
