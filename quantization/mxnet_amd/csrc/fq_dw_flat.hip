// libfakequant — K2p depthwise 3x3 with quantise-on-load: small planes as flat 16-byte ranges through an LDS transpose
#include "fq_dw.h"      // what the depthwise forms share; fq_common.h: the list of units, the design rules

namespace {
// K2p: small planes through an LDS transpose.  The column-walking forms (fq_dw_cols.hip, fq_dw_planes.hip) read and write a plane row by row: every
// memory instruction of a wavefront touches 56-byte pieces of 4-9 different planes (9-18 cache lines, each of them again
// by the next two rows), and the kernel is bound by the rate at which the CU's memory pipeline takes such instructions
// (tools/dw_trace.py: 26 loads per wavefront take 2.5 us to ISSUE when 12 wavefronts per CU do it together; no loads /
// no stores ablation: 21 of 25 us remain).  Here a wavefront moves its P planes (one contiguous P * H * W * 4 byte range)
// with 16 bytes per lane on consecutive addresses - every cache line is touched once, by one instruction:
//   A  flat range -> registers (requested ONE BLOCK AHEAD) -> quantise (no neighbours needed) -> wavefront-private LDS tile
//   B  lane = (plane, column pair): walk down the rows reading the tile (8 bytes per lane and row), 3x3 sums as packed
//      fp32 FMA chains, epilogue, result written over the tile row just consumed
//   C  tile -> registers -> flat 16-byte stores
// No workgroup barrier: a wavefront only ever touches its own tile (LDS operations of a wavefront complete in order).
// Phase boundary of the flat form: compiler-level ordering only (LDS operations of one wavefront execute in order).
#define FQ_DWF_PHASE()                                             \
  do {                                                             \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         \
    __builtin_amdgcn_wave_barrier();                               \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");         \
  } while (0)

struct DwFlatGeom {
  int C;
  unsigned planes;          // n * c
  unsigned per, rem;        // workgroup b works on blocks [b * per + min(b, rem), ...) - per + (b < rem) of them
  FastDiv by_c;             // plane % C, plane / C
};

template <int S, bool QUANT, bool ONLINE, int H, int W, int EPI>
__global__ __launch_bounds__(kBlock) void dwconv3x3_flat_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwFlatGeom g, const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr,
    float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out, const float* __restrict__ bn_scale,
    const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  // phase B shapes: PAIR - stride 1, even W: two columns per lane, packed FMA chains, in place;
  //                 ONE  - stride 1, odd W: one column per lane, in place;  DOWN - stride 2 (even W): one OUTPUT column per lane
  constexpr bool PAIR = S == 1 && W % 2 == 0, DOWN = S == 2;
  static_assert(S == 1 || W % 2 == 0, "stride 2 reads column pairs");
  constexpr int HO = (H - 1) / S + 1, WO = (W - 1) / S + 1;
  constexpr int IN = H * W, OUT = HO * WO;           // floats per plane
  constexpr int LPP = DOWN ? WO : (PAIR ? W / 2 : W);      // lanes per plane in phase B
  constexpr int PMAX = 64 / LPP;
  // planes per wavefront and block: the flat ranges must be whole 16-byte groups (planes of 49 floats: multiples of 4 planes)
  constexpr int P = (IN % 4 == 0 && OUT % 4 == 0) ? PMAX : PMAX / 4 * 4;
  static_assert(P >= 1 && (P * IN) % 4 == 0 && (P * OUT) % 4 == 0, "no 16-byte flat range for this plane size");
  constexpr bool TAIL_OK = IN % 4 == 0 && OUT % 4 == 0;  // else the host only takes tensors of whole blocks (planes % P == 0)
  constexpr int NFI = P * IN / 4, NFO = P * OUT / 4;   // 16-byte groups per wavefront and block, in / out
  constexpr int NLI = (NFI + 63) / 64, NLO = (NFO + 63) / 64;
  constexpr unsigned kOob = 0x80000000u;   // beyond every resource of this kernel (host: tensors < 2 GiB)
  __shared__ f4 tile[kBlock / 64][NLI * 64];
  __shared__ f4 otile[kBlock / 64][DOWN ? NLO * 64 : 1];  // stride 1 writes its results over the tile rows already consumed
  __shared__ unsigned k_stat[kDwStatSlots];
  if (threadIdx.x < kDwStatSlots) k_stat[threadIdx.x] = 0u;
  PW_STAMP(0);
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned b = blockIdx.x;
  const unsigned blk_begin = b * g.per + (b < g.rem ? b : g.rem);
  const unsigned blk_end = blk_begin + g.per + (b < g.rem ? 1u : 0u);
  const unsigned planes = g.planes;
  const unsigned n_samples = (unsigned)n;
  unsigned s_base;
  {
    const unsigned p0 = blk_begin * (P * (kBlock / 64));
    s_base = fast_div(p0 < planes ? p0 : planes - 1, g.by_c);
  }
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr, has_bias = bias != nullptr;
  const fq_rsrc rx = make_rsrc(x, (int64_t)planes * IN * 4), ry = make_rsrc(y, (int64_t)planes * OUT * 4);
  const fq_rsrc rw = make_rsrc(wgt, (int64_t)g.C * 36);
  // phase B coordinates of this lane
  const unsigned j = lane / LPP, pos = lane - j * LPP;
  const bool b_lane = lane < P * LPP;
  const bool first = pos == 0, last = pos == LPP - 1;
  float* const my_tile = reinterpret_cast<float*>(tile[wave]);
  float* const my_out = DOWN ? reinterpret_cast<float*>(otile[wave]) : my_tile;

  struct Blk {
    f4 raw[NLI];
    f4 w03, w47;
    float w8, bch, bsc, bsh;
  };
  auto issue = [&](unsigned blk, Blk& k) __attribute__((always_inline)) {
    const unsigned base = (blk * (kBlock / 64) + wave) * P;                  // first plane of this wavefront (uniform)
    const unsigned left = base < planes ? planes - base : 0u;
    const unsigned np = left < (unsigned)P ? left : (unsigned)P;
    const unsigned lim = TAIL_OK ? np * (IN / 4) : (np == (unsigned)P ? (unsigned)NFI : 0u);   // 16-byte groups that exist
    // nontemporal: the input (a 26-103 MB tensor the producer left in the Infinity Cache) is read once - +0.9 % images/s with
    // three batches in flight, five alternating runs (profiles/r5_nt_sweep3.txt)
#pragma unroll
    for (int i = 0; i < NLI; ++i)
      k.raw[i] = buf_ld_v4f_nt(rx, (lane + 64u * i) < lim ? lane * 16u : kOob, base * (IN * 4u) + 1024u * i);
    const unsigned ch = (b_lane && j < left) ? fast_mod(base + j, g.by_c) : 0u;
    k.w03 = buf_ld_v4f(rw, ch * 36u, 0);
    k.w47 = buf_ld_v4f(rw, ch * 36u, 16);
    k.w8 = buf_ld_f32(rw, ch * 36u, 32);
    k.bch = has_bias ? bias[ch] : 0.0f;
    k.bsc = has_bn ? bn_scale[ch] : 1.0f;
    k.bsh = has_bn ? bn_shift[ch] : 0.0f;
  };

  Blk nxt;
  ThresholdReq treq;
  if (QUANT) treq = threshold_request(in_stat, n, ONLINE ? nullptr : in_thr, blockIdx.x == 0);   // first in the memory queue
  FQ_PIN();
  PW_STAMP(6);
  if (blk_begin < blk_end) issue(blk_begin, nxt);
  FQ_PIN();
  PW_STAMP(7);
  QParams q = {};
  if (QUANT)                                              // while the first block is on its way
    q = dw_qparams_finish<ONLINE>(treq, in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
  PW_STAMP(1);
  __syncthreads();                                        // statistic table zeroed
  for (unsigned blk = blk_begin; blk < blk_end; ++blk) {
    if (blk == blk_begin + 1) PW_STAMP(2);
    Blk cur = nxt;
    FQ_PIN();
    if (blk + 1 < blk_end) issue(blk + 1, nxt);
    FQ_PIN();
    const unsigned base = (blk * (kBlock / 64) + wave) * P;
    const unsigned left = base < planes ? planes - base : 0u;
    const unsigned np = left < (unsigned)P ? left : (unsigned)P;
    const unsigned lim_out = TAIL_OK ? np * (OUT / 4) : (np == (unsigned)P ? (unsigned)NFO : 0u);
    // (phases A and B of the PAIR shape have a TWIN, word for word: dwconv3x3_flat_stat_kernel below, the statistic pass - a change
    // to the quantiser, the tap chain or the epilogue here is a change there; tests/test_gpu_front_store.py compares the two)
    // ---- A: quantise in flat order, stage ---------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < NLI; ++i) {
      f4 v = cur.raw[i];
      if (QUANT) v = fq_code4(v, q) * q.scale;
      tile[wave][lane + 64 * i] = v;
    }
    FQ_DWF_PHASE();
    // ---- B: 3x3 on the tile ----------------------------------------------------------------------------------------------
    float m = 0.0f;
    const bool is_out = b_lane && j < left;
    if (b_lane) {
      const f4 w03 = cur.w03, w47 = cur.w47;
      if (PAIR) {
        float* lp = my_tile + j * IN + pos * 2;
        f2 aL = {0.f, 0.f}, aC = {0.f, 0.f}, aR = {0.f, 0.f};     // row r-1: (L, q0), (q0, q1), (q1, R)
        f2 bL, bC, bR;
        {
          const f2 v = *reinterpret_cast<const f2*>(lp);
          bL = (f2){left_of(v.y, first), v.x};
          bC = v;
          bR = (f2){v.y, right_of(v.x, last)};
        }
#pragma unroll
        for (int r = 0; r < H; ++r) {
          f2 cL = {0.f, 0.f}, cC = {0.f, 0.f}, cR = {0.f, 0.f};
          if (r + 1 < H) {
            const f2 v = *reinterpret_cast<const f2*>(lp + (r + 1) * W);
            cL = (f2){left_of(v.y, first), v.x};
            cC = v;
            cR = (f2){v.y, right_of(v.x, last)};
          }
          f2 acc = dw_taps2(w03.x, w03.y, w03.z, w03.w, w47.x, w47.y, w47.z, w47.w, cur.w8, aL, aC, aR, bL, bC, bR, cL, cC, cR);
          acc = dw_finish2<EPI>(acc, has_bias, cur.bch, has_bn, cur.bsc, cur.bsh, act);
          m = fmaxf(m, fmaxf(fabsf(acc.x), fabsf(acc.y)));
          *reinterpret_cast<f2*>(lp + r * W) = acc;          // row r of the tile was read in the previous step
          aL = bL; aC = bC; aR = bR;
          bL = cL; bC = cC; bR = cR;
        }
      } else {
        auto window = [&](float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2) -> float {
          float acc = dw_taps(w03.x, w03.y, w03.z, w03.w, w47.x, w47.y, w47.z, w47.w, cur.w8, a0, a1, a2, b0, b1, b2, c0, c1, c2);
          acc = dw_finish<EPI>(acc, has_bias, cur.bch, has_bn, cur.bsc, cur.bsh, act);
          m = fmaxf(m, fabsf(acc));
          return acc;
        };
        if (!DOWN) {
          float* lp = my_tile + j * IN + pos;
          float a0 = 0.f, a1 = 0.f, a2 = 0.f;
          float b1 = lp[0];
          float b0 = left_of(b1, first), b2 = right_of(b1, last);
#pragma unroll
          for (int r = 0; r < H; ++r) {
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            if (r + 1 < H) {
              c1 = lp[(r + 1) * W];
              c0 = left_of(c1, first);
              c2 = right_of(c1, last);
            }
            lp[r * W] = window(a0, a1, a2, b0, b1, b2, c0, c1, c2);
            a0 = b0; a1 = b1; a2 = b2;
            b0 = c0; b1 = c1; b2 = c2;
          }
        } else {
          // output row r: input rows 2r-1 (a), 2r (b), 2r+1 (c); per row: left = the left lane's odd column, centre / right own
          const float* lp = my_tile + j * IN + pos * 2;
          float* op = my_out + j * OUT + pos;
          float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
          for (int r = 0; r < HO; ++r) {
            const f2 vb = *reinterpret_cast<const f2*>(lp + (2 * r) * W);
            const float b0 = left_of(vb.y, first);
            float c0 = 0.f, c1 = 0.f, c2 = 0.f;
            if (2 * r + 1 < H) {
              const f2 vc = *reinterpret_cast<const f2*>(lp + (2 * r + 1) * W);
              c1 = vc.x;
              c2 = vc.y;
              c0 = left_of(vc.y, first);
            }
            op[r * WO] = window(a0, a1, a2, b0, vb.x, vb.y, c0, c1, c2);
            a0 = c0; a1 = c1; a2 = c2;
          }
        }
      }
    }
    FQ_DWF_PHASE();
    // ---- C: flat stores ---------------------------------------------------------------------------------------------------
    {
      f4 ov[NLO];
#pragma unroll
      for (int i = 0; i < NLO; ++i) ov[i] = DOWN ? otile[wave][lane + 64 * i] : tile[wave][lane + 64 * i];
#pragma unroll
      for (int i = 0; i < NLO; ++i)
        buf_st_v4f_unguarded(ry, (lane + 64u * i) < lim_out ? lane * 16u : kOob, base * (OUT * 4u) + 1024u * i, ov[i]);
      hold_store_data(ov);              // fq_common.h: nothing may write a store's data registers right behind it
    }
    if (has_stat) {
      const unsigned sample = fast_div(base + (is_out ? j : 0u), g.by_c);
      dw_stat_update(k_stat, s_base, sample, is_out, m, (int)lane, stat_out);
    }
    __builtin_amdgcn_wave_barrier();                      // (the next block's phase A overwrites the tile)
  }
  PW_STAMP(3);
  if (has_stat) dw_stat_flush(k_stat, s_base, n_samples, stat_out);
  PW_STAMP(5);
}

// The STATISTIC PASS of the form (stride 1, quantised input, even W), as the four-columns form has one (fq_dw_cols.hip: NOSTORE):
// every output is computed and joins the maximum, none is stored - phase B leaves the tile alone and there is no phase C.  `y` is
// no output: when not null it is the int8 buffer [n][c][h * w] that receives the low byte of the CODE of every input element (two's
// complement for signed codes).  Phase A holds the four codes of each 16-byte group it loads and the buffer is in the same flat
// order: one coalesced dword per lane and group.  A kernel of its own, phases A and B of dwconv3x3_flat_kernel's PAIR shape word
// for word: as a mode of that kernel - a template argument, or a shared body - it renames or re-schedules every existing
// instantiation (tools/kdiff.py).
template <bool ONLINE, int H, int W, int EPI>
__global__ __launch_bounds__(kBlock) void dwconv3x3_flat_stat_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwFlatGeom g, const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr,
    float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out, const float* __restrict__ bn_scale,
    const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  static_assert(W % 2 == 0 && (H * W) % 4 == 0, "two columns per lane, planes of whole 16-byte groups");
  constexpr int IN = H * W;                          // floats per plane
  constexpr int LPP = W / 2;                         // lanes per plane in phase B
  constexpr int P = 64 / LPP;                        // planes per wavefront and block
  constexpr int NFI = P * IN / 4;                    // 16-byte groups per wavefront and block
  constexpr int NLI = (NFI + 63) / 64;
  constexpr unsigned kOob = 0x80000000u;   // beyond every resource of this kernel (host: tensors < 2 GiB)
  __shared__ f4 tile[kBlock / 64][NLI * 64];
  __shared__ unsigned k_stat[kDwStatSlots];
  if (threadIdx.x < kDwStatSlots) k_stat[threadIdx.x] = 0u;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned b = blockIdx.x;
  const unsigned blk_begin = b * g.per + (b < g.rem ? b : g.rem);
  const unsigned blk_end = blk_begin + g.per + (b < g.rem ? 1u : 0u);
  const unsigned planes = g.planes;
  const unsigned n_samples = (unsigned)n;
  unsigned s_base;
  {
    const unsigned p0 = blk_begin * (P * (kBlock / 64));
    s_base = fast_div(p0 < planes ? p0 : planes - 1, g.by_c);
  }
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr, has_bias = bias != nullptr;
  const fq_rsrc rx = make_rsrc(x, (int64_t)planes * IN * 4), rc = make_rsrc(y, y != nullptr ? (int64_t)planes * IN : 0);
  const fq_rsrc rw = make_rsrc(wgt, (int64_t)g.C * 36);
  const unsigned j = lane / LPP, pos = lane - j * LPP;
  const bool b_lane = lane < P * LPP;
  const bool first = pos == 0, last = pos == LPP - 1;
  float* const my_tile = reinterpret_cast<float*>(tile[wave]);

  struct Blk {
    f4 raw[NLI];
    f4 w03, w47;
    float w8, bch, bsc, bsh;
  };
  auto issue = [&](unsigned blk, Blk& k) __attribute__((always_inline)) {
    const unsigned base = (blk * (kBlock / 64) + wave) * P;                  // first plane of this wavefront (uniform)
    const unsigned left = base < planes ? planes - base : 0u;
    const unsigned np = left < (unsigned)P ? left : (unsigned)P;
    const unsigned lim = np * (IN / 4);                                      // 16-byte groups that exist
#pragma unroll
    for (int i = 0; i < NLI; ++i)
      k.raw[i] = buf_ld_v4f_nt(rx, (lane + 64u * i) < lim ? lane * 16u : kOob, base * (IN * 4u) + 1024u * i);
    const unsigned ch = (b_lane && j < left) ? fast_mod(base + j, g.by_c) : 0u;
    k.w03 = buf_ld_v4f(rw, ch * 36u, 0);
    k.w47 = buf_ld_v4f(rw, ch * 36u, 16);
    k.w8 = buf_ld_f32(rw, ch * 36u, 32);
    k.bch = has_bias ? bias[ch] : 0.0f;
    k.bsc = has_bn ? bn_scale[ch] : 1.0f;
    k.bsh = has_bn ? bn_shift[ch] : 0.0f;
  };

  Blk nxt;
  const ThresholdReq treq = threshold_request(in_stat, n, ONLINE ? nullptr : in_thr, blockIdx.x == 0);   // first in the memory queue
  FQ_PIN();
  if (blk_begin < blk_end) issue(blk_begin, nxt);
  FQ_PIN();
  const QParams q = dw_qparams_finish<ONLINE>(treq, in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
  __syncthreads();                                        // statistic table zeroed
  for (unsigned blk = blk_begin; blk < blk_end; ++blk) {
    Blk cur = nxt;
    FQ_PIN();
    if (blk + 1 < blk_end) issue(blk + 1, nxt);
    FQ_PIN();
    const unsigned base = (blk * (kBlock / 64) + wave) * P;
    const unsigned left = base < planes ? planes - base : 0u;
    const unsigned np = left < (unsigned)P ? left : (unsigned)P;
    const unsigned lim = np * (IN / 4);
    // ---- A: quantise in flat order, keep the codes, stage --------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < NLI; ++i) {
      const f4 k = fq_code4(cur.raw[i], q);
      const unsigned wd = ((unsigned)(int)k.x & 255u) | (((unsigned)(int)k.y & 255u) << 8) | (((unsigned)(int)k.z & 255u) << 16) |
                          (((unsigned)(int)k.w & 255u) << 24);
      buf_st_f32(rc, (lane + 64u * i) < lim ? lane * 4u : kOob, base * (unsigned)IN + 256u * i, __uint_as_float(wd));
      tile[wave][lane + 64 * i] = k * q.scale;
    }
    FQ_DWF_PHASE();
    // ---- B: 3x3 on the tile, the maximum only ---------------------------------------------------------------------------------
    float m = 0.0f;
    const bool is_out = b_lane && j < left;
    if (b_lane) {
      const f4 w03 = cur.w03, w47 = cur.w47;
      const float* lp = my_tile + j * IN + pos * 2;
      f2 aL = {0.f, 0.f}, aC = {0.f, 0.f}, aR = {0.f, 0.f};     // row r-1: (L, q0), (q0, q1), (q1, R)
      f2 bL, bC, bR;
      {
        const f2 v = *reinterpret_cast<const f2*>(lp);
        bL = (f2){left_of(v.y, first), v.x};
        bC = v;
        bR = (f2){v.y, right_of(v.x, last)};
      }
#pragma unroll
      for (int r = 0; r < H; ++r) {
        f2 cL = {0.f, 0.f}, cC = {0.f, 0.f}, cR = {0.f, 0.f};
        if (r + 1 < H) {
          const f2 v = *reinterpret_cast<const f2*>(lp + (r + 1) * W);
          cL = (f2){left_of(v.y, first), v.x};
          cC = v;
          cR = (f2){v.y, right_of(v.x, last)};
        }
        f2 acc = dw_taps2(w03.x, w03.y, w03.z, w03.w, w47.x, w47.y, w47.z, w47.w, cur.w8, aL, aC, aR, bL, bC, bR, cL, cC, cR);
        acc = dw_finish2<EPI>(acc, has_bias, cur.bch, has_bn, cur.bsc, cur.bsh, act);
        m = fmaxf(m, fmaxf(fabsf(acc.x), fabsf(acc.y)));
        aL = bL; aC = bC; aR = bR;
        bL = cL; bC = cC; bR = cR;
      }
    }
    if (has_stat) {
      const unsigned sample = fast_div(base + (is_out ? j : 0u), g.by_c);
      dw_stat_update(k_stat, s_base, sample, is_out, m, (int)lane, stat_out);
    }
    FQ_DWF_PHASE();                                       // (the next block's phase A overwrites the tile)
  }
  if (has_stat) dw_stat_flush(k_stat, s_base, n_samples, stat_out);
}

// ---- K2p, flat: 14x14 (stride 1 and 2), 7x7 and 28x28 (stride 1 and 2) planes ------------------------------------------------
// tuning: bit 0 14x14 s1, bit 1 14x14 s2, bit 2 7x7, bit 3 28x28 s1, bit 4 28x28 s2
// (28x28: 40.1 -> 34.6 us stride 1.  Stride 2 on 28x28 was dropped in round 2 because 0.05 % of its outputs changed from run
// to run at full size; round 3 found the cause - NOT a data race: a VALU write of a 16-byte buffer store's data register
// right behind the store, a hazard hipcc does not guard when soffset is a register (fq_common.h at buf_st_v4f,
// profiles/r3_dw_flat_race.txt, tools/isa_lint.py) - every instantiation of this kernel had the
// pattern one instruction further away.  With the stores guarded the form is exact at every occupancy.  Through round 4 it
// was built and tested but not chosen by shape - one batch at a time it was no faster than the four-columns-per-lane form
// (28.3 us against ~25; whole step 1.1967 against 1.1919 ms, profiles/r3_dw_flat_race.txt); with three batches in flight and
// its nontemporal loads it is: default workload +1.77 % images/s (sd 0.03, profiles/r5_heuristics_ab.txt).)
int dw_flat_kind(const DwCall& d) {           // the bit of FQ_DW_FLAT, -1: not a plane size of this form
  return (d.h == 14 && d.wdt == 14) ? (d.stride == 1 ? 0 : 1)
         : (d.h == 7 && d.wdt == 7 && d.stride == 1) ? 2
         : (d.h == 28 && d.wdt == 28) ? (d.stride == 1 ? 3 : 4) : -1;
}
int dw_flat_planes(int kind) { return kind == 0 ? 9 : kind >= 3 ? 4 : 8; }      // per wavefront and block (dwconv3x3_flat_kernel: P)

}  // namespace

namespace fqi {
bool dw_flat_applies(const DwCall& d, int form) {
  static const int flat_on = env_int("FQ_DW_FLAT", 31) & 31;
  const int kind = dw_flat_kind(d);
  const bool whole = kind == 0 || kind >= 3 || (d.n * d.c) % dw_flat_planes(kind) == 0;     // planes of 49 floats: no 16-byte tail
  return kind >= 0 && (form == 5 || (form == 0 && ((flat_on >> kind) & 1))) && whole && aligned16(d.x) && aligned16(d.y) &&
         d.n * d.c * d.h * d.wdt * 4 < (1ll << 31);
}
// the statistic pass (y == NULL) of a 28 x 28 plane: this form instead of the four-columns one, whose every memory instruction
// touches many short rows there (fq_dwconv.hip asks before it falls back to that form)
bool dw_flat_stat_applies(const DwCall& d) {
  static const int flat_on = env_int("FQ_DW_FLAT", 31) & 31;
  return d.y == nullptr && d.quant && d.lo_neg != kRangeMode && dw_flat_kind(d) == 3 && ((flat_on >> 3) & 1) && aligned16(d.x) &&
         aligned16(d.x_codes_out) && d.n * d.c * d.h * d.wdt * 4 < (1ll << 31);
}
int dw_run_flat(const DwCall& d) {
  const int kind = dw_flat_kind(d);
  DwFlatGeom fg;
  fg.C = (int)d.c;
  fg.planes = (unsigned)(d.n * d.c);
  fg.by_c = fast_div_for((unsigned)d.c);
  const int64_t nblk = dw_blocks(d.n * d.c, dw_flat_planes(kind));
  static const int fl_tune = env_int("FQ_DW_FLAT_WG_PER_CU", 0);
  // three workgroups per CU, each with one block in work and one requested: measured best for all three shapes
  // (512 x 14x14: 2 / 3 / 4 / 6 per CU = 22.2 / 19.6 / 20.7 / 21.9 us; 1024 x 7x7: 16.1 / 14.6 / 17.3 (8) / 16.4 us)
  const int grid = dw_grid(nblk, fl_tune > 0 ? fl_tune : 3);
  fg.per = (unsigned)(nblk / grid);
  fg.rem = (unsigned)(nblk % grid);
  if (d.y == nullptr)
    return dw_launch(d, grid, 0, [](auto, auto o, auto e) { return dwconv3x3_flat_stat_kernel<o(), 28, 28, e()>; }, fg);
  auto go = [&](auto s, auto hw) {
    return dw_launch(d, grid, 0, [](auto q, auto o, auto e) {
      return dwconv3x3_flat_kernel<decltype(s)::value, q(), o(), decltype(hw)::value, decltype(hw)::value, e()>;
    }, fg);
  };
  return kind == 0 ? go(dw_int<1>{}, dw_int<14>{}) : kind == 1 ? go(dw_int<2>{}, dw_int<14>{})
         : kind == 2 ? go(dw_int<1>{}, dw_int<7>{}) : kind == 4 ? go(dw_int<2>{}, dw_int<28>{})
                     : go(dw_int<1>{}, dw_int<28>{});
}
}  // namespace fqi
