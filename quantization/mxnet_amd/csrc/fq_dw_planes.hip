// libfakequant — K2o depthwise 3x3 with quantise-on-load: whole small planes in registers, pipelined across blocks
#include "fq_dw.h"      // what the depthwise forms share; fq_common.h: the list of units, the design rules

namespace {
// K2o: small planes (H rows known at compile time, a plane row fits one wavefront): a wavefront holds EVERY input row of
// its planes in registers and requests the rows, weights and constants of its NEXT block before it works on the current
// one (K2d restarts its prefetch ring in every block: two exposed memory latencies + the weight gather per 14 row steps).
// These layers are bound by instruction issue, not by memory (ablation without loads and stores: 21 of 25 us on
// 512x14x14, profiles/r2_dw_planes.txt), so the form is built around the instruction count per output:
//   * CPL = 2 columns per lane where W is even: 8-byte loads and stores, and the 3x3 sums of the two outputs run as ONE
//     chain of packed fp32 FMAs (v_pk_fma_f32: two IEEE FMAs per lane per instruction, same order as the scalar chain);
//   * no halo lanes: a plane takes W / CPL lanes, its edge lanes replace the neighbour's value by 0 (one select);
//   * horizontal neighbours by DPP wave shifts (lane_prev / lane_next), epilogue fixed at compile time (EPI).
// Buffer addressing: idle lanes and the tail read 0 and store nothing through an out-of-range offset, row strides sit in
// scalar registers.
template <int S, int H, int CPL>
struct DwPlanesBlk {
  static constexpr int kIn = (S == 2 || CPL == 2) ? 2 : 1;     // input columns per lane
  float raw[kIn * H];      // row-major: (column 0[, column 1]) of rows 0..H-1
  float w[9];
  float bch, bsc, bsh;
};

template <int S, bool QUANT, bool ONLINE, int H, int CPL, int EPI>
__global__ __launch_bounds__(kBlock) void dwconv3x3_planes_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwColGeom g, int64_t total_segs, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  static_assert(S == 1 || CPL == 2, "stride 2 reads two input columns per lane");
  typedef DwPlanesBlk<S, H, CPL> Blk;
  constexpr int KIN = Blk::kIn;
  constexpr int HO = (H - 1) / S + 1;
  constexpr unsigned kOob = 0x80000000u;                 // beyond every resource of this kernel (host: tensors < 2 GiB)
  __shared__ unsigned k_stat[kDwStatSlots];
  if (threadIdx.x < kDwStatSlots) k_stat[threadIdx.x] = 0u;
  PW_STAMP(0);
  const int lane = threadIdx.x & 63;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int seg_in_wave = lane / g.SEG;                   // g.SEG lanes per plane: W / CPL (stride 1), Wo (stride 2)
  const int pos = lane - seg_in_wave * g.SEG;
  const bool lane_used = seg_in_wave < g.segs;
  const bool first = pos == 0, last = pos == g.SEG - 1;   // edge lanes of a plane: no left / right neighbour
  const unsigned segs_per_block = (unsigned)g.segs * (kBlock / 64);
  const unsigned tsegs = (unsigned)total_segs, C_u = (unsigned)g.C;           // one segment per plane: tsegs planes
  const DwBlkRange rg = dw_block_range((tsegs + segs_per_block - 1) / segs_per_block, tsegs, segs_per_block, 1u, C_u);
  const unsigned blk_begin = rg.begin, blk_end = rg.end;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr, has_bias = bias != nullptr;
  const unsigned plane_in = (unsigned)(H * g.W), plane_out = (unsigned)(HO * g.Wo);
  const unsigned row_in = (unsigned)g.W * 4u, row_out = (unsigned)g.Wo * 4u;
  const fq_rsrc rx = make_rsrc(x, (int64_t)tsegs * plane_in * 4), ry = make_rsrc(y, (int64_t)tsegs * plane_out * 4);
  const fq_rsrc rw = make_rsrc(wgt, (int64_t)g.C * 36);
  const unsigned ic0 = (unsigned)pos * KIN;               // first input column of this lane
  const unsigned oc0 = S == 1 ? ic0 : (unsigned)pos;      // first output column of this lane

  auto issue = [&](unsigned blk, Blk& b) __attribute__((always_inline)) {
    const unsigned seg = blk * segs_per_block + wave * (unsigned)g.segs + (unsigned)seg_in_wave;
    const bool seg_ok = lane_used && seg < tsegs;
    const unsigned xoff = seg_ok ? (seg * plane_in + ic0) * 4u : kOob;
#pragma unroll
    for (int r = 0; r < H; ++r) {
      if (KIN == 1) {
        b.raw[r] = buf_ld_f32(rx, xoff, (unsigned)r * row_in);
      } else {
        const f2 v = buf_ld_2f32(rx, xoff, (unsigned)r * row_in);
        b.raw[2 * r] = v.x;
        b.raw[2 * r + 1] = v.y;
      }
    }
    const unsigned ch = seg_ok ? seg % C_u : 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) b.w[k] = buf_ld_f32(rw, ch * 36u, (unsigned)k * 4u);
    b.bch = has_bias ? bias[ch] : 0.0f;
    b.bsc = has_bn ? bn_scale[ch] : 1.0f;
    b.bsh = has_bn ? bn_shift[ch] : 0.0f;
  };

  Blk nxt;
  ThresholdReq treq;
  if (QUANT) treq = threshold_request(in_stat, n, ONLINE ? nullptr : in_thr, blockIdx.x == 0);   // first in the memory queue
  FQ_PIN();
  if (blk_begin < blk_end) issue(blk_begin, nxt);
  FQ_PIN();
  QParams q = {};
  if (QUANT)                                              // while the first block is on its way
    q = dw_qparams_finish<ONLINE>(treq, in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
  PW_STAMP(1);
  __syncthreads();                                        // statistic table zeroed
  for (unsigned blk = blk_begin; blk < blk_end; ++blk) {
    if (blk == blk_begin + 1) PW_STAMP(2);
#ifdef FQ_PW_TRACE
    if (blk == blk_begin) {                               // trace build: separate "first block's data arrives" from "first pass through the code"
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      PW_STAMP(4);
    }
#endif
    Blk cur = nxt;
    FQ_PIN();
    if (blk + 1 < blk_end) issue(blk + 1, nxt);
    FQ_PIN();
    const unsigned seg = blk * segs_per_block + wave * (unsigned)g.segs + (unsigned)seg_in_wave;
    const bool is_out = lane_used && seg < tsegs;
    const unsigned yoff = is_out ? (seg * plane_out + oc0) * 4u : kOob;
    const unsigned sample = (seg < tsegs ? seg : tsegs - 1) / C_u;
    float m = 0.0f;
    auto fq = [&](float v) -> float { return QUANT ? fq_code(v, q) * q.scale : v; };
    const float* w = cur.w;
    if (S == 1 && CPL == 2) {
      // two outputs per lane: (L, q0, q1) and (q0, q1, R) per input row, summed as one packed chain
      f2 aL = {0.f, 0.f}, aC = {0.f, 0.f}, aR = {0.f, 0.f};     // row r-1: (L, q0), (q0, q1), (q1, R)
      f2 bL, bC, bR;
      {
        const float q0 = fq(cur.raw[0]), q1 = fq(cur.raw[1]);
        bL = (f2){left_of(q1, first), q0};
        bC = (f2){q0, q1};
        bR = (f2){q1, right_of(q0, last)};
      }
#pragma unroll
      for (int r = 0; r < H; ++r) {
        f2 cL = {0.f, 0.f}, cC = {0.f, 0.f}, cR = {0.f, 0.f};
        if (r + 1 < H) {
          const float q0 = fq(cur.raw[2 * r + 2]), q1 = fq(cur.raw[2 * r + 3]);
          cL = (f2){left_of(q1, first), q0};
          cC = (f2){q0, q1};
          cR = (f2){q1, right_of(q0, last)};
        }
        f2 acc = dw_taps2(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], aL, aC, aR, bL, bC, bR, cL, cC, cR);
        acc = dw_finish2<EPI>(acc, has_bias, cur.bch, has_bn, cur.bsc, cur.bsh, act);
        m = fmaxf(m, fmaxf(fabsf(acc.x), fabsf(acc.y)));
        buf_st_2f32(ry, yoff, (unsigned)r * row_out, acc);
        aL = bL; aC = bC; aR = bR;
        bL = cL; bC = cC; bR = cR;
      }
    } else {
      auto finish = [&](int r, float acc) __attribute__((always_inline)) {
        acc = dw_finish<EPI>(acc, has_bias, cur.bch, has_bn, cur.bsc, cur.bsh, act);
        m = fmaxf(m, fabsf(acc));
        buf_st_f32(ry, yoff, (unsigned)r * row_out, acc);
      };
      auto window = [&](float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2) -> float {
        return dw_taps(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], a0, a1, a2, b0, b1, b2, c0, c1, c2);
      };
      if (S == 1) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        float b1 = fq(cur.raw[0]);
        float b0 = left_of(b1, first), b2 = right_of(b1, last);
#pragma unroll
        for (int r = 0; r < H; ++r) {
          float c0 = 0.f, c1 = 0.f, c2 = 0.f;
          if (r + 1 < H) {
            c1 = fq(cur.raw[r + 1]);
            c0 = left_of(c1, first);
            c2 = right_of(c1, last);
          }
          finish(r, window(a0, a1, a2, b0, b1, b2, c0, c1, c2));
          a0 = b0; a1 = b1; a2 = b2;
          b0 = c0; b1 = c1; b2 = c2;
        }
      } else {
        // output row r: input rows 2r-1 (a), 2r (b), 2r+1 (c); per row: left = the left lane's odd column, centre / right own
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int r = 0; r < HO; ++r) {
          const float b1 = fq(cur.raw[4 * r]), b2 = fq(cur.raw[4 * r + 1]);
          const float b0 = left_of(b2, first);
          float c0 = 0.f, c1 = 0.f, c2 = 0.f;
          if (2 * r + 1 < H) {
            c1 = fq(cur.raw[4 * r + 2]);
            c2 = fq(cur.raw[4 * r + 3]);
            c0 = left_of(c2, first);
          }
          finish(r, window(a0, a1, a2, b0, b1, b2, c0, c1, c2));
          a0 = c0; a1 = c1; a2 = c2;
        }
      }
    }
    if (has_stat) dw_stat_update(k_stat, rg.s_base, sample, is_out, m, lane, stat_out);
  }
  PW_STAMP(3);
  if (has_stat) dw_stat_flush(k_stat, rg.s_base, rg.n_samples, stat_out);
  PW_STAMP(5);
}

// ---- K2o, planes: small planes whole in registers, pipelined across blocks ------------------------------------------------
bool dw_planes_two_cols(const DwCall& d) {
  static const int planes_cpl = env_int("FQ_DW_PLANES_CPL", 2);          // 1: one column per lane even where W is even (A/B)
  const bool al8 = ((((uintptr_t)d.x) | ((uintptr_t)d.y)) & 7) == 0;
  return d.wdt % 2 == 0 && al8 && (d.stride == 2 || planes_cpl == 2);
}

}  // namespace

namespace fqi {
bool dw_planes_applies(const DwCall& d, int form) {
  static const int planes_on = env_int("FQ_DW_PLANES", 1);
  const bool can_planes = (d.h == 14 || d.h == 7) && d.wdt <= 64 && (d.stride == 1 || (dw_planes_two_cols(d) && d.h == 14)) &&
                          d.n * d.c * d.h * d.wdt * 4 < (1ll << 31);
  return (form == 4 || (form == 0 && planes_on)) && can_planes;
}
int dw_run_planes(const DwCall& d) {
  const bool two_cols = dw_planes_two_cols(d);
  // lanes per plane (no halo lanes): one segment per plane
  DwColGeom cg = dw_col_geom(d, (int)(d.stride == 2 ? d.wo : (two_cols ? d.wdt / 2 : d.wdt)), 0);
  cg.sw = cg.Wo;                                          // (output columns, as the other forms have it: two per lane with two_cols)
  const int64_t total_segs = d.n * d.c;
  static const int pl_wg_per_cu = env_int("FQ_DW_PLANES_WG_PER_CU", 5);
  const int grid = dw_grid(dw_blocks(total_segs, cg.segs), pl_wg_per_cu);
  auto go = [&](auto s, auto h, auto cpl) {
    return dw_launch(d, grid, 0, [](auto q, auto o, auto e) {
      return dwconv3x3_planes_kernel<decltype(s)::value, q(), o(), decltype(h)::value, decltype(cpl)::value, e()>;
    }, cg, total_segs);
  };
  if (d.stride == 2) return go(dw_int<2>{}, dw_int<14>{}, dw_int<2>{});
  if (d.h == 14) return two_cols ? go(dw_int<1>{}, dw_int<14>{}, dw_int<2>{}) : go(dw_int<1>{}, dw_int<14>{}, dw_int<1>{});
  return two_cols ? go(dw_int<1>{}, dw_int<7>{}, dw_int<2>{}) : go(dw_int<1>{}, dw_int<7>{}, dw_int<1>{});
}
}  // namespace fqi
