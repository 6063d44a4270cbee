// libfakequant — K2d / K2e depthwise 3x3 with quantise-on-load, the sliding window in registers: one column / four columns per lane
#include "fq_dw.h"      // what the depthwise forms share; fq_common.h: the list of units, the design rules

namespace {
// K2d: depthwise 3x3, register sliding-window form (no LDS, no barriers).  A wavefront holds `segs` independent
// SEGMENTS; a segment is `sw` adjacent output columns of one plane plus halo lanes (stride 1: one on each side, stride
// 2: one on the left).  Every lane streams ITS input column(s) top to bottom — one coalesced 4-byte load per lane per
// input row, quantised once — and gets its horizontal neighbours from the adjacent lanes with wavefront shuffles; the
// three live input rows stay in registers, loads run D rows ahead of their use.
template <int S, bool QUANT, bool ONLINE, int EPI>
__global__ __launch_bounds__(kBlock) void dwconv3x3_cols_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwColGeom g, int64_t total_segs, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  // output rows of input kept in flight (S=2: 4 loads per row).  (16 / 8 - every row of a 14x14 plane in flight at
  // once - measured SLOWER on the same box: 38 vs 36 us per 512x14x14 layer.)
  constexpr int D = (S == 1) ? 8 : 4;
  __shared__ unsigned k_stat[kDwStatSlots];
  if (threadIdx.x < kDwStatSlots) k_stat[threadIdx.x] = 0u;
  PW_STAMP(0);
  // The quantisation parameters are derived AFTER the first block's loads have been issued (ensure_q below): the batch
  // statistic is a dependent chain of two cold loads + an fp64 tree (~2.8 us per workgroup, tools/dw_trace.py) that
  // otherwise sits in front of the first useful load of every workgroup.
  QParams q = {};
  bool q_ready = !QUANT;
  auto ensure_q = [&]() __attribute__((always_inline)) {
    if (QUANT && !q_ready) {
      q = dw_qparams<ONLINE>(in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
      q_ready = true;
    }
  };
  PW_STAMP(1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg_in_wave = lane / g.SEG;
  const int pos = lane - seg_in_wave * g.SEG;
  const bool lane_used = seg_in_wave < g.segs;
  const int64_t segs_per_block = (int64_t)g.segs * (kBlock / 64);
  const int64_t nblk = (total_segs + segs_per_block - 1) / segs_per_block;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  const int plane_in = g.H * g.W, plane_out = g.Ho * g.Wo;

  // (Row strips per plane were tried for load balance and measured slower: every strip restarts the prefetch ring.)
  const unsigned tsegs = (unsigned)total_segs, nsegx = (unsigned)g.nsegx, C_u = (unsigned)g.C;
  const DwBlkRange rg = dw_block_range((unsigned)nblk, tsegs, (unsigned)segs_per_block, nsegx, C_u);
  __syncthreads();                                       // statistic table zeroed
  for (unsigned blk = rg.begin; blk < rg.end; ++blk) {
    const unsigned seg = blk * (unsigned)segs_per_block + (unsigned)wave * (unsigned)g.segs + (unsigned)seg_in_wave;
    const bool seg_ok = lane_used && seg < tsegs;
    const unsigned plane = seg_ok ? seg / nsegx : 0u;
    const int sx = seg_ok ? (int)(seg - plane * nsegx) : 0;
    const unsigned sample_u = plane / C_u;
    const int ch = (int)(plane - sample_u * C_u);
    const int sample = (int)sample_u;
    // column bookkeeping
    int oc, ic0;                                          // output column; first input column this lane loads
    bool is_out;
    if (S == 1) {
      ic0 = sx * g.sw + pos - 1;                          // pos 0 / sw+1 are the halo lanes
      oc = ic0;
      is_out = seg_ok && pos >= 1 && pos <= g.sw && oc < g.Wo;
    } else {
      oc = sx * g.sw + pos - 1;                           // pos 0 is the left-halo lane
      ic0 = 2 * oc;                                       // this lane loads input columns 2*oc and 2*oc + 1
      is_out = seg_ok && pos >= 1 && oc < g.Wo;
    }
    const bool ld0 = seg_ok && (S == 1 ? (ic0 >= 0 && ic0 < g.W) : (pos >= 1 && ic0 < g.W));
    const bool ld1 = seg_ok && S == 2 && (ic0 + 1 >= 0) && (ic0 + 1 < g.W);     // stride 2: second column (halo lane: col 2*sx*sw - 1)
    const float* xp = x + plane * (int64_t)plane_in + ic0;
    float* yp = y + plane * (int64_t)plane_out + oc;
    const float* wk = wgt + ch * 9;
    const float w00 = wk[0], w01 = wk[1], w02 = wk[2], w10 = wk[3], w11 = wk[4], w12 = wk[5], w20 = wk[6],
                w21 = wk[7], w22 = wk[8];
    const float bch = bias != nullptr ? bias[ch] : 0.0f;
    const float bsc = has_bn ? bn_scale[ch] : 1.0f, bsh = has_bn ? bn_shift[ch] : 0.0f;
    float m = 0.0f;
    if (blk == rg.begin) PW_STAMP(2);

    const int last_row = g.H - 1;                          // (loads: unconditional from a clamped row, masked by keep)
    if (S == 1) {
      // rows: a = input row r-1, b = row r, c = row r+1 (each as left / centre / right)
      const float* xs = ld0 ? xp : x;                      // lanes with nothing to load read element 0
      auto ldrow = [&](int row) -> float {
        const int rc = row < last_row ? row : last_row;
        return keep(xs[(int64_t)rc * g.W], ld0 && row <= last_row);
      };
      auto emit = [&](int r, float c1, float& a0, float& a1, float& a2, float& b0, float& b1, float& b2) {
        if (QUANT) c1 = fq_code(c1, q) * q.scale;
        const float c0 = lane_prev(c1), c2 = lane_next(c1);
        float acc = dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a0, a1, a2, b0, b1, b2, c0, c1, c2);
        acc = dw_finish<EPI>(acc, bias != nullptr, bch, has_bn, bsc, bsh, act);
        m = fmaxf(m, keep(fabsf(acc), is_out));
        if (is_out) yp[(int64_t)r * g.Wo] = acc;
        a0 = b0; a1 = b1; a2 = b2;
        b0 = c0; b1 = c1; b2 = c2;
      };
      float raw[D];
#pragma unroll
      for (int k = 0; k < D; ++k) raw[k] = ldrow(1 + k);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      float b1 = ldrow(0);
      FQ_PIN();
      ensure_q();
      if (QUANT) b1 = fq_code(b1, q) * q.scale;
      float b0 = lane_prev(b1), b2 = lane_next(b1);
      const int rend = g.Ho;                              // same trip count for every lane of the grid
      int r0 = 0;
      for (; r0 + D <= rend; r0 += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float c1 = raw[k];
          raw[k] = ldrow(r0 + k + 1 + D);
          emit(r0 + k, c1, a0, a1, a2, b0, b1, b2);
        }
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (r0 + k < rend) emit(r0 + k, raw[k], a0, a1, a2, b0, b1, b2);
    } else {
      // stride 2: output row r uses input rows 2r-1 (a), 2r (b), 2r+1 (c); per input row: left = neighbour's 2nd
      // column, centre = own 1st column, right = own 2nd column
      const float* xs0 = ld0 ? xp : x;
      const float* xs1 = ld1 ? xp + 1 : x;
      auto ld_a = [&](int row) -> float {
        const int rc = row < last_row ? row : last_row;
        return keep(xs0[(int64_t)rc * g.W], ld0 && row <= last_row);
      };
      auto ld_b = [&](int row) -> float {
        const int rc = row < last_row ? row : last_row;
        return keep(xs1[(int64_t)rc * g.W], ld1 && row <= last_row);
      };
      auto emit2 = [&](int r, float b1, float b2, float c1, float c2, float& a0, float& a1, float& a2) {
        if (QUANT) {
          b1 = fq_code(b1, q) * q.scale;
          b2 = fq_code(b2, q) * q.scale;
          c1 = fq_code(c1, q) * q.scale;
          c2 = fq_code(c2, q) * q.scale;
        }
        const float b0 = lane_prev(b2), c0 = lane_prev(c2);
        float acc = dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a0, a1, a2, b0, b1, b2, c0, c1, c2);
        acc = dw_finish<EPI>(acc, bias != nullptr, bch, has_bn, bsc, bsh, act);
        m = fmaxf(m, keep(fabsf(acc), is_out));
        if (is_out) yp[(int64_t)r * g.Wo] = acc;
        a0 = c0; a1 = c1; a2 = c2;
      };
      float rb0[D], rb1[D], rc0[D], rc1[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        rb0[k] = ld_a(2 * k);
        rb1[k] = ld_b(2 * k);
        rc0[k] = ld_a(2 * k + 1);
        rc1[k] = ld_b(2 * k + 1);
      }
      FQ_PIN();
      ensure_q();
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      const int rend = g.Ho;
      int r0 = 0;
      for (; r0 + D <= rend; r0 += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float b1 = rb0[k], b2 = rb1[k], c1 = rc0[k], c2 = rc1[k];
          const int rn = r0 + k + D;
          rb0[k] = ld_a(2 * rn);
          rb1[k] = ld_b(2 * rn);
          rc0[k] = ld_a(2 * rn + 1);
          rc1[k] = ld_b(2 * rn + 1);
          emit2(r0 + k, b1, b2, c1, c2, a0, a1, a2);
        }
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (r0 + k < rend) emit2(r0 + k, rb0[k], rb1[k], rc0[k], rc1[k], a0, a1, a2);
    }
    if (blk == rg.begin) PW_STAMP(3);
    if (has_stat) dw_stat_update(k_stat, rg.s_base, sample, is_out, m, lane, stat_out);
  }
  if (has_stat) dw_stat_flush(k_stat, rg.s_base, rg.n_samples, stat_out);
  PW_STAMP(5);
}

// K2e: the same sliding window with FOUR input columns per lane (16-byte loads, 16-byte stores for stride 1 / 8-byte
// for stride 2) — needs W % 4 == 0.  With 4-byte accesses the kernel above cannot keep enough bytes in flight
// (PMC: 38 % of wave cycles parked on vmcnt at 4.1 TB/s); this form has 4x the bytes per outstanding load.
// Lane p of a segment: p = 0 left-halo lane, 1..L compute lanes (input columns 4(p-1)..4(p-1)+3), L+1 right-halo lane
// (stride 1 only).  Halo lanes load and quantise like the others; their neighbours pick up .w / .x by shuffle.
// NT: nontemporal LOADS - an input beyond the 256 MB Infinity Cache is dead after this pass and should not displace the
// output, which the consumer does find there (measured in the model: 64 @112x112 stride 2, 411 MB in / 103 MB out, 110 -> 99 us;
// with nontemporal stores too, or on the 205 MB inputs of the stride-1 layers, the step gets slower)
// NOSTORE (stride 1, quantised input): the layer's statistic pass - every output is computed as above and joins the maximum, none
// is stored.  `y` then is no output: when not null it is the int8 buffer [n][c][h * w] that receives the CODE of every input
// element as the quantise-on-load produced it (the low byte of the integer: two's complement for signed codes) - one dword per
// lane and input row, written by the compute lane that owns the four columns (the halo lanes' copies are not written).
template <int S, bool QUANT, bool ONLINE, bool NT, int EPI, bool NOSTORE = false>
__global__ __launch_bounds__(kBlock) void dwconv3x3_cols4_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwColGeom g, int64_t total_segs, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  // Input rows are fetched in BURSTS of D rows (double buffered): the D loads of a burst leave the wave back to back
  // and hit the same DRAM pages; one load per step (a ring) spreads them ~700 cycles apart, and with thousands of
  // waves each streaming its own plane every access then opens a new page.
  constexpr int D = (S == 1) ? 4 : 2;
  static_assert(!NOSTORE || (S == 1 && QUANT), "the statistic pass exists for stride 1 with a quantised input");
  __shared__ unsigned k_stat[kDwStatSlots];
  if (threadIdx.x < kDwStatSlots) k_stat[threadIdx.x] = 0u;
  // (deriving q after the first block's loads, as K2d does, was measured 3-5 % SLOWER here: the row bursts of these large
  // planes already hide the prologue, and the extra live state costs registers)
  QParams q = {};
  if (QUANT) q = dw_qparams<ONLINE>(in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg_in_wave = lane / g.SEG;
  const int pos = lane - seg_in_wave * g.SEG;
  const bool lane_used = seg_in_wave < g.segs;
  const int64_t segs_per_block = (int64_t)g.segs * (kBlock / 64);
  const int64_t nblk = (total_segs + segs_per_block - 1) / segs_per_block;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  const int plane_in = g.H * g.W, plane_out = g.Ho * g.Wo;
  const int last_row = g.H - 1;
  const unsigned tsegs = (unsigned)total_segs, nsegx = (unsigned)g.nsegx, C_u = (unsigned)g.C;
  const DwBlkRange rg = dw_block_range((unsigned)nblk, tsegs, (unsigned)segs_per_block, nsegx, C_u);
  __syncthreads();                                       // statistic table zeroed
  for (unsigned blk = rg.begin; blk < rg.end; ++blk) {
    const unsigned seg = blk * (unsigned)segs_per_block + (unsigned)wave * (unsigned)g.segs + (unsigned)seg_in_wave;
    const bool seg_ok = lane_used && seg < tsegs;
    const unsigned plane = seg_ok ? seg / nsegx : 0u;
    const int sx = seg_ok ? (int)(seg - plane * nsegx) : 0;
    const unsigned sample_u = plane / C_u;
    const int ch = (int)(plane - sample_u * C_u);
    const int sample = (int)sample_u;
    const int ic0 = (sx * g.sw + pos - 1) * 4;            // first of the 4 input columns this lane loads
    const bool ld_ok = seg_ok && ic0 >= 0 && ic0 < g.W;
    const int oc = S == 1 ? ic0 : ic0 / 2;                // first output column (4 outputs for S=1, 2 for S=2)
    const bool is_out = seg_ok && pos >= 1 && pos <= g.sw && oc < g.Wo;
    const f4* xs = reinterpret_cast<const f4*>(ld_ok ? x + plane * (int64_t)plane_in + ic0 : x);
    float* yp = y + plane * (int64_t)plane_out + oc;
    const int rowq = g.W / 4;                             // f4 per input row
    const float* wk = wgt + ch * 9;
    const float w00 = wk[0], w01 = wk[1], w02 = wk[2], w10 = wk[3], w11 = wk[4], w12 = wk[5], w20 = wk[6],
                w21 = wk[7], w22 = wk[8];
    const float bch = bias != nullptr ? bias[ch] : 0.0f;
    const float bsc = has_bn ? bn_scale[ch] : 1.0f, bsh = has_bn ? bn_shift[ch] : 0.0f;
    float m = 0.0f;
    auto ldrow = [&](int row) -> f4 {
      const int rc = row < last_row ? row : last_row;
      return keep4(ld4<NT>(xs + (int64_t)rc * rowq), ld_ok && row <= last_row);
    };
    auto quant4 = [&](f4 v) -> f4 { return QUANT ? fq_code4(v, q) * q.scale : v; };
    auto finish = [&](float acc) -> float { return dw_finish<EPI>(acc, bias != nullptr, bch, has_bn, bsc, bsh, act); };
    // statistic pass: input row `row` quantised, its codes kept (where there is such a row and a buffer)
    unsigned* const cp = reinterpret_cast<unsigned*>(y) + (plane * (int64_t)plane_in + (ld_ok ? ic0 : 0)) / 4;
    auto quant4_keep = [&](f4 v, int row) -> f4 {
      const f4 k = fq_code4(v, q);
      if (y != nullptr && is_out && row <= last_row) {
        const unsigned b0 = (unsigned)(int)k.x & 255u, b1 = (unsigned)(int)k.y & 255u, b2 = (unsigned)(int)k.z & 255u,
                       b3 = (unsigned)(int)k.w & 255u;
        cp[(int64_t)row * rowq] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      }
      return k * q.scale;
    };

    if (S == 1) {
      // a, b, c: rows r-1, r, r+1 as (left, v.x, v.y, v.z, v.w, right)
      float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[6];
      f4 raw[D];
#pragma unroll
      for (int k = 0; k < D; ++k) raw[k] = ldrow(1 + k);
      {
        const f4 v = NOSTORE ? quant4_keep(ldrow(0), 0) : quant4(ldrow(0));
        b[0] = lane_prev(v.w);
        b[1] = v.x; b[2] = v.y; b[3] = v.z; b[4] = v.w;
        b[5] = lane_next(v.x);
      }
      auto emit = [&](int r, f4 craw) {
        const f4 v = NOSTORE ? quant4_keep(craw, r + 1) : quant4(craw);
        float c[6];
        c[0] = lane_prev(v.w);
        c[1] = v.x; c[2] = v.y; c[3] = v.z; c[4] = v.w;
        c[5] = lane_next(v.x);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          o[k] = finish(dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a[k], a[k + 1], a[k + 2], b[k], b[k + 1],
                                b[k + 2], c[k], c[k + 1], c[k + 2]));
        }
        const float mm = fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3])));
        m = fmaxf(m, keep(mm, is_out));
        if (!NOSTORE && is_out) {
          if (g.nts) __builtin_nontemporal_store((f4){o[0], o[1], o[2], o[3]}, reinterpret_cast<f4*>(yp + (int64_t)r * g.Wo));
          else *reinterpret_cast<f4*>(yp + (int64_t)r * g.Wo) = (f4){o[0], o[1], o[2], o[3]};
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          a[k] = b[k];
          b[k] = c[k];
        }
      };
      int r0 = 0;
      for (; r0 + D <= g.Ho; r0 += D) {
        f4 nxt[D];
#pragma unroll
        for (int k = 0; k < D; ++k) nxt[k] = ldrow(r0 + k + 1 + D);
#pragma unroll
        for (int k = 0; k < D; ++k) emit(r0 + k, raw[k]);
#pragma unroll
        for (int k = 0; k < D; ++k) raw[k] = nxt[k];
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (r0 + k < g.Ho) emit(r0 + k, raw[k]);
    } else {
      // stride 2: lane holds input columns 4j..4j+3 -> outputs 2j (cols 4j-1,4j,4j+1) and 2j+1 (cols 4j+1..4j+3)
      float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};              // (left, x, y, z, w) of input row 2r-1
      f4 rb[D], rc[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        rb[k] = ldrow(2 * k);
        rc[k] = ldrow(2 * k + 1);
      }
      auto emit2 = [&](int r, f4 braw, f4 craw) {
        const f4 vb = quant4(braw), vc = quant4(craw);
        const float b[5] = {lane_prev(vb.w), vb.x, vb.y, vb.z, vb.w};
        const float c[5] = {lane_prev(vc.w), vc.x, vc.y, vc.z, vc.w};
        float o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          o[k] = finish(dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a[2 * k], a[2 * k + 1], a[2 * k + 2], b[2 * k],
                                b[2 * k + 1], b[2 * k + 2], c[2 * k], c[2 * k + 1], c[2 * k + 2]));
        }
        m = fmaxf(m, keep(fmaxf(fabsf(o[0]), fabsf(o[1])), is_out));
        if (is_out) {
          typedef float f2v __attribute__((ext_vector_type(2)));
          if (g.nts) __builtin_nontemporal_store((f2v){o[0], o[1]}, reinterpret_cast<f2v*>(yp + (int64_t)r * g.Wo));
          else *reinterpret_cast<float2*>(yp + (int64_t)r * g.Wo) = make_float2(o[0], o[1]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) a[k] = c[k];
      };
      int r0 = 0;
      for (; r0 + D <= g.Ho; r0 += D) {
        f4 nb[D], nc[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          nb[k] = ldrow(2 * (r0 + k + D));
          nc[k] = ldrow(2 * (r0 + k + D) + 1);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) emit2(r0 + k, rb[k], rc[k]);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          rb[k] = nb[k];
          rc[k] = nc[k];
        }
      }
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (r0 + k < g.Ho) emit2(r0 + k, rb[k], rc[k]);
    }
    if (has_stat) dw_stat_update(k_stat, rg.s_base, sample, is_out, m, lane, stat_out);
  }
  if (has_stat) dw_stat_flush(k_stat, rg.s_base, rg.n_samples, stat_out);
}

}  // namespace

namespace fqi {
// ---- K2e / K2d, cols4 and cols: one geometry (dw_col_geom) and one grid rule (dw_cols_grid), both in fq_dw.h -----------------
bool dw_cols4_applies(const DwCall& d, int form) {
  const bool can4 = (d.wdt % 4 == 0) && aligned16(d.x) && aligned16(d.y) && aligned16(d.x_codes_out) && ((d.h * d.wdt) % 4 == 0) &&
                    (d.stride == 1 || ((d.wdt / 2) % 2 == 0));
  return (form == 3 || form == 0) && can4;
}
int dw_run_cols4(const DwCall& d) {
  DwColGeom cg = dw_col_geom(d, (int)(d.wdt / 4), d.stride == 1 ? 2 : 1);      // compute lanes per full row: quads
  const int64_t total_segs = d.n * d.c * cg.nsegx;
  FQ_REQUIRE(total_segs < (1ll << 31) - 1024, "fq_dwconv3x3: tensor too large for 32-bit segment indices");
  const int grid = dw_cols_grid(total_segs, cg);
  // nontemporal loads above this many MB of input (300 through round 4 = the 411 MB tensor only; 200 takes in the three
  // 205 MB ones: +0.4 ... +0.7 % images/s in two alternating A/Bs, 100 +0.3 %, 500 -0.5 %: profiles/r5_heuristics_ab.txt)
  static const int dw_nt_mb = env_int("FQ_DW_NT_MB", 200);
  const bool nt = 4.0 * (double)d.n * d.c * d.h * d.wdt > 1e6 * dw_nt_mb;
  static const int dw_nts_mb = env_int("FQ_DW_NTS_MB", 1 << 30);        // nontemporal stores from this many MB of output on
  cg.nts = 4.0 * (double)d.n * d.c * cg.Ho * cg.Wo >= 1e6 * dw_nts_mb ? 1 : 0;
  auto go = [&](auto s, auto nt_c) {
    return dw_launch(d, grid, 0, [](auto q, auto o, auto e) {
      return dwconv3x3_cols4_kernel<decltype(s)::value, q(), o(), decltype(nt_c)::value, e()>;
    }, cg, total_segs);
  };
  if (d.y == nullptr) {       // the statistic pass (dwconv3x3_impl: stride 1, quantised input)
    auto go_stat = [&](auto nt_c) {
      return dw_launch(d, grid, 0, [](auto, auto o, auto e) {
        return dwconv3x3_cols4_kernel<1, true, o(), decltype(nt_c)::value, e(), true>;
      }, cg, total_segs);
    };
    return nt ? go_stat(std::true_type{}) : go_stat(std::false_type{});
  }
  if (d.stride == 1) return nt ? go(dw_int<1>{}, std::true_type{}) : go(dw_int<1>{}, std::false_type{});
  return nt ? go(dw_int<2>{}, std::true_type{}) : go(dw_int<2>{}, std::false_type{});
}
bool dw_cols_applies(const DwCall& d, int form) {      // narrow planes (7x7): LDS staging coalesces better
  return form == 2 || ((form == 0 || form == 3) && d.wdt >= 14);
}
int dw_run_cols(const DwCall& d) {
  const DwColGeom cg = dw_col_geom(d, (int)d.wo, d.stride == 1 ? 2 : 1);
  const int64_t total_segs = d.n * d.c * cg.nsegx;
  FQ_REQUIRE(total_segs < (1ll << 31) - 1024, "fq_dwconv3x3: tensor too large for 32-bit segment indices");
  const int grid = dw_cols_grid(total_segs, cg);
  auto go = [&](auto s) {
    return dw_launch(d, grid, 0, [](auto q, auto o, auto e) {
      return dwconv3x3_cols_kernel<decltype(s)::value, q(), o(), e()>;
    }, cg, total_segs);
  };
  return d.stride == 1 ? go(dw_int<1>{}) : go(dw_int<2>{});
}
}  // namespace fqi
