// libfakequant — K2c/K2d/K2e depthwise 3x3 with quantise-on-load
// (see fq_common.h for the list of translation units and the design rules)
#include "fq_common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat2(float v) { return (f2){v, v}; }

// ---------------------------------------------------------------------------------------------------------------
// What the five kernel forms below share.  Each thing is written here once.
// ---------------------------------------------------------------------------------------------------------------
// (dw_taps, the 3x3 sum of one output, lives in fq_common.h: fq_pwconv_i8_stat recomputes a depthwise layer with it)
// Two outputs as ONE chain of packed fp32 FMAs (v_pk_fma_f32: two IEEE FMAs per lane per instruction, same order)
__device__ __forceinline__ f2 dw_taps2(float w00, float w01, float w02, float w10, float w11, float w12, float w20, float w21,
                                       float w22, f2 a0, f2 a1, f2 a2, f2 b0, f2 b1, f2 b2, f2 c0, f2 c1, f2 c2) {
  f2 acc = {0.f, 0.f};
  acc = __builtin_elementwise_fma(splat2(w00), a0, acc);
  acc = __builtin_elementwise_fma(splat2(w01), a1, acc);
  acc = __builtin_elementwise_fma(splat2(w02), a2, acc);
  acc = __builtin_elementwise_fma(splat2(w10), b0, acc);
  acc = __builtin_elementwise_fma(splat2(w11), b1, acc);
  acc = __builtin_elementwise_fma(splat2(w12), b2, acc);
  acc = __builtin_elementwise_fma(splat2(w20), c0, acc);
  acc = __builtin_elementwise_fma(splat2(w21), c1, acc);
  acc = __builtin_elementwise_fma(splat2(w22), c2, acc);
  return acc;
}

// The input quantiser of a launch (a kernel without one keeps `QParams q = {}`).  dw_qparams loads the threshold where it
// stands; dw_qparams_finish turns the loads that threshold_request issued earlier into the same parameters.
template <bool ONLINE>
__device__ __forceinline__ QParams dw_qparams(const float* in_stat, int n, const float* in_thr,
                                              float levels, int lo_neg_max, float eps, float* cur_max_out) {
  const float max_ = input_threshold(in_stat, n, ONLINE ? nullptr : in_thr, cur_max_out, blockIdx.x == 0);
  return make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
}
template <bool ONLINE>
__device__ __forceinline__ QParams dw_qparams_finish(const ThresholdReq& treq, const float* in_stat, int n,
                                                     const float* in_thr, float levels, int lo_neg_max, float eps,
                                                     float* cur_max_out) {
  const float max_ = threshold_finish(treq, in_stat, n, ONLINE ? nullptr : in_thr, cur_max_out, blockIdx.x == 0);
  return make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
}

// A workgroup takes a CONTIGUOUS range of blocks (few samples -> a small LDS statistic table, one flush) and its
// wavefronts run through them without barriers.  Index arithmetic is unsigned 32-bit (host: total_segs < 2^31): the
// 64-bit divisions it replaces cost each block 2.3 us (tools/dw_trace.py).
struct DwBlkRange {
  unsigned begin, end;      // blocks of this workgroup
  unsigned n_samples;
  unsigned s_base;          // sample of the first block: slot 0 of the statistic table
};
__device__ __forceinline__ DwBlkRange dw_block_range(unsigned nblk, unsigned tsegs, unsigned segs_per_block, unsigned nsegx,
                                                     unsigned C) {
  DwBlkRange r;
  r.begin = (unsigned)((uint64_t)nblk * blockIdx.x / gridDim.x);
  r.end = (unsigned)((uint64_t)nblk * (blockIdx.x + 1) / gridDim.x);
  r.n_samples = tsegs / nsegx / C;
  const unsigned seg0 = r.begin * segs_per_block;
  r.s_base = (seg0 < tsegs ? seg0 : tsegs - 1) / nsegx / C;
  return r;
}

// Per-sample statistic: the workgroup's LDS table k_stat[kStatSlots] holds the maxima of samples s_base .. s_base + 15 as
// bit patterns (|x| >= 0 orders like an unsigned int); samples beyond it go to memory at once.  dw_stat_update is called per
// wavefront and block without a barrier (m: the lane's maximum, counted where is_out), dw_stat_flush once at the end.
// (SampleT: int or unsigned, as the form holds its sample index - the one-type version widens the index differently and costs
// the stride-2 four-columns-per-lane kernels two vector registers)
constexpr int kStatSlots = 16;
template <class SampleT>
__device__ __forceinline__ void dw_stat_update(unsigned* k_stat, unsigned s_base, SampleT sample, bool is_out, float m,
                                               int lane, float* stat_out) {
  const unsigned s0 = (unsigned)__builtin_amdgcn_readfirstlane((int)sample);
  const bool wave_uniform = __all(!is_out || (unsigned)sample == s0);
  if (wave_uniform) {
    const float wm = wave_max_nonneg(is_out ? m : 0.0f);
    if (lane == 0 && __float_as_uint(wm) != 0u) {
      const unsigned slot = s0 - s_base;
      if (slot < (unsigned)kStatSlots) atomicMax(&k_stat[slot], __float_as_uint(wm));
      else atomic_max_f32(stat_out + s0, wm);
    }
  } else if (is_out) {
    const unsigned slot = (unsigned)sample - s_base;
    if (slot < (unsigned)kStatSlots) atomicMax(&k_stat[slot], __float_as_uint(m));
    else atomic_max_f32(stat_out + sample, m);
  }
}
__device__ __forceinline__ void dw_stat_flush(const unsigned* k_stat, unsigned s_base, unsigned n_samples,
                                              float* stat_out) {
  __syncthreads();
  if (threadIdx.x < kStatSlots && k_stat[threadIdx.x] != 0u && s_base + threadIdx.x < n_samples)
    FQ_STAT_FLUSH_MAX(reinterpret_cast<unsigned*>(stat_out) + s_base + threadIdx.x, k_stat[threadIdx.x]);
}

// Loads are UNCONDITIONAL from clamped (always valid) addresses and masked afterwards with a bitwise AND — a
// `cond ? load : 0` select is turned back into a predicated load by hipcc (CodeGenPrepare sinks the load under a
// branch), which then waits vmcnt(0) right behind it and the prefetch ring is gone.
__device__ __forceinline__ float keep(float v, bool ok) { return __uint_as_float(__float_as_uint(v) & (ok ? 0xFFFFFFFFu : 0u)); }
__device__ __forceinline__ f4 keep4(f4 v, bool ok) {
  const unsigned mk = ok ? 0xFFFFFFFFu : 0u;
  f4 r;
  r.x = __uint_as_float(__float_as_uint(v.x) & mk);
  r.y = __uint_as_float(__float_as_uint(v.y) & mk);
  r.z = __uint_as_float(__float_as_uint(v.z) & mk);
  r.w = __uint_as_float(__float_as_uint(v.w) & mk);
  return r;
}
// The value the lane on the left / right holds, 0 for the edge lane of a plane.  The shift is taken by EVERY lane and masked
// afterwards: under a branch the edge lanes would be switched off, and a DPP read from a switched-off lane returns 0
__device__ __forceinline__ float left_of(float v, bool first) {
  const float t = lane_prev(v);
  return first ? 0.0f : t;
}
__device__ __forceinline__ float right_of(float v, bool last) {
  const float t = lane_next(v);
  return last ? 0.0f : t;
}

// ---------------------------------------------------------------------------------------------------------------
// K2c: depthwise 3x3 (pad 1, stride S) with quantise-on-load and BN / activation / statistic epilogue.
// A workgroup step ("tile") is P whole planes (small planes) or a strip of output rows of one plane (large planes).
// The input rows of a tile are contiguous in memory: they are read once, coalesced (16 B per lane), quantised ONCE per
// element and staged into an LDS tile that carries a zero border, so the 9-tap loop has no bounds checks.  In the
// compute phase consecutive lanes own consecutive output COLUMNS (conflict-free LDS reads, coalesced stores) and slide
// down a segment of rows keeping the 3x3 window in registers: 3 new LDS values per output (6 for stride 2).
// ---------------------------------------------------------------------------------------------------------------
struct DwGeom {
  int C, H, W, Ho, Wo;
  int P;        // planes per tile (whole-plane mode) or 1
  int TR;       // output rows per tile
  int strips;   // tiles per plane along rows (1 in whole-plane mode)
  int IR;       // LDS rows per plane (TR*S + 2)
  int WS;       // LDS row stride (>= W + 2)
  int nseg;     // row segments per tile in the compute phase
  int RS;       // output rows per segment
  int vec_in;   // 16-byte loads allowed
};

template <int S, bool QUANT, bool ONLINE>
__global__ __launch_bounds__(kBlock) void dwconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                           const float* __restrict__ bias, float* __restrict__ y,
                                                           DwGeom g, int64_t tiles, const float* __restrict__ in_stat,
                                                           int n, const float* __restrict__ in_thr, float levels,
                                                           int lo_neg_max, float eps,
                                                           float* __restrict__ cur_max_out,
                                                           const float* __restrict__ bn_scale,
                                                           const float* __restrict__ bn_shift, int act,
                                                           float* __restrict__ stat_out) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ float red[4];
  QParams q = {};
  if (QUANT) q = dw_qparams<ONLINE>(in_stat, n, in_thr, levels, lo_neg_max, eps, cur_max_out);
  const int lds_elems = g.P * g.IR * g.WS;
  const int plane_in = g.H * g.W, plane_out = g.Ho * g.Wo;
  const bool has_bn = bn_scale != nullptr;
  const bool has_stat = stat_out != nullptr;

  const ChunkRange rg = block_range(tiles);
  for (int64_t t = rg.begin; t < rg.end; ++t) {
    const int64_t pg = t / g.strips;                   // plane group
    const int strip = (int)(t - pg * g.strips);
    const int64_t plane0 = pg * g.P;                   // first (n*C + c) plane of the tile
    const int ch0 = (int)(plane0 % g.C);               // P divides C: the tile's planes are ch0 .. ch0+P-1 of ONE sample
    const int orow0 = strip * g.TR;                    // first output row
    const int orows = (g.Ho - orow0) < g.TR ? (g.Ho - orow0) : g.TR;
    const int irow_first = orow0 * S - 1;              // input row held by LDS row 0 (may be -1)
    const int r_lo = irow_first < 0 ? 0 : irow_first;
    int r_hi = irow_first + g.IR - 1;
    if (r_hi > g.H - 1) r_hi = g.H - 1;

    __syncthreads();                                   // previous tile fully consumed
    for (int i = threadIdx.x * 4; i < lds_elems; i += kBlock * 4)
      *reinterpret_cast<f4*>(tile + i) = (f4){0.f, 0.f, 0.f, 0.f};     // (allocation is padded to a multiple of 4)
    __syncthreads();
    // ---- load + quantise + stage: rows [r_lo, r_hi] of P consecutive planes -------------------------------------
    // whole-plane mode: r_lo = 0, r_hi = H-1 and the P planes are one contiguous range; strip mode: P = 1.
    {
      const float* src = x + plane0 * (int64_t)plane_in + (int64_t)r_lo * g.W;
      const int rows_per_plane = r_hi - r_lo + 1;
      const int cnt = (g.P > 1) ? g.P * plane_in : rows_per_plane * g.W;
      const unsigned W = (unsigned)g.W, RP = (unsigned)rows_per_plane;
      if (g.vec_in) {
        const f4* p4 = reinterpret_cast<const f4*>(src);
        for (int i = threadIdx.x; i < cnt / 4; i += kBlock) {
          f4 v = p4[i];
          if (QUANT) v = fq_code4(v, q) * q.scale;
          const unsigned e = (unsigned)i * 4u;
          unsigned row = e / W;                                   // row index over the tile's planes
          unsigned col = e - row * W;
          unsigned pl = row / RP;
          unsigned r = row - pl * RP;
          float* d = tile + (pl * g.IR + (r + r_lo - irow_first)) * g.WS + col + 1;
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            d[0] = vv[k];
            ++d;
            if (++col == W) {                                     // next row (possibly next plane)
              col = 0;
              if (++r == RP) { r = 0; ++pl; }
              d = tile + (pl * g.IR + (r + r_lo - irow_first)) * g.WS + 1;
            }
          }
        }
      } else {
        for (int i = threadIdx.x; i < cnt; i += kBlock) {
          float v = src[i];
          if (QUANT) v = fq_code(v, q) * q.scale;
          const unsigned row = (unsigned)i / W;
          const unsigned col = (unsigned)i - row * W;
          const unsigned pl = row / RP;
          const unsigned r = row - pl * RP;
          tile[(pl * g.IR + (r + r_lo - irow_first)) * g.WS + col + 1] = v;
        }
      }
    }
    __syncthreads();
    // ---- sliding 3x3 window down a row segment; lane <-> output column ------------------------------------------
    float m = 0.0f;
    const int items = g.P * g.nseg * g.Wo;
    for (int it = threadIdx.x; it < items; it += kBlock) {
      const unsigned ps = (unsigned)it / (unsigned)g.Wo;
      const unsigned col = (unsigned)it - ps * (unsigned)g.Wo;
      const unsigned pl = ps / (unsigned)g.nseg;
      const unsigned seg = ps - pl * (unsigned)g.nseg;
      const int rr0 = (int)seg * g.RS;
      int rr1 = rr0 + g.RS;
      if (rr1 > orows) rr1 = orows;
      if (rr0 >= rr1) continue;
      const int ch = ch0 + (int)pl;
      const float* wk = wgt + ch * 9;
      const float w00 = wk[0], w01 = wk[1], w02 = wk[2], w10 = wk[3], w11 = wk[4], w12 = wk[5], w20 = wk[6],
                  w21 = wk[7], w22 = wk[8];
      const float bch = bias != nullptr ? bias[ch] : 0.0f;
      const float bsc = has_bn ? bn_scale[ch] : 1.0f, bsh = has_bn ? bn_shift[ch] : 0.0f;
      const float* l = tile + (pl * g.IR + rr0 * S) * g.WS + col * S;       // LDS col 0 == input col -1
      float a0 = l[0], a1 = l[1], a2 = l[2];
      float b0 = 0.f, b1 = 0.f, b2 = 0.f;
      if (S == 1) {
        b0 = l[g.WS];
        b1 = l[g.WS + 1];
        b2 = l[g.WS + 2];
      }
      float* dst = y + (plane0 + pl) * (int64_t)plane_out + (int64_t)(orow0 + rr0) * g.Wo + col;
      for (int r = rr0; r < rr1; ++r) {
        float c0, c1, c2;
        if (S == 1) {
          const float* lc = l + 2 * g.WS;
          c0 = lc[0]; c1 = lc[1]; c2 = lc[2];
        } else {
          const float* lb = l + g.WS;
          b0 = lb[0]; b1 = lb[1]; b2 = lb[2];
          const float* lc = lb + g.WS;
          c0 = lc[0]; c1 = lc[1]; c2 = lc[2];
        }
        float acc = dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a0, a1, a2, b0, b1, b2, c0, c1, c2);
        if (bias != nullptr) acc = (act & kActBiasMul) ? acc * bch : acc + bch;
        if (has_bn) {
          acc = acc * bsc;
          acc = acc + bsh;
        }
        acc = act_rt(acc, act & 15);
        *dst = acc;
        m = fmaxf(m, fabsf(acc));
        dst += g.Wo;
        l += S * g.WS;
        if (S == 1) {
          a0 = b0; a1 = b1; a2 = b2;
          b0 = c0; b1 = c1; b2 = c2;
        } else {
          a0 = c0; a1 = c1; a2 = c2;
        }
      }
    }
    if (has_stat) {
      m = block_max(m, red);
      if (threadIdx.x == 0) atomic_max_f32(stat_out + plane0 / g.C, m);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// K2d: depthwise 3x3, register sliding-window form (no LDS, no barriers).  A wavefront holds `segs` independent
// SEGMENTS; a segment is `sw` adjacent output columns of one plane plus halo lanes (stride 1: one on each side, stride
// 2: one on the left).  Every lane streams ITS input column(s) top to bottom — one coalesced 4-byte load per lane per
// input row, quantised once — and gets its horizontal neighbours from the adjacent lanes with wavefront shuffles; the
// three live input rows stay in registers, loads run D rows ahead of their use.
// ---------------------------------------------------------------------------------------------------------------
struct DwColGeom {
  int C, H, W, Ho, Wo;
  int sw;       // output columns per segment
  int nsegx;    // segments per plane row
  int SEG;      // lanes per segment (sw + halo lanes)
  int segs;     // segments per wavefront
  int nts;      // cols4 form: nontemporal stores (an output the Infinity Cache cannot hold beside the other batches' tensors)
};

template <int S, bool QUANT, bool ONLINE, int EPI>
__global__ __launch_bounds__(kBlock) void dwconv3x3_cols_kernel(
    const float* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
    float* __restrict__ y, DwColGeom g, int64_t total_segs, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out) {
  // output rows of input kept in flight (S=2: 4 loads per row).  (16 / 8 - every row of a 14x14 plane in flight at
  // once - measured SLOWER on the same box: 38 vs 36 us per 512x14x14 layer.)
  constexpr int D = (S == 1) ? 8 : 4;
  __shared__ unsigned k_stat[kStatSlots];
  if (threadIdx.x < kStatSlots) k_stat[threadIdx.x] = 0u;
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

// ---------------------------------------------------------------------------------------------------------------
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
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f2 buf_ld_2f32(fq_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void buf_st_2f32(fq_rsrc r, unsigned voff, unsigned soff, f2 v) {
  typedef unsigned v2u __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, (int)voff, (int)soff, 0);
}

template <int EPI>
__device__ __forceinline__ f2 dw_finish2(f2 acc, bool has_bias, float bch, bool has_bn, float bsc, float bsh, int act) {
  if (EPI == kEpiRuntime) {
    acc.x = dw_finish<EPI>(acc.x, has_bias, bch, has_bn, bsc, bsh, act);
    acc.y = dw_finish<EPI>(acc.y, has_bias, bch, has_bn, bsc, bsh, act);
    return acc;
  }
  acc = acc * splat2(bsc);
  acc = acc + splat2(bsh);
  acc.x = fmaxf(acc.x, 0.0f);
  acc.y = fmaxf(acc.y, 0.0f);
  if (EPI == kEpiBnRelu6) {
    acc.x = fminf(acc.x, 6.0f);
    acc.y = fminf(acc.y, 6.0f);
  }
  return acc;
}

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
  __shared__ unsigned k_stat[kStatSlots];
  if (threadIdx.x < kStatSlots) k_stat[threadIdx.x] = 0u;
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

// ---------------------------------------------------------------------------------------------------------------
// K2p: small planes through an LDS transpose.  The column-walking forms above read and write a plane row by row: every
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
// ---------------------------------------------------------------------------------------------------------------
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
  __shared__ unsigned k_stat[kStatSlots];
  if (threadIdx.x < kStatSlots) k_stat[threadIdx.x] = 0u;
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

// ---------------------------------------------------------------------------------------------------------------
// K2e: the same sliding window with FOUR input columns per lane (16-byte loads, 16-byte stores for stride 1 / 8-byte
// for stride 2) — needs W % 4 == 0.  With 4-byte accesses the kernel above cannot keep enough bytes in flight
// (PMC: 38 % of wave cycles parked on vmcnt at 4.1 TB/s); this form has 4x the bytes per outstanding load.
// Lane p of a segment: p = 0 left-halo lane, 1..L compute lanes (input columns 4(p-1)..4(p-1)+3), L+1 right-halo lane
// (stride 1 only).  Halo lanes load and quantise like the others; their neighbours pick up .w / .x by shuffle.
// ---------------------------------------------------------------------------------------------------------------
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
  __shared__ unsigned k_stat[kStatSlots];
  if (threadIdx.x < kStatSlots) k_stat[threadIdx.x] = 0u;
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

// in_flags bit of the library's own callers: `in_thr` is a range record (fq_common.h: kRangeMode), the weights are integer
// codes held in fp32 and the quantiser hands on CODES (multiply-back scale 1): the depthwise layer of nn.Conv2D(quantized=True)
constexpr unsigned kFlagRangeRecord = 0x100u;
constexpr unsigned kFlagBiasMultiplies = 0x200u;      // `bias` is the per-channel dequantisation factor (kActBiasMul)

namespace {

// One call of the unit: the arguments and what every form derives from them.
struct DwCall {
  const float *x, *w, *bias;
  float* y;
  int64_t n, c, h, wdt;
  int stride;
  const float *in_stat, *in_thr;
  float* out_current_max;
  const float *bn_scale, *bn_shift;
  int act;
  float* stat_out;
  hipStream_t st;
  bool quant, online, prezeroed;
  int epi;                  // kEpi*: the epilogue fixed at compile time, or the run-time one
  float levels, eps;
  int lo_neg;
  int64_t ho, wo;
  void* x_codes_out;        // y == NULL (the statistic pass): where the codes of x go, or NULL
};

// The launch of every form: zeroes the statistic, opens the profile scope, turns (quant, online) and epi into template
// arguments and launches kernel_for(quant_c, online_c, epi_c) with `geom...` between y and in_stat.
template <class KernelFor, class... Geom>
int dw_launch(const DwCall& d, int grid, size_t lds, KernelFor kernel_for, Geom... geom) {
  using std::integral_constant;
  if (d.stat_out && !d.prezeroed) FQ_HIP(hipMemsetAsync(d.stat_out, 0, d.n * sizeof(float), d.st));
  // algorithmic bytes: the layer's; moved: the statistic pass reads x and writes at most one byte per element of it
  const double in_bytes = 4.0 * (double)d.n * d.c * d.h * d.wdt, out_bytes = 4.0 * (double)d.n * d.c * d.ho * d.wo;
  ProfScope prof(FQ_KERNEL_DWCONV, in_bytes + out_bytes, d.st,
                 d.y ? -1.0 : in_bytes + (d.x_codes_out ? 0.25 * in_bytes : 0.0));
  float* const y_arg = d.y ? d.y : static_cast<float*>(d.x_codes_out);      // (the statistic pass takes its code buffer there)
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, d.st, d.x, d.w, d.bias, y_arg, geom..., d.in_stat, (int)d.n,
                       d.in_thr, d.levels, d.lo_neg, d.eps, d.out_current_max, d.bn_scale, d.bn_shift, d.act, d.stat_out);
  };
  auto with_epi = [&](auto quant_c, auto online_c) {
    if (d.epi == kEpiBnRelu) launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiBnRelu>{}));
    else if (d.epi == kEpiBnRelu6) launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiBnRelu6>{}));
    else launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiRuntime>{}));
  };
  if (!d.quant) with_epi(std::false_type{}, std::false_type{});
  else if (d.online) with_epi(std::true_type{}, std::true_type{});
  else with_epi(std::true_type{}, std::false_type{});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}
template <int V>
using dw_int = std::integral_constant<int, V>;

// Persistent grids: a block is what the four wavefronts of a workgroup do in one step (`segs` segments or planes each);
// every workgroup is resident at once and walks a contiguous range of blocks.
int64_t dw_blocks(int64_t total_segs, int segs) {
  const int64_t per_block = (int64_t)segs * (kBlock / 64);
  return (total_segs + per_block - 1) / per_block;
}
int dw_grid(int64_t nblk, int wg_per_cu) {
  const int64_t cap = (int64_t)num_cu() * wg_per_cu;
  return (int)(nblk < cap ? nblk : cap);
}

// Lanes of the register forms: a plane row of `units` compute lanes is cut into nsegx segments of sw lanes, each with `halo`
// lanes beside them, and a wavefront holds as many segments as fit.
DwColGeom dw_col_geom(const DwCall& d, int units, int halo) {
  DwColGeom cg = {};
  cg.C = (int)d.c;
  cg.H = (int)d.h;
  cg.W = (int)d.wdt;
  cg.Ho = (int)d.ho;
  cg.Wo = (int)d.wo;
  const int max_sw = 64 - halo;
  cg.nsegx = (units + max_sw - 1) / max_sw;
  cg.sw = (units + cg.nsegx - 1) / cg.nsegx;
  cg.SEG = cg.sw + halo;
  cg.segs = 64 / cg.SEG;
  return cg;
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
bool dw_flat_applies(const DwCall& d, int form) {
  static const int flat_on = env_int("FQ_DW_FLAT", 31) & 31;
  const int kind = dw_flat_kind(d);
  const bool whole = kind == 0 || kind >= 3 || (d.n * d.c) % dw_flat_planes(kind) == 0;     // planes of 49 floats: no 16-byte tail
  return kind >= 0 && (form == 5 || (form == 0 && ((flat_on >> kind) & 1))) && whole && aligned16(d.x) && aligned16(d.y) &&
         d.n * d.c * d.h * d.wdt * 4 < (1ll << 31);
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
  auto go = [&](auto s, auto hw) {
    return dw_launch(d, grid, 0, [](auto q, auto o, auto e) {
      return dwconv3x3_flat_kernel<decltype(s)::value, q(), o(), decltype(hw)::value, decltype(hw)::value, e()>;
    }, fg);
  };
  return kind == 0 ? go(dw_int<1>{}, dw_int<14>{}) : kind == 1 ? go(dw_int<2>{}, dw_int<14>{})
         : kind == 2 ? go(dw_int<1>{}, dw_int<7>{}) : kind == 4 ? go(dw_int<2>{}, dw_int<28>{})
                     : go(dw_int<1>{}, dw_int<28>{});
}

// ---- K2o, planes: small planes whole in registers, pipelined across blocks ------------------------------------------------
bool dw_planes_two_cols(const DwCall& d) {
  static const int planes_cpl = env_int("FQ_DW_PLANES_CPL", 2);          // 1: one column per lane even where W is even (A/B)
  const bool al8 = ((((uintptr_t)d.x) | ((uintptr_t)d.y)) & 7) == 0;
  return d.wdt % 2 == 0 && al8 && (d.stride == 2 || planes_cpl == 2);
}
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

// ---- K2e / K2d, cols4 and cols: the sliding window with four columns / one column per lane ------------------------------------
// Both: every workgroup resident at once, each walking a contiguous range of blocks.  6 per CU: the kernels use ~100 scalar
// registers, and a CU admits 256-thread workgroups 8 at a time only up to 80 (MI355X_MICROARCH.md, residency) - with
// 8 per CU asked for, a quarter of the grid ran as a second, thin round (14x14 layers: 31.7 -> 28.0 us; capping the
// scalar registers at 80 instead makes all 8 resident and is no faster)
int dw_cols_grid(int64_t total_segs, const DwColGeom& cg) {
  static const int dw_wg_per_cu = env_int("FQ_DW_WG_PER_CU", 6);
  return dw_grid(dw_blocks(total_segs, cg.segs), dw_wg_per_cu);
}
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

// ---- K2c, tiles: every shape ---------------------------------------------------------------------------------------------------
int dw_run_tiles(const DwCall& d) {
  const int stride = d.stride;
  DwGeom g;
  g.C = (int)d.c;
  g.H = (int)d.h;
  g.W = (int)d.wdt;
  g.Ho = (int)d.ho;
  g.Wo = (int)d.wo;
  g.WS = g.W + 2;
  if ((g.WS & 1) == 0) g.WS += 1;                       // odd dword stride
  const int lds_budget = 8192;                          // floats (32 KiB) -> up to 5 workgroups per CU
  const int plane_in = g.H * g.W;
  if (plane_in <= 4096 && (g.H + 2) * g.WS <= lds_budget) {
    g.TR = g.Ho;
    g.strips = 1;
    g.IR = g.H + 2;
    g.P = 1;
    for (int p = (int)(d.c < 64 ? d.c : 64); p >= 1; --p)
      if (d.c % p == 0 && p * g.IR * g.WS <= lds_budget) {
        g.P = p;
        break;
      }
  } else {
    g.P = 1;
    int tr = (lds_budget / g.WS - 2) / stride;
    FQ_REQUIRE(tr >= 1, "fq_dwconv3x3: rows of %d floats do not fit the LDS tile", g.W);
    g.strips = (g.Ho + tr - 1) / tr;
    g.TR = (g.Ho + g.strips - 1) / g.strips;
    g.IR = g.TR * stride + 2;
  }
  {
    const int per_seg = g.P * g.Wo;
    int nseg = (2 * kBlock + per_seg - 1) / per_seg;    // aim at ~2 work items per lane
    if (nseg < 1) nseg = 1;
    if (nseg > g.TR) nseg = g.TR;
    g.RS = (g.TR + nseg - 1) / nseg;
    g.nseg = (g.TR + g.RS - 1) / g.RS;
  }
  const bool base_ok = aligned16(d.x);
  if (g.P > 1 || g.strips == 1)
    g.vec_in = base_ok && (((int64_t)g.P * plane_in) % 4 == 0) && (plane_in % 4 == 0 || g.P % 4 == 0);
  else
    g.vec_in = base_ok && (g.W % 4 == 0) && (plane_in % 4 == 0);
  const int64_t tiles = (d.n * d.c / g.P) * g.strips;
  const size_t lds = (size_t)((g.P * g.IR * g.WS + 3) / 4 * 4 + 16) * sizeof(float);
  auto go = [&](auto s) {       // (this form has the run-time epilogue only)
    return dw_launch(d, grid_for(tiles), lds, [](auto q, auto o, auto) {
      return dwconv3x3_kernel<decltype(s)::value, q(), o()>;
    }, g, tiles);
  };
  return stride == 1 ? go(dw_int<1>{}) : go(dw_int<2>{});
}

}  // namespace

static int dwconv3x3_impl(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                          int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                          float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                          fqStream_t stream, void* x_codes_out = nullptr) {
  FQ_REQUIRE(x && w && (y || stat_out), "fq_dwconv3x3: null pointer");
  FQ_REQUIRE(y || !x_codes_out || (in_width <= 8 && !(in_flags & kFlagRangeRecord) &&
                                   ((in_flags & FQ_ACT_SIGNED) || !(in_flags & FQ_ACT_LO_NEG_MAX))),
             "fq_dwconv3x3: x_codes_out keeps codes that fit a byte (at most 8 bits; unsigned levels with a clip range from 0)");
  FQ_REQUIRE(!(y && x_codes_out), "fq_dwconv3x3: x_codes_out belongs to the statistic pass (y == NULL)");
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && wdt > 0 && n * c < (1ll << 31) && h * wdt < (1ll << 28),
             "fq_dwconv3x3: bad shape (n=%lld c=%lld h=%lld w=%lld)", (long long)n, (long long)c, (long long)h,
             (long long)wdt);
  FQ_REQUIRE(stride == 1 || stride == 2, "fq_dwconv3x3: stride must be 1 or 2, got %d", stride);
  // in_stat alone: online; in_thr alone: offline; both: offline, the statistic only feeds out_current_max
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_dwconv3x3: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_dwconv3x3: unknown activation %d", act);
  const bool quant = in_stat != nullptr || in_thr != nullptr;
  if (quant) FQ_REQUIRE(in_width >= 2 && in_width <= 16, "fq_dwconv3x3: width %d out of range", in_width);
  if (in_flags & kFlagBiasMultiplies) act |= kActBiasMul;   // (after the range check; bias != NULL: run-time epilogue)
  static const int epi_on = env_int("FQ_DW_EPI", 1);    // 0: always the run-time epilogue (A/B)

  DwCall d = {};
  d.x = x; d.w = w; d.bias = bias; d.y = y; d.x_codes_out = x_codes_out;
  d.n = n, d.c = c, d.h = h, d.wdt = wdt, d.stride = stride;
  d.in_stat = in_stat, d.in_thr = in_thr, d.out_current_max = out_current_max;
  d.bn_scale = bn_scale, d.bn_shift = bn_shift, d.act = act, d.stat_out = stat_out;
  d.st = (hipStream_t)stream;
  d.quant = quant, d.online = quant && in_thr == nullptr, d.prezeroed = prezeroed;
  d.epi = (epi_on && bn_scale != nullptr && bias == nullptr)
              ? (act == FQ_ACT_RELU ? kEpiBnRelu : act == FQ_ACT_RELU6 ? kEpiBnRelu6 : kEpiRuntime)
              : kEpiRuntime;
  d.levels = act_levels(in_width, in_flags);
  d.lo_neg = (in_flags & kFlagRangeRecord) ? kRangeMode : ((in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0);
  d.eps = (in_flags & FQ_ACT_NO_EPS) ? 0.0f : kEps;
  d.ho = (h - 1) / stride + 1, d.wo = (wdt - 1) / stride + 1;

  // 0 auto, 1 LDS tiles, 2 one column per lane, 3 four columns per lane, 4 whole planes, 5 flat.  A forced form that does
  // not take the shape falls through to the next one that does.
  static const int form = env_int("FQ_DW_FORM", 0);
  if (y == nullptr) {         // the statistic pass: one form
    FQ_REQUIRE(quant && stride == 1 && dw_cols4_applies(d, 3),
               "fq_dwconv3x3: without y (statistic pass) only stride 1, a quantised input and rows of a multiple of 4 floats, "
               "16-byte aligned, are taken (n=%lld c=%lld h=%lld w=%lld stride %d)", (long long)n, (long long)c, (long long)h,
               (long long)wdt, stride);
    return dw_run_cols4(d);
  }
  if (dw_flat_applies(d, form)) return dw_run_flat(d);
  if (dw_planes_applies(d, form)) return dw_run_planes(d);
  if (dw_cols4_applies(d, form)) return dw_run_cols4(d);
  if (dw_cols_applies(d, form)) return dw_run_cols(d);
  return dw_run_tiles(d);
}

namespace fqi {
// depthwise 3x3 of nn.Conv2D(quantized=True): x quantised on load with the range record `rec` (codes, not values, enter the
// sums), wcodes_f32 = the int8 weight codes as fp32, y = act(sum * svec[c]) with svec = in_scale * w_scale, or - a BatchNorm
// folded behind the block - y = act((sum * svec[c]) * bn_scale[c] + bn_shift[c]), every step separately rounded
int dw_range_call(const float* x, const float* wcodes_f32, float* y, int64_t n, int64_t c, int64_t h, int64_t wdt, int stride,
                  const float* rec, const float* svec, const float* bn_scale, const float* bn_shift, int act,
                  float* stat_out, hipStream_t st) {
  return dwconv3x3_impl(x, wcodes_f32, svec, y, n, c, h, wdt, stride, nullptr, rec, 8, kFlagRangeRecord | kFlagBiasMultiplies,
                        nullptr, bn_scale, bn_shift, act, stat_out, (fqStream_t)st);
}
}  // namespace fqi

extern "C" {

int fq_dwconv3x3(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                 int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                 float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                 fqStream_t stream, void* x_codes_out) {
  FQ_REQUIRE(!(in_flags & ~(FQ_ACT_SIGNED | FQ_ACT_LO_NEG_MAX | FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_dwconv3x3: unknown flags");
  return dwconv3x3_impl(x, w, bias, y, n, c, h, wdt, stride, in_stat, in_thr, in_width, in_flags, out_current_max, bn_scale,
                        bn_shift, act, stat_out, stream, x_codes_out);
}

}  // extern "C"
