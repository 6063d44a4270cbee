// libfakequant — K2c depthwise 3x3 with quantise-on-load on LDS tiles: the form of fq_dwconv3x3 that takes every shape
#include "fq_dw.h"      // what the depthwise forms share; fq_common.h: the list of units, the design rules

namespace {
// K2c: depthwise 3x3 (pad 1, stride S) with quantise-on-load and BN / activation / statistic epilogue.
// A workgroup step ("tile") is P whole planes (small planes) or a strip of output rows of one plane (large planes).
// The input rows of a tile are contiguous in memory: they are read once, coalesced (16 B per lane), quantised ONCE per
// element and staged into an LDS tile that carries a zero border, so the 9-tap loop has no bounds checks.  In the
// compute phase consecutive lanes own consecutive output COLUMNS (conflict-free LDS reads, coalesced stores) and slide
// down a segment of rows keeping the 3x3 window in registers: 3 new LDS values per output (6 for stride 2).
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

}  // namespace

namespace fqi {
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
}  // namespace fqi
