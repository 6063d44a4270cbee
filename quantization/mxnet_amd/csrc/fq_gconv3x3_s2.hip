// libfakequant — K2g2 grouped 3x3 convolution with STRIDE 2 (pad 1, 4 .. 32 channels per group) on int8 codes: the three layers
// that open stages 2, 3 and 4 of the ResNeXt nets (see fq_common.h for the list of translation units and the design rules; what
// the four grouped kernels share: fq_gconv.h)
#include "fq_gconv.h"

namespace {

// K2g2.  Weights, slabs, work split and epilogue are K2g's (fq_gconv3x3.hip): output channel tile ct multiplies with input slab ct
// only, nine v_mfma_i32_32x32x32_i8 per 32 OUTPUT pixels, the nine A fragments resident while the workgroup walks a band of NB
// pixel blocks, the next block's region quantised under the current block's multiplies, one barrier per block.  What stride 2
// changes is the panel.  Output pixel (oh, ow) reads input (2 oh + dy, 2 ow + dx), so consecutive output pixels are NOT
// consecutive input pixels and K2g's "tap = the panel read dy * W + dx rows further on" has nothing to shift.  Therefore:
//   * PARITY PHASES.  The quantised input of a region lives in FOUR panels, one per (row parity pr, column parity pc), each with
//     the OUTPUT's geometry: row p of panel (pr, pc) - p a flattened (n, r, c) position of the (Ho, Wo) plane - holds input pixel
//     (2 r + pr, 2 c + pc).  Tap (dy, dx) of output pixel j is then row j + (dy < 0 ? -Wo : 0) + (dx < 0 ? -1 : 0) of panel
//     (dy & 1, dx & 1): a wave-uniform shift again, 32 consecutive output pixels are 32 consecutive panel rows for every tap;
//   * the halo is Wo + 1 positions on ONE side (in front), and only taps with dy < 0 or dx < 0 reach into it.  All four panels
//     keep the same origin j0 - Wo - 1 (one address rule); the even-row panels skip the region tiles no tap of theirs reads;
//   * positions of an odd phase that do not exist - row H of an odd plane, column W of an odd row - hold a clamped neighbour.  The
//     nine validity bits per lane and pixel tile turn them, the padding and the neighbouring sample into code 0: dy = -1 at
//     oh = 0, dy = +1 at 2 oh + 1 >= H, the same in x;
//   * a load unit is (region tile of 32 positions, slab, row parity): lane = position, 16 channels, BOTH column phases - one
//     8-byte load per channel fetches input columns 2 c and 2 c + 1 when W is even (every address is then 8-byte aligned), two
//     4-byte loads when W is odd - quantised into two ds_write_b128, one per column-phase panel.
// The kernel quantises four input values per output value and multiplies as much as K2g per OUTPUT pixel: it lives on loads in
// flight, so the block is PT = 2 tiles (64 output pixels) with two slabs - two regions of (64 + Wo + 1 -> 96 positions) x 4 panels
// x 80 bytes = 60 KiB at every ResNeXt plane, two workgroups per compute unit - and PT = 4 stays behind FQ_GCS2_PT for the table in
// DESIGN 3.11.  One slab (C == 32): four pixel tiles, one per wavefront.
// Budget per wavefront: 36 (A) + 16 * PTW (accumulators) + 64 (two units of 2 x 16 values in flight) + 8 (B) VGPRs.
constexpr int kGs2NW = 4;

template <int WC, int PT>
__global__ __launch_bounds__(kGs2NW * 64, 2) void gconv3x3_s2_i8_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, float* __restrict__ y, GcGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out) {
  constexpr int NW = kGs2NW, WP = NW / WC, PTW = PT / WP, NCH = WC * 32, BPX = 32 * PT;
  static_assert(PTW >= 1 && PTW * WP == PT, "every wavefront owns whole pixel tiles");
  extern __shared__ __attribute__((aligned(16))) unsigned char gs2_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;      // one phase; a set is four of them
  const unsigned set_bytes = 4u * panel_bytes;
  const GcTables ct = gc_tables<NCH>(gs2_smem + 2u * set_bytes);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HWo = (unsigned)g.HWo, Wo = (unsigned)g.Wo, cols = (unsigned)g.cols;
  const unsigned plane4i = (unsigned)g.HW * 4u, plane4o = HWo * 4u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  const bool evenw = g.evenw != 0;
  unsigned item, blk0, blk1, s_band;
  int slab0, ch0;
  if (!mma_xcd_item(g.items, item)) return;
  gc_work_item<WC, BPX>(g, HWo, item, slab0, ch0, blk0, blk1, s_band);
  const int64_t samp_i = (int64_t)g.C * g.HW * 4, samp_o = (int64_t)g.C * HWo * 4;
  const int64_t n_samp = (int64_t)(cols / HWo);

  // ---- a block's region -> a set of four panels: units of (region tile, slab, row parity), wave-strided -------------------------
  const int NU = g.RT * WC * 2;
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) { return gc_region_of(x, blk, BPX, Wo, HWo, samp_i, n_samp); };
  // (an even-row panel is read at the shifts 0 and -1 only: its tiles in front of position Wo are never looked at)
  auto unit_ok = [&](int u) __attribute__((always_inline)) {
    const int us = u >> 1, rt = us / WC;
    return u < NU && slab0 + (us - rt * WC) < g.NSLAB && ((u & 1) || rt * 32 + 31 >= (int)Wo);
  };
  auto issue = [&](const GcRegion& r, int u, float (&v)[2][16]) __attribute__((always_inline)) {
    const int pr = u & 1, us = u >> 1, rt = us / WC, s = us - rt * WC;
    int jr = r.jr0 + rt * 32 + pl;
    jr = jr < 0 ? 0 : (jr < (int)cols ? jr : (int)cols - 1);            // outside the tensor: any valid position (masked later)
    const unsigned nr = (unsigned)jr / HWo, rem = (unsigned)jr - nr * HWo;
    const unsigned rr = rem / Wo, cc = rem - rr * Wo;
    unsigned ih = 2u * rr + (unsigned)pr;
    ih = ih < (unsigned)g.H ? ih : (unsigned)g.H - 1u;                  // row H of an odd plane does not exist: its neighbour
    const unsigned xo = ((nr - r.n_base) * (unsigned)g.C + 16u * h) * plane4i + (ih * (unsigned)g.W + 2u * cc) * 4u;
    if (evenw) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint64_t t = gc_ld_b64(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
        v[0][i] = __builtin_bit_cast(float, (unsigned)t);
        v[1][i] = __builtin_bit_cast(float, (unsigned)(t >> 32));
      }
    } else {
      const unsigned xo1 = xo + (2u * cc + 1u < (unsigned)g.W ? 4u : 0u);        // column W of an odd row: its neighbour
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        v[0][i] = buf_ld_f32(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
        v[1][i] = buf_ld_f32(r.xr, xo1, (unsigned)(ch0 + s * 32 + i) * plane4i);
      }
    }
  };
  float bufa[2][16], bufb[2][16];
  const ThresholdReq treq = threshold_request(in_stat, n, in_thr, item == 0);   // first in the memory queue (fq_common.h)
  FQ_PIN();
  GcRegion rg = region_of(blk0);
  if (unit_ok(wave)) issue(rg, wave, bufa);                             // in flight during the set-up
  FQ_PIN();
  const float max_ = threshold_finish(treq, in_stat, n, in_thr, cur_max_out, item == 0);
  const QParams q = make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
  const int zoff = g.zoff;
  const float sx = q.scale;
  mma_stat_init(k_stat);
  gc_fill_tables<NCH, NW * 64>(ct, ch0, g.C, sx, zoff, wscale, wsum, bias, bn_scale, bn_shift, has_bn);
  const int ubias = 128 - zoff;
  const unsigned nn_xor = fq_nonneg_xor(ubias);
  const bool nonneg = fq_nonneg(q);
  auto quant_to_set = [&](unsigned char* set, int u, const float (&v)[2][16]) __attribute__((always_inline)) {
    const int pr = u & 1, us = u >> 1, rt = us / WC, s = us - rt * WC;
    unsigned char* row = set + (unsigned)(2 * pr) * panel_bytes + (size_t)(rt * 32 + pl) * g.ROW + s * 32 + 16 * h;
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) *reinterpret_cast<v4i*>(row + (unsigned)pc * panel_bytes) = gc_quant16(v[pc], nonneg, q, ubias, nn_xor);
  };
  // the first region: nothing to hide it under
  for (int u = wave; u < NU; u += 2 * NW) {
    if (unit_ok(u + NW)) issue(rg, u + NW, bufb);
    FQ_PIN();
    if (unit_ok(u)) quant_to_set(gs2_smem, u, bufa);
    FQ_PIN();
    if (unit_ok(u + 2 * NW)) issue(rg, u + 2 * NW, bufa);
    FQ_PIN();
    if (unit_ok(u + NW)) quant_to_set(gs2_smem, u + NW, bufb);
    FQ_PIN();
  }

  // ---- this wavefront's slab: nine A fragments, resident for the whole band ------------------------------------------------------
  const int wc = wave % WC, wp = wave / WC;
  const int slab = slab0 + wc;
  const bool mine = slab < g.NSLAB;                                     // (a slab group wider than the layer: this wavefront
                                                                        // only helps to quantise)
  v4i afrag[9];
  gc_load_afrag(wfrag, slab, mine, lane, afrag);
  const int zb = stored_zero4(ubias);                                   // four codes "0" in the stored representation
  const float* fbias = bias;
  FQ_PIN();
  __syncthreads();                                                      // first set, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* set = gs2_smem + cur * set_bytes;
    unsigned char* other = gs2_smem + (cur ^ 1u) * set_bytes;
    const bool has_next = blk + 1 < blk1;
    const unsigned j0 = blk * (unsigned)BPX;
    const int jr0 = (int)j0 - (int)Wo - 1;
    const unsigned s_base = j0 / HWo;                                   // first sample this block's output touches
    GcRegion nx = rg;
    if (has_next) nx = region_of(blk + 1);
    // per pixel tile: the lane's output pixel, its nine tap-validity bits, its panel row
    unsigned smp[PTW], pp[PTW], tapmask[PTW], rbase[PTW];
#pragma unroll
    for (int t = 0; t < PTW; ++t) {
      unsigned j = j0 + (unsigned)((wp * PTW + t) * 32 + pl);
      j = j < cols ? j : cols - 1;                                      // lanes past the end copy the last pixel
      smp[t] = j / HWo;
      pp[t] = j - smp[t] * HWo;
      const int oh = (int)(pp[t] / Wo), ow = (int)(pp[t] - (unsigned)oh * Wo);
      unsigned m = 0;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const bool ok = (dy >= 0 || oh > 0) && (dy <= 0 || 2 * oh + 1 < g.H) && (dx >= 0 || ow > 0) && (dx <= 0 || 2 * ow + 1 < g.W);
        m |= ok ? (1u << tap) : 0u;
      }
      tapmask[t] = m;
      rbase[t] = (unsigned)((int)j - jr0) * (unsigned)g.ROW + (unsigned)(wc * 32 + 16 * h);
    }
    v16i acc[PTW];
#pragma unroll
    for (int t = 0; t < PTW; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0;
    // unit k of this wavefront (wave + NW k) of the NEXT region rides under tap k: loaded a tap ahead, quantised behind the MFMAs
    if (has_next && unit_ok(wave)) issue(nx, wave, bufa);
    FQ_PIN();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (mine) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const unsigned phase = (unsigned)(((dy & 1) << 1) | (dx & 1)) * panel_bytes;                // wave-uniform, as the shift
        const int shift = ((dy < 0 ? -(int)Wo : 0) + (dx < 0 ? -1 : 0)) * g.ROW;
#pragma unroll
        for (int t = 0; t < PTW; ++t)
          gc_mma_tap(set + phase + (unsigned)((int)rbase[t] + shift), (tapmask[t] >> tap) & 1u, zb, afrag[tap], acc[t]);
      }
      FQ_PIN();
      if (has_next) {
        const int u = wave + NW * tap;
        if (tap < 8 && unit_ok(u + NW)) issue(nx, u + NW, (tap & 1) ? bufa : bufb);
        FQ_PIN();
        if (unit_ok(u)) quant_to_set(other, u, (tap & 1) ? bufb : bufa);
        FQ_PIN();
      }
    }
    if (has_next) {                                                     // a region of more than 36 units (Wo > 80): the rest, plainly
      for (int u = wave + NW * 9; u < NU; u += NW) {
        if (unit_ok(u)) {
          issue(nx, u, bufa);
          quant_to_set(other, u, bufa);
        }
      }
    }
    FQ_PIN();
    __syncthreads();                                  // the next set is whole; every wavefront is done reading this one
    if (has_next) rg = nx;
    if (!mine) continue;
    // ---- epilogue: lane = output pixel; a window (mma_out_rsrc) from this wavefront's slab on -----------------------------------
    const int64_t skip = (int64_t)slab * 32 * plane4o;
    const fq_rsrc yr = mma_out_rsrc(y, s_base, samp_o, skip, mma_out_bytes(s_base, n_samp, samp_o, skip));
    const int cb = wc * 32 + 4 * h;
    mma_epilogue_dispatch(fbias, has_bn, act, q, std::false_type{},
                          [&](auto bias_c, auto bn_c, auto act_c, auto) __attribute__((always_inline)) {
      constexpr int BIAS_M = decltype(bias_c)::value, BN_M = decltype(bn_c)::value, ACT_M = decltype(act_c)::value;
#pragma unroll
      for (int t = 0; t < PTW; ++t) {
        const unsigned yo = ((smp[t] - s_base) * (unsigned)g.C + 4u * h) * plane4o + pp[t] * 4u;
        float m = 0.0f;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int c0 = cb + 8 * gq;
          const v4i zs = *reinterpret_cast<const v4i*>(ct.zs + c0);
          const f4 sxw = *reinterpret_cast<const f4*>(ct.sxw + c0);
          const f4 bsc = *reinterpret_cast<const f4*>(ct.bsc + c0);
          const f4 bsh = *reinterpret_cast<const f4*>(ct.bsh + c0);
          f4 bch = (f4){0.f, 0.f, 0.f, 0.f};
          if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) bch = *reinterpret_cast<const f4*>(ct.bias + c0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = (float)(acc[t][4 * gq + r] + zs[r]) * sxw[r];
            if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) v = v + bch[r];
            if (BN_M == 1 || (BN_M < 0 && has_bn)) {
              v = v * bsc[r];
              v = v + bsh[r];
            }
            v = ACT_M < 0 ? act_rt(v, act) : act_rt(v, ACT_M);
            buf_st_f32(yr, yo, (unsigned)(8 * gq + r) * plane4o, v);
            m = fmaxf(m, fabsf(v));
          }
        }
        if (has_stat) mma_stat_update(k_stat, stat_out, smp[t], s_band, m);
      }
    });
  }
  if (has_stat) {
    __syncthreads();
    mma_stat_flush(k_stat, stat_out, s_band, cols, HWo);
  }
}

constexpr GcEntry kGs2Entry = {"fq_gconv3x3_s2_i8", nullptr, 2, FQ_GCONV3X3_S2_MAX_W, false};

// FQ_GCONV3X3_S2_MAX_W is the widest plane whose two region sets fit with either instantiation the rule below picks
static_assert(gc_lds_bytes(2, 2, 2, (FQ_GCONV3X3_S2_MAX_W + 1) / 2) <= kGcLdsMax &&
              gc_lds_bytes(2, 1, 4, (FQ_GCONV3X3_S2_MAX_W + 1) / 2) <= kGcLdsMax,
              "FQ_GCONV3X3_S2_MAX_W does not follow from the LDS budget");

template <int WC, int PT>
int gconv3x3_s2_go(const GcCall& a, const GcGeom& g, int64_t grid, size_t lds, hipStream_t st) {
  return gc_launch<&gconv3x3_s2_i8_kernel<WC, PT>>(kGs2Entry.name, kGs2NW * 64, FQ_LAUNCH_GCONV3X3S2, {WC, PT, g.NB, a.cg}, a, g, grid, lds,
                                                   st);
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_s2_i8_supported(int64_t cin, int64_t cout, int64_t groups) { return gc_supported(cin, cout, groups); }

int fq_gconv3x3_s2_i8(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                      float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                      const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                      const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  GcCall a = {x, nullptr, wscale, wsum, bias, y, in_stat, 0, in_thr, 0.0f, 0, out_current_max, bn_scale, bn_shift, act, stat_out,
              nullptr, 0};
  bool prezeroed;
  if (int rc = gc_check(kGs2Entry, a, wcodes, n, c, groups, h, w, in_width, in_flags, prezeroed)) return rc;
  const int wc = gc_slabs_per_group(c), wo = (int)((w - 1) / 2 + 1);
  // pixel tiles per block: see the kernel's comment (FQ_GCS2_PT: tuning, read per call, taken where the two sets still fit LDS)
  int pt = wc == 2 ? 2 : 4;
  const int tune_pt = env_int("FQ_GCS2_PT", 0);
  if (wc == 2 && (tune_pt == 2 || tune_pt == 4) && gc_lds_bytes(2, wc, tune_pt, wo) <= kGcLdsMax) pt = tune_pt;
  GcGeom g;
  int64_t grid;
  size_t lds;
  // the band, as the stride-1 form: four blocks, else two (FQ_GCS2_NB: tuning, read per call)
  if (int rc = gc_plan(kGs2Entry, a, wcodes, n, c, h, w, in_flags, pt, 4, env_int("FQ_GCS2_NB", 0), 4, 4, g, grid, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gc_zero_stat(stat_out, prezeroed, n, st)) return rc;
  ProfScope prof(FQ_KERNEL_GCONV3X3, 4.0 * (double)n * c * ((int64_t)g.HW + g.HWo), st);
  if (wc == 1) return gconv3x3_s2_go<1, 4>(a, g, grid, lds, st);
  if (pt == 4) return gconv3x3_s2_go<2, 4>(a, g, grid, lds, st);
  return gconv3x3_s2_go<2, 2>(a, g, grid, lds, st);
}

}  // extern "C"
