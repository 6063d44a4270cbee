// libfakequant — K2g grouped 3x3 convolution (stride 1, pad 1, 4 .. 32 channels per group) on int8 codes: the 3x3 layers of the
// ResNeXt bottlenecks (see fq_common.h for the list of translation units and the design rules; what the four grouped kernels
// share - geometry, work items, regions, A fragments, quantiser, launch, the entry points' checks and plan: fq_gconv.h)
#include "fq_gconv.h"

namespace {

// K2g.  With cin == cout == C and cg = C / groups in {4, 8, 16, 32} no group straddles a slab of 32 channels: output channel
// tile ct multiplies with input slab ct ONLY, K = 9 taps x 32 channels, nine v_mfma_i32_32x32x32_i8 per 32 pixels.  The weights
// arrive expanded to (C, 3, 3, 32) - row co holds its group's cg codes at slab position ((co % 32) / cg) * cg + j, zeros
// elsewhere (ops.weight_codes_g3x3) - so a narrower group rides as a zero-filled block-diagonal tile and fq_weight_codes' buffer
// (row_len 288, row_pad 320: ten fragments per tile, the tenth all zero and never fetched) is taken as it is.
// The dense form (fq_conv3x3_kernel.h) has every channel group re-quantise all Cin channels of its region and streams 9 * Cin / 32
// weight fragments per tile; here the problem partitions:
//   * a work item is (a band of NB consecutive pixel blocks of 128 pixels, WC consecutive slabs).  The workgroup quantises ITS
//     slabs of a block's region (the block and its halo of W + 1 pixels on either side, as the dense form) into an LDS panel
//     [region pixel][32 * WC + 16 bytes]: no input channel is quantised by more than one workgroup column, only the halo repeats;
//   * wavefront (wc, wp) owns slab wc and pixel tiles wp * PTW .. of every block.  Its nine A fragments - 36 VGPRs - are loaded
//     ONCE and stay in registers while the workgroup walks the band;
//   * two panels: while the MFMAs of block i read one, the region of block i + 1 goes through registers (one unit of 32 pixels x
//     32 channels per tap: sixteen buffer loads issued a tap ahead, quantised, one ds_write_b128) into the other.  One barrier per
//     block; the stores of block i follow it, under the first taps of block i + 1;
//   * for tap (dy, dx) the B fragment is the panel read dy * W + dx pixels further on; out-of-image taps become the code 0
//     through nine validity bits per lane and pixel tile; epilogue with lane = pixel: all as in the dense form.
// Budget per wavefront: 36 (A) + 16 * PTW (accumulators) + 32 (two units in flight) + 8 (B) VGPRs; LDS 2 * RT * 32 * (32 WC + 16)
// bytes - 40 KiB at W = 56 with WC = 2 - plus 20 * 32 * WC bytes of per-channel constants.
constexpr int kGcPT = 4;                         // pixel tiles of 32 per block
constexpr int kGcNW = 4;

template <int WC>
__global__ __launch_bounds__(kGcNW * 64, 2) void gconv3x3_i8_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, float* __restrict__ y, GcGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out) {
  constexpr int NW = kGcNW, WP = NW / WC, PTW = kGcPT / WP, NCH = WC * 32, BPX = 32 * kGcPT;
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;
  const GcTables ct = gc_tables<NCH>(gc_smem + 2u * panel_bytes);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HW = (unsigned)g.HW, W = (unsigned)g.W, cols = (unsigned)g.cols;
  const unsigned plane4 = HW * 4u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  unsigned item, blk0, blk1, s_band;
  int slab0, ch0;
  if (!mma_xcd_item(g.items, item)) return;
  gc_work_item<WC, BPX>(g, HW, item, slab0, ch0, blk0, blk1, s_band);
  const int64_t samp = (int64_t)g.C * HW * 4;
  const int64_t n_samp = (int64_t)(cols / HW);

  // ---- a block's region -> a panel: units of (region tile of 32 pixels, slab), wave-strided; lane = pixel, 16 channels ------
  const int NU = g.RT * WC;
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) { return gc_region_of(x, blk, BPX, W, HW, samp, n_samp); };
  auto unit_ok = [&](int u) __attribute__((always_inline)) { return u < NU && slab0 + u % WC < g.NSLAB; };
  auto issue = [&](const GcRegion& r, int u, float (&v)[16]) __attribute__((always_inline)) {
    const int rt = u / WC, s = u - rt * WC;
    int jr = r.jr0 + rt * 32 + pl;
    jr = jr < 0 ? 0 : (jr < (int)cols ? jr : (int)cols - 1);            // outside the tensor: any valid pixel (masked later)
    const unsigned nr = (unsigned)jr / HW;
    const unsigned xo = ((nr - r.n_base) * (unsigned)g.C + 16u * h) * plane4 + ((unsigned)jr - nr * HW) * 4u;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = buf_ld_f32(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4);
  };
  float bufa[16], bufb[16];
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
  auto quant_to_panel = [&](unsigned char* panel, int u, const float (&v)[16]) __attribute__((always_inline)) {
    const v4i f = gc_quant16(v, nonneg, q, ubias, nn_xor);
    const int rt = u / WC, s = u - rt * WC;
    *reinterpret_cast<v4i*>(panel + (size_t)(rt * 32 + pl) * g.ROW + s * 32 + 16 * h) = f;
  };
  // the first region: nothing to hide it under
  for (int u = wave; u < NU; u += 2 * NW) {
    if (unit_ok(u + NW)) issue(rg, u + NW, bufb);
    FQ_PIN();
    if (unit_ok(u)) quant_to_panel(gc_smem, u, bufa);
    FQ_PIN();
    if (unit_ok(u + 2 * NW)) issue(rg, u + 2 * NW, bufa);
    FQ_PIN();
    if (unit_ok(u + NW)) quant_to_panel(gc_smem, u + NW, bufb);
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
  __syncthreads();                                                      // first panel, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* panel = gc_smem + cur * panel_bytes;
    unsigned char* other = gc_smem + (cur ^ 1u) * panel_bytes;
    const bool has_next = blk + 1 < blk1;
    const unsigned j0 = blk * (unsigned)BPX;
    const int jr0 = (int)j0 - (int)W - 1;
    const unsigned s_base = j0 / HW;                                    // first sample this block's output touches
    GcRegion nx = rg;
    if (has_next) nx = region_of(blk + 1);
    // per pixel tile: the lane's pixel, its nine tap-validity bits, its panel row
    unsigned smp[PTW], pp[PTW], tapmask[PTW], rbase[PTW];
#pragma unroll
    for (int t = 0; t < PTW; ++t) {
      unsigned j = j0 + (unsigned)((wp * PTW + t) * 32 + pl);
      j = j < cols ? j : cols - 1;                                      // lanes past the end copy the last pixel
      smp[t] = j / HW;
      pp[t] = j - smp[t] * HW;
      const int hh = (int)(pp[t] / W), ww = (int)(pp[t] - (unsigned)hh * W);
      unsigned m = 0;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const bool ok = hh + dy >= 0 && hh + dy < g.H && ww + dx >= 0 && ww + dx < g.W;
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
        const int shift = ((tap / 3 - 1) * (int)W + (tap % 3 - 1)) * g.ROW;   // wave-uniform
#pragma unroll
        for (int t = 0; t < PTW; ++t)
          gc_mma_tap(panel + (unsigned)((int)rbase[t] + shift), (tapmask[t] >> tap) & 1u, zb, afrag[tap], acc[t]);
      }
      FQ_PIN();
      if (has_next) {
        const int u = wave + NW * tap;
        if (tap < 8 && unit_ok(u + NW)) issue(nx, u + NW, (tap & 1) ? bufa : bufb);
        FQ_PIN();
        if (unit_ok(u)) quant_to_panel(other, u, (tap & 1) ? bufb : bufa);
        FQ_PIN();
      }
    }
    if (has_next) {                                                     // a region of more than 36 units (W > 500): the rest, plainly
      for (int u = wave + NW * 9; u < NU; u += NW) {
        if (unit_ok(u)) {
          issue(nx, u, bufa);
          quant_to_panel(other, u, bufa);
        }
      }
    }
    FQ_PIN();
    __syncthreads();                                  // the next panel is whole; every wavefront is done reading this one
    if (has_next) rg = nx;
    if (!mine) continue;
    // ---- epilogue: lane = pixel; a window (mma_out_rsrc) from this wavefront's slab on ---------------------------------------
    const int64_t skip = (int64_t)slab * 32 * plane4;
    const fq_rsrc yr = mma_out_rsrc(y, s_base, samp, skip, mma_out_bytes(s_base, n_samp, samp, skip));
    const int cb = wc * 32 + 4 * h;
    mma_epilogue_dispatch(fbias, has_bn, act, q, std::false_type{},
                          [&](auto bias_c, auto bn_c, auto act_c, auto) __attribute__((always_inline)) {
      constexpr int BIAS_M = decltype(bias_c)::value, BN_M = decltype(bn_c)::value, ACT_M = decltype(act_c)::value;
#pragma unroll
      for (int t = 0; t < PTW; ++t) {
        const unsigned yo = ((smp[t] - s_base) * (unsigned)g.C + 4u * h) * plane4 + pp[t] * 4u;
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
            buf_st_f32(yr, yo, (unsigned)(8 * gq + r) * plane4, v);
            m = fmaxf(m, fabsf(v));
          }
        }
        if (has_stat) mma_stat_update(k_stat, stat_out, smp[t], s_band, m);
      }
    });
  }
  if (has_stat) {
    __syncthreads();
    mma_stat_flush(k_stat, stat_out, s_band, cols, HW);
  }
}

constexpr GcEntry kGcEntry = {"fq_gconv3x3_i8", "fq_conv3x3_i8", 1, FQ_GCONV3X3_MAX_W, false};

template <int WC>
int gconv3x3_go(const GcCall& a, const GcGeom& g, int64_t grid, size_t lds, hipStream_t st) {
  return gc_launch<&gconv3x3_i8_kernel<WC>>(kGcEntry.name, kGcNW * 64, FQ_LAUNCH_GCONV3X3, {WC, kGcPT / (kGcNW / WC), g.NB, a.cg}, a, g,
                                            grid, lds, st);
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_i8_supported(int64_t cin, int64_t cout, int64_t groups) { return gc_supported(cin, cout, groups); }

int fq_gconv3x3_i8(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                   float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                   const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                   const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  GcCall a = {x, nullptr, wscale, wsum, bias, y, in_stat, 0, in_thr, 0.0f, 0, out_current_max, bn_scale, bn_shift, act, stat_out,
              nullptr, 0};
  bool prezeroed;
  if (int rc = gc_check(kGcEntry, a, wcodes, n, c, groups, h, w, in_width, in_flags, prezeroed)) return rc;
  GcGeom g;
  int64_t grid;
  size_t lds;
  // the band: four blocks per workgroup while that leaves two workgroups per compute unit, else two (FQ_GC_NB: tuning, read per call)
  if (int rc = gc_plan(kGcEntry, a, wcodes, n, c, h, w, in_flags, kGcPT, 4, env_int("FQ_GC_NB", 0), 4, 4, g, grid, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gc_zero_stat(stat_out, prezeroed, n, st)) return rc;
  ProfScope prof(FQ_KERNEL_GCONV3X3, 8.0 * (double)n * c * (h * w), st);
  if (gc_slabs_per_group(c) == 2) return gconv3x3_go<2>(a, g, grid, lds, st);
  return gconv3x3_go<1>(a, g, grid, lds, st);
}

}  // extern "C"
