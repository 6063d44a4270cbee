// libfakequant — K2gc grouped 3x3 convolution (stride 1, pad 1, 4 .. 32 channels per group) between C16 code tensors
// (fq_gconv3x3_i8_c16): the 3x3 layers of the ResNeXt bottlenecks under stored thresholds
// (see fq_common.h for the list of translation units and the design rules; the fp32 -> fp32 form: fq_gconv3x3.hip; what the
// four grouped kernels share: fq_gconv.h)
#include "fq_gconv.h"

namespace {

// K2gc.  Weights, slabs, bands, the two panels [region pixel][32 WC + 16 bytes], the tap shift and the nine validity bits are
// K2g's (fq_gconv3x3.hip): output channel tile ct multiplies with input slab ct only, nine v_mfma_i32_32x32x32_i8 per 32 pixels,
// the A fragments resident for a band.  What a code tensor on either side changes is everything around the multiplies:
//   * region fill (IN16).  A unit - 32 region pixels x one slab - is ONE 16-byte load per lane: the lane of half h takes its
//     pixel's vector of block 2 slab + h, and the bytes are the panel's bytes.  4 VGPRs and a plain copy, where K2g holds 16
//     VGPRs, sixteen loads and a quantiser per unit: a wavefront issues ALL its units of the next region (UF of them, 16 VGPRs
//     at 56x56) before the first tap and writes them to the other panel behind the sixth, nothing per tap.  Regions of more
//     units (wide planes) take the rest in further rounds behind the multiplies.  fp32 in (codes out only): K2g's quantising
//     fill, two units in flight, after the taps - the form a unit takes whose opening 1x1 cannot write codes;
//   * the registers that frees - K2g: 222 VGPRs, two wavefronts per SIMD - go to occupancy.  PT = 4 pixel tiles per block keeps
//     K2g's block of 128 pixels and asks for three wavefronts per SIMD (__launch_bounds__(256, 3); three workgroups' panels, 41
//     KiB each at 56x56, fit a CU's LDS); PT = 8 doubles the block and the tiles per wavefront under the resident A fragments
//     (half the weight fetches and halo per pixel) at two wavefronts per SIMD.  FQ_GC16_PT picks; DESIGN.md 3.11 has both;
//   * code stores (OUT16).  In the 32x32 accumulator layout the lane of half h holds channels 8 gq + 4 h + r of its pixel: half
//     of each 16-channel block.  Two v_permlane32_swap exchange the packed dwords between lane l and lane l + 32, after which
//     the lane of half h owns block 2 slab + h of its pixel whole: one 16-byte store per lane and tile, 512 contiguous bytes
//     per 32 pixels (FQ_GC16_ST4=1: the dense form's four 4-byte pieces, for the comparison).
// The values are K2g's bit for bit: same sums, same epilogue chain, then the consumer's quantiser from fq_mma.h.
constexpr int kG16NW = 4;
// wavefronts per SIMD asked of the compiler: three with the small block and codes in; the fp32 fill carries K2g's 32 VGPRs of
// values on their way to the quantiser and keeps K2g's two
constexpr int g16_lb(int pt, bool in16) { return pt == 4 && in16 ? 3 : 2; }

template <int WC, int PT, bool IN16, bool OUT16>
__global__ __launch_bounds__(kG16NW * 64, g16_lb(PT, IN16)) void gconv3x3_c16_kernel(
    const void* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, void* __restrict__ y, GcGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out, const float* __restrict__ out_thr) {
  constexpr int NW = kG16NW, WP = NW / WC, PTW = PT / WP, NCH = WC * 32, BPX = 32 * PT;
  constexpr int UF = PT == 4 ? 4 : 6;                                   // IN16: units a wavefront keeps in flight
  extern __shared__ __attribute__((aligned(16))) unsigned char g16_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;
  const GcTables ct = gc_tables<NCH>(g16_smem + 2u * panel_bytes);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HW = (unsigned)g.HW, W = (unsigned)g.W, cols = (unsigned)g.cols;
  const unsigned plane4 = HW * 4u, plane16 = HW * 16u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  unsigned item, blk0, blk1, s_band;
  int slab0, ch0;
  if (!mma_xcd_item(g.items, item)) return;
  gc_work_item<WC, BPX>(g, HW, item, slab0, ch0, blk0, blk1, s_band);
  const int64_t x_samp = IN16 ? (int64_t)g.CB * plane16 : (int64_t)g.C * plane4;
  const int64_t y_samp = OUT16 ? (int64_t)g.CB * plane16 : (int64_t)g.C * plane4;
  const int64_t n_samp = (int64_t)(cols / HW);

  // ---- a block's region -> a panel: units of (region tile of 32 pixels, slab), wave-strided; lane = pixel, 16 channels ------
  const int NU = g.RT * WC;
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) { return gc_region_of(x, blk, BPX, W, HW, x_samp, n_samp); };
  auto unit_ok = [&](int u) __attribute__((always_inline)) { return u < NU && slab0 + u % WC < g.NSLAB; };
  auto unit_pixel = [&](const GcRegion& r, int u, unsigned& nr, unsigned& p) __attribute__((always_inline)) {
    int jr = r.jr0 + (u / WC) * 32 + pl;
    jr = jr < 0 ? 0 : (jr < (int)cols ? jr : (int)cols - 1);            // outside the tensor: any valid pixel (masked later)
    nr = (unsigned)jr / HW;
    p = (unsigned)jr - nr * HW;
  };
  auto panel_at = [&](unsigned char* panel, int u) __attribute__((always_inline)) {
    const int rt = u / WC, s = u - rt * WC;
    return reinterpret_cast<v4i*>(panel + (size_t)(rt * 32 + pl) * g.ROW + s * 32 + 16 * h);
  };
  // IN16: round k0 of a wavefront's units, wave + NW (k0 + k): one 16-byte vector of block 2 slab + h each
  v4i ub[UF];
  auto issue16 = [&](const GcRegion& r, int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < UF; ++k) {
      const int u = wave + NW * (k0 + k);
      if (unit_ok(u)) {
        unsigned nr, p;
        unit_pixel(r, u, nr, p);
        ub[k] = buf_ld_v4i(r.xr, ((nr - r.n_base) * (unsigned)g.CB + (unsigned)h) * plane16 + p * 16u,
                           (unsigned)(2 * (slab0 + u % WC)) * plane16);
      }
    }
  };
  auto write16 = [&](unsigned char* panel, int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < UF; ++k) {
      const int u = wave + NW * (k0 + k);
      if (unit_ok(u)) *panel_at(panel, u) = ub[k];
    }
  };
  const int rounds = (NU + NW * UF - 1) / (NW * UF);                    // (one at 56x56 and below)
  // fp32 in: K2g's unit - sixteen loads, quantised, one ds_write_b128 - two in flight
  auto issue32 = [&](const GcRegion& r, int u, float (&v)[16]) __attribute__((always_inline)) {
    unsigned nr, p;
    unit_pixel(r, u, nr, p);
    const unsigned xo = ((nr - r.n_base) * (unsigned)g.C + 16u * h) * plane4 + p * 4u;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = buf_ld_f32(r.xr, xo, (unsigned)(ch0 + (u % WC) * 32 + i) * plane4);
  };
  float bufa[IN16 ? 1 : 16], bufb[IN16 ? 1 : 16];
  const ThresholdReq treq = threshold_request(in_stat, n, in_thr, item == 0);   // first in the memory queue (fq_common.h)
  FQ_PIN();
  GcRegion rg = region_of(blk0);
  if constexpr (IN16) {
    issue16(rg, 0);                                                     // in flight during the set-up
  } else {
    if (unit_ok(wave)) issue32(rg, wave, bufa);
  }
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
    *panel_at(panel, u) = gc_quant16(v, nonneg, q, ubias, nn_xor);
  };
  // a whole region, nothing to hide it under: the first one, and every region of the fp32 form (whose first unit is in flight);
  // IN16: from round k0 on, of which round `flying` is in flight already
  auto fill = [&](const GcRegion& r, unsigned char* panel, int k0, int flying) __attribute__((always_inline)) {
    if constexpr (IN16) {
      for (int k = k0; k < rounds * UF; k += UF) {
        if (k != flying) issue16(r, k);
        FQ_PIN();
        write16(panel, k);
        FQ_PIN();
      }
    } else {
      for (int u = wave; u < NU; u += 2 * NW) {
        if (unit_ok(u + NW)) issue32(r, u + NW, bufb);
        FQ_PIN();
        if (unit_ok(u)) quant_to_panel(panel, u, bufa);
        FQ_PIN();
        if (unit_ok(u + 2 * NW)) issue32(r, u + 2 * NW, bufa);
        FQ_PIN();
        if (unit_ok(u + NW)) quant_to_panel(panel, u + NW, bufb);
        FQ_PIN();
      }
    }
  };
  fill(rg, g16_smem, 0, 0);

  // ---- this wavefront's slab: nine A fragments, resident for the whole band ------------------------------------------------------
  const int wc = wave % WC, wp = wave / WC;
  const int slab = slab0 + wc;
  const bool mine = slab < g.NSLAB;                                     // (a slab group wider than the layer: this wavefront
                                                                        // only helps to fill)
  v4i afrag[9];
  gc_load_afrag(wfrag, slab, mine, lane, afrag);
  const int zb = stored_zero4(ubias);                                   // four codes "0" in the stored representation
  const float* fbias = bias;
  // the consumer's quantiser of a C16 output (fq_mma.h)
  const QParams q2 = mma_out_qparams<OUT16, false>(out_thr, nullptr, g.out_levels, g.out_lo_neg, eps);
  const int ubias2 = 128 - g.out_zoff;
  FQ_PIN();
  __syncthreads();                                                      // first panel, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* panel = g16_smem + cur * panel_bytes;
    unsigned char* other = g16_smem + (cur ^ 1u) * panel_bytes;
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
    // IN16: the wavefront's first round of the NEXT region is in flight under the taps and lands behind the sixth
    if constexpr (IN16) {
      if (has_next) issue16(nx, 0);
    } else {
      if (has_next && unit_ok(wave)) issue32(nx, wave, bufa);           // (the first unit of the fill behind the taps)
    }
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
      if constexpr (IN16) {
        if (tap == 5 && has_next) {
          write16(other, 0);
          FQ_PIN();
        }
      }
    }
    if (has_next) fill(nx, other, IN16 ? UF : 0, -1);                   // (IN16: the further rounds of a wide plane's region)
    FQ_PIN();
    __syncthreads();                                  // the next panel is whole; every wavefront is done reading this one
    if (has_next) rg = nx;
    if (!mine) continue;
    // ---- epilogue: lane = pixel; a window (mma_out_rsrc) from this wavefront's slab on - OUT16: from its first block on ------
    const int64_t skip = OUT16 ? (int64_t)(2 * slab) * plane16 : (int64_t)slab * 32 * plane4;
    const fq_rsrc yr = mma_out_rsrc(y, s_base, y_samp, skip, mma_out_bytes(s_base, n_samp, y_samp, skip));
    const int cb = wc * 32 + 4 * h;
    mma_epilogue_dispatch(fbias, has_bn, act, q2, std::integral_constant<bool, OUT16>{},
                          [&](auto bias_c, auto bn_c, auto act_c, auto nn2_c) __attribute__((always_inline)) {
      constexpr int BIAS_M = decltype(bias_c)::value, BN_M = decltype(bn_c)::value, ACT_M = decltype(act_c)::value;
      constexpr bool NN2 = decltype(nn2_c)::value;
      constexpr bool FOLD = OUT16 && ACT_M == FQ_ACT_RELU;               // (mma_fold: ReLU and the consumer's clip as one median)
      const QParams qc = mma_fold<ACT_M, FOLD>(q2);
#pragma unroll
      for (int t = 0; t < PTW; ++t) {
        const unsigned yo = ((smp[t] - s_base) * (unsigned)g.C + 4u * h) * plane4 + pp[t] * 4u;
        float m = 0.0f;
        int packed[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          FQ_PIN();                                  // (eight channels' constants at a time: hoisted, they cost the third wavefront)
          const int c0 = cb + 8 * gq;
          const v4i zs = *reinterpret_cast<const v4i*>(ct.zs + c0);
          const f4 sxw = *reinterpret_cast<const f4*>(ct.sxw + c0);
          const f4 bsc = *reinterpret_cast<const f4*>(ct.bsc + c0);
          const f4 bsh = *reinterpret_cast<const f4*>(ct.bsh + c0);
          f4 bch = (f4){0.f, 0.f, 0.f, 0.f};
          if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) bch = *reinterpret_cast<const f4*>(ct.bias + c0);
          float vq[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = (float)(acc[t][4 * gq + r] + zs[r]) * sxw[r];
            if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) v = v + bch[r];
            if (BN_M == 1 || (BN_M < 0 && has_bn)) {
              v = v * bsc[r];
              v = v + bsh[r];
            }
            if (!FOLD) v = ACT_M < 0 ? act_rt(v, act) : act_rt(v, ACT_M);
            vq[r] = v;
            if constexpr (!OUT16) buf_st_f32(yr, yo, (unsigned)(8 * gq + r) * plane4, v);
            m = FOLD ? fmaxf(m, v) : fmaxf(m, fabsf(v));
          }
          if constexpr (OUT16) {
            FQ_PIN();
            packed[gq] = fq_pack4<NN2>(vq[0], vq[1], vq[2], vq[3], qc, ubias2, fq_nonneg_xor(ubias2));
            asm volatile("" : "+v"(packed[gq]));
          }
        }
        if constexpr (OUT16) {
          const unsigned yo16 = (smp[t] - s_base) * (unsigned)g.CB * plane16 + pp[t] * 16u;
          if (g.st4) {                               // four pieces of 4 bytes, 16 bytes apart across lanes (the dense form's)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
              buf_st_f32(yr, yo16 + 4u * h, (unsigned)(gq >> 1) * plane16 + 8u * (gq & 1), __int_as_float(packed[gq]));
          } else {
            // lane l <-> lane l + 32: half 0 keeps (gq 0, gq 1) of both halves = block 2 slab, half 1 gets (gq 2, gq 3) = block
            // 2 slab + 1; dword order inside a block: channels 4 h' + 8 (gq & 1)
            const auto s01 = __builtin_amdgcn_permlane32_swap((unsigned)packed[0], (unsigned)packed[2], false, false);
            const auto s23 = __builtin_amdgcn_permlane32_swap((unsigned)packed[1], (unsigned)packed[3], false, false);
            const f4 o = (f4){__uint_as_float(s01[0]), __uint_as_float(s01[1]), __uint_as_float(s23[0]), __uint_as_float(s23[1])};
            buf_st_v4f(yr, yo16 + (unsigned)h * plane16, 0, o);
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

constexpr GcEntry kG16Entry = {"fq_gconv3x3_i8_c16", "fq_conv3x3_i8_c16", 1, FQ_GCONV3X3_C16_MAX_W, true};

// the panels are K2g's, so the widest plane is: both default instantiations (PT = 4) must fit
static_assert(gc_lds_bytes(1, 2, 4, FQ_GCONV3X3_C16_MAX_W) <= kGcLdsMax && gc_lds_bytes(1, 1, 4, FQ_GCONV3X3_C16_MAX_W) <= kGcLdsMax,
              "FQ_GCONV3X3_C16_MAX_W does not follow from the LDS budget");

template <int WC, int PT, bool IN16, bool OUT16>
int gconv3x3_c16_go(const GcCall& a, const GcGeom& g, int64_t grid, size_t lds, hipStream_t st) {
  return gc_launch<&gconv3x3_c16_kernel<WC, PT, IN16, OUT16>>(kG16Entry.name, kG16NW * 64, FQ_LAUNCH_GCONV3X3_C16,
                                                              {WC, PT / (kG16NW / WC), g.NB, a.cg, IN16 ? 1 : 0, OUT16 ? 1 : 0}, a, g,
                                                              grid, lds, st);
}

// three forms; the larger block (PT = 8) is built for codes on both sides, the form the ResNeXt units run
template <int WC>
int gconv3x3_c16_pick(const GcCall& a, const GcGeom& g, int pt, bool in16, bool out16, int64_t grid, size_t lds, hipStream_t st) {
  if (in16 && out16) return pt == 8 ? gconv3x3_c16_go<WC, 8, true, true>(a, g, grid, lds, st)
                                    : gconv3x3_c16_go<WC, 4, true, true>(a, g, grid, lds, st);
  if (in16) return gconv3x3_c16_go<WC, 4, true, false>(a, g, grid, lds, st);
  return gconv3x3_c16_go<WC, 4, false, true>(a, g, grid, lds, st);
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_i8_c16(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                       const float* bias, void* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w,
                       const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                       const float* bn_scale, const float* bn_shift, int act, float* stat_out, const float* out_thr,
                       int out_width, unsigned out_flags, fqStream_t stream) {
  const bool in16 = x_is_c16 != 0, out16 = out_thr != nullptr;
  GcCall a = {x, nullptr, wscale, wsum, bias, y, in_stat, 0, in_thr, 0.0f, 0, out_current_max, bn_scale, bn_shift, act, stat_out,
              out_thr, 0};
  bool prezeroed;
  if (int rc = gc_check(kG16Entry, a, wcodes, n, c, groups, h, w, in_width, in_flags, prezeroed)) return rc;
  FQ_REQUIRE(in16 || out16, "fq_gconv3x3_i8_c16: neither side is a C16 tensor (use fq_gconv3x3_i8)");
  FQ_REQUIRE(!in16 || in_thr != nullptr, "fq_gconv3x3_i8_c16: a C16 input was quantised with a stored threshold: give in_thr");
  const int wc = gc_slabs_per_group(c);
  // the block: 128 pixels at three wavefronts per SIMD, or (codes on both sides; FQ_GC16_PT=8: tuning, read per call) 256 at two
  int pt = 4;
  if (env_int("FQ_GC16_PT", 0) == 8 && in16 && out16 && gc_lds_bytes(1, wc, 8, (int)w) <= kGcLdsMax) pt = 8;
  GcGeom g;
  int64_t grid;
  size_t lds;
  // the band: two blocks per workgroup - one block has nothing to load under its multiplies, and with a region in flight as one
  // burst more workgroups beat longer bands (measured, DESIGN.md 3.11: 39.2 us against 42.2 with four at 28x28, level at 56x56; four
  // blocks of a 7x7 plane span more samples than the statistic table holds; FQ_GC16_NB: tuning, read per call)
  if (int rc = gc_plan(kG16Entry, a, wcodes, n, c, h, w, in_flags, pt, 2, env_int("FQ_GC16_NB", 0), in16 ? 1 : 4, out16 ? 1 : 4, g, grid,
                       lds))
    return rc;
  if (int rc = gc_out_quant(kG16Entry, out16, out_width, out_flags, g)) return rc;
  g.st4 = env_int("FQ_GC16_ST4", 0) == 1 ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gc_zero_stat(stat_out, prezeroed, n, st)) return rc;
  const double elems = (double)n * c * g.HW;
  ProfScope prof(FQ_KERNEL_GCONV3X3, 8.0 * elems, st, (in16 ? 1.0 : 4.0) * elems + (out16 ? 1.0 : 4.0) * elems);
  if (wc == 2) return gconv3x3_c16_pick<2>(a, g, pt, in16, out16, grid, lds, st);
  return gconv3x3_c16_pick<1>(a, g, pt, in16, out16, grid, lds, st);
}

}  // extern "C"
