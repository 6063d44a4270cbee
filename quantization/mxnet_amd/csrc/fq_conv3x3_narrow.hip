// libfakequant — K2w dense 3x3 convolution (stride 1, pad 1) on int8 codes for 16 and 32 input channels: the first two stages of
// the CIFAR ResNets (see fq_common.h for the list of translation units and the design rules)
#include "fq_mma.h"
#include "fq_common.h"

namespace {

// K2w.  The dense form (fq_conv3x3_kernel.h) needs K slabs of 32 channels that do not straddle a tap and 9 * Cin a multiple of 64:
// Cin >= 64.  Below that a pixel's codes are 16 or 32 bytes, the planes are small (32x32, 16x16) and a launch per 32-pixel tile
// would be all set-up.  Here, as in the grouped form (fq_gconv3x3.hip):
//   * a work item is (a band of NB consecutive pixel blocks of 128 pixels, a group of WC channel tiles of 32).  The workgroup
//     quantises ALL Cin channels of a block's region (the block and its halo of W + 1 pixels on either side) into an LDS panel
//     [region pixel][ROW bytes]; every channel tile multiplies with the same panel;
//   * wavefront (wc, wp) owns channel tile wc of the group and pixel tiles wp * PTW .. of every block.  Its NS A fragments
//     (fq_weight_codes' fragment-major copy, rows (tap, ci): row_len 288 / row_pad 320 with Cin = 32, 144 / 192 with Cin = 16; the
//     all-zero padding fragments are never fetched) are loaded ONCE and stay in registers while the workgroup walks the band;
//   * two panels: while the MFMAs of block i read one, the region of block i + 1 goes through registers (units of 16 floats per
//     lane, loaded a K step ahead, quantised, one ds_write_b128) into the other.  One barrier per block;
//   * Cin = 32: one tap is one K slab, NS = 9 v_mfma_i32_32x32x32_i8 per tile; lane half h reads bytes [16 h, 16 h + 16) of its
//     pixel's row, ROW = 48 so that the 16-byte reads of 16 consecutive pixels fall into 16 different bank groups;
//   * Cin = 16: a K slab is TWO taps - in the A fragment lanes 0..31 hold k 0..15 (tap 2 s) and lanes 32..63 k 16..31 (tap
//     2 s + 1) - so the two lane halves read the SAME panel at two different tap shifts, each with its own validity bit.
//     NS = 5: four paired slabs and a half one, whose upper half meets the zero padding of the weight rows (k 144..159) and
//     reads tap 8 again to stay inside the panel.  ROW = 16: consecutive pixels are consecutive 16-byte vectors;
//   * out-of-image taps become the code 0 through nine validity bits per lane and pixel tile (zero padding IS data: for unsigned
//     codes the re-centred byte of code 0, the wsum correction covers all nine taps); channels past Cout of a partial tile are
//     masked through kOobOffset; epilogue with lane = pixel, statistic over existing outputs: all as in the dense form.
// Budget per wavefront: 4 NS (A) + 16 PTW (accumulators) + 32 (two units in flight) + 4 PTW (B) VGPRs; LDS 2 panels of
// NU * 1024 (Cin = 16) / NU * 1536 (Cin = 32) bytes - 8 KiB at W = 32, 18 KiB at W = 16 - plus 20 * 32 * WC bytes of constants.
struct NGeom {
  int Cin, Cout, H, W, HW;
  int CS, CTM;               // channel groups = ceil(channel tiles / WC); channel tiles present in the weight buffer
  int NB;                    // pixel blocks per band
  int NU;                    // units of a region
  int zoff;
  int64_t cols, nblocks, items;   // n * HW; pixel blocks of 128; bands * CS
};

constexpr int kNrPT = 4;                         // pixel tiles of 32 per block
constexpr int kNrNW = 4;
constexpr int nr_row(int cin) { return cin == 16 ? 16 : 48; }
constexpr int nr_ppu(int cin) { return cin == 16 ? 64 : 32; }           // region pixels a unit of 64 lanes x 16 channels covers

template <int CIN, int WC>
__global__ __launch_bounds__(kNrNW * 64, 2) void conv3x3_narrow_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, float* __restrict__ y, NGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out) {
  constexpr int NW = kNrNW, WP = NW / WC, PTW = kNrPT / WP, NCH = WC * 32;
  constexpr int ROW = nr_row(CIN), PPU = nr_ppu(CIN);
  constexpr int NS = CIN == 16 ? 5 : 9;                                 // K slabs multiplied
  constexpr int KTS = CIN == 16 ? 6 : 10;                               // fragments per channel tile in the buffer (row_pad / 32)
  extern __shared__ __attribute__((aligned(16))) unsigned char nr_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.NU * (unsigned)(PPU * ROW);
  float* c_sxw = reinterpret_cast<float*>(nr_smem + 2u * panel_bytes);
  float* c_bsc = c_sxw + NCH;
  float* c_bsh = c_bsc + NCH;
  float* c_bias = c_bsh + NCH;
  int* c_zs = reinterpret_cast<int*>(c_bias + NCH);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const int up = CIN == 16 ? lane : pl;                                 // this lane's pixel in a unit
  const int uc = CIN == 16 ? 0 : 16 * h;                                // ... and its first channel
  const unsigned HW = (unsigned)g.HW, W = (unsigned)g.W, cols = (unsigned)g.cols;
  const unsigned plane4 = HW * 4u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  unsigned item;
  if (!mma_xcd_item(g.items, item)) return;
  const unsigned band = item / (unsigned)g.CS, cg = item - band * (unsigned)g.CS;
  const int ch0 = (int)cg * NCH;                                        // first output channel of the workgroup
  const unsigned blk0 = band * (unsigned)g.NB;
  const unsigned blk1 = blk0 + (unsigned)g.NB < (unsigned)g.nblocks ? blk0 + (unsigned)g.NB : (unsigned)g.nblocks;
  const unsigned s_band = blk0 * (32u * kNrPT) / HW;                    // first sample the band's OUTPUT touches
  const int64_t x_samp = (int64_t)g.Cin * HW * 4, y_samp = (int64_t)g.Cout * HW * 4;
  const int64_t n_samp = (int64_t)(cols / HW);

  // ---- a block's region -> a panel: units of 64 lanes x 16 channels, wave-strided ---------------------------------------------
  const int NU = g.NU;
  struct Region {
    fq_rsrc xr;
    int jr0;
    unsigned n_base;
  };
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) {
    Region r;
    r.jr0 = (int)(blk * (32u * kNrPT)) - (int)W - 1;                    // first pixel of the region (may be < 0)
    r.n_base = (unsigned)(r.jr0 < 0 ? 0 : r.jr0) / HW;                  // first sample the region touches
    r.xr = make_rsrc(reinterpret_cast<const char*>(x) + r.n_base * x_samp, (n_samp - r.n_base) * x_samp);
    return r;
  };
  auto issue = [&](const Region& r, int u, float (&v)[16]) __attribute__((always_inline)) {
    int jr = r.jr0 + u * PPU + up;
    jr = jr < 0 ? 0 : (jr < (int)cols ? jr : (int)cols - 1);            // outside the tensor: any valid pixel (masked later)
    const unsigned nr = (unsigned)jr / HW;
    const unsigned xo = ((nr - r.n_base) * (unsigned)CIN + (unsigned)uc) * plane4 + ((unsigned)jr - nr * HW) * 4u;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = buf_ld_f32(r.xr, xo, (unsigned)i * plane4);
  };
  float bufa[16], bufb[16];
  const ThresholdReq treq = threshold_request(in_stat, n, in_thr, item == 0);   // first in the memory queue (fq_common.h)
  FQ_PIN();
  Region rg = region_of(blk0);
  if (wave < NU) issue(rg, wave, bufa);                                 // in flight during the set-up
  FQ_PIN();
  const float max_ = threshold_finish(treq, in_stat, n, in_thr, cur_max_out, item == 0);
  const QParams q = make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
  const int zoff = g.zoff;
  const float sx = q.scale;
  mma_stat_init(k_stat);
  for (int i = threadIdx.x; i < NCH; i += NW * 64) {
    const bool ok = ch0 + i < g.Cout;
    const int ic = ok ? ch0 + i : 0;
    c_sxw[i] = ok ? sx * wscale[ic] : 0.0f;
    c_zs[i] = ok ? zoff * wsum[ic] : 0;
    c_bias[i] = ok && bias != nullptr ? bias[ic] : 0.0f;
    c_bsc[i] = has_bn && ok ? bn_scale[ic] : (ok ? 1.0f : 0.0f);
    c_bsh[i] = has_bn && ok ? bn_shift[ic] : 0.0f;
  }
  const int ubias = 128 - zoff;
  const unsigned nn_xor = fq_nonneg_xor(ubias);
  const bool nonneg = fq_nonneg(q);
  // (non-negative quotients - unsigned activations - take the 5-instruction quantiser of fq_common.h)
  auto quant_to_panel = [&](unsigned char* panel, int u, const float (&v)[16]) __attribute__((always_inline)) {
    v4i f;
    if (nonneg) {
#pragma unroll
      for (int d = 0; d < 4; ++d) f[d] = fq_pack4<true>(v[4 * d + 0], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3], q, ubias, nn_xor);
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d) f[d] = fq_pack4<false>(v[4 * d + 0], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3], q, ubias, nn_xor);
    }
    asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
    *reinterpret_cast<v4i*>(panel + (unsigned)(u * PPU + up) * (unsigned)ROW + (unsigned)uc) = f;
  };
  // the first region: nothing to hide it under
  for (int u = wave; u < NU; u += 2 * NW) {
    if (u + NW < NU) issue(rg, u + NW, bufb);
    FQ_PIN();
    quant_to_panel(nr_smem, u, bufa);
    FQ_PIN();
    if (u + 2 * NW < NU) issue(rg, u + 2 * NW, bufa);
    FQ_PIN();
    if (u + NW < NU) quant_to_panel(nr_smem, u + NW, bufb);
    FQ_PIN();
  }

  // ---- this wavefront's channel tile: NS A fragments, resident for the whole band -------------------------------------------------
  const int wc = wave % WC, wp = wave / WC;
  const int ctg = (int)cg * WC + wc;                                    // channel tile in the layer
  const int cvalid = g.Cout - (ch0 + wc * 32);                          // valid channels of this wavefront's tile
  const bool mine = ctg < g.CTM && cvalid > 0;                          // (a group wider than the layer: this wavefront only
                                                                        // helps to quantise)
  const fq_rsrc wr = make_rsrc(wfrag + (((int64_t)ctg * KTS) << 10), mine ? NS * 1024 : 0);
  v4i afrag[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) afrag[s] = buf_ld_v4i(wr, (unsigned)lane * 16u, (unsigned)(s << 10));
  const int zb = stored_zero4(ubias);                                   // four codes "0" in the stored representation
  const float* fbias = bias;
  const bool partial = cvalid < 32;
  FQ_PIN();
  __syncthreads();                                                      // first panel, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* panel = nr_smem + cur * panel_bytes;
    unsigned char* other = nr_smem + (cur ^ 1u) * panel_bytes;
    const bool has_next = blk + 1 < blk1;
    const unsigned j0 = blk * (32u * kNrPT);
    const int jr0 = (int)j0 - (int)W - 1;
    const unsigned s_base = j0 / HW;                                    // first sample this block's output touches
    Region nx = rg;
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
      // region row of pixel j + shift: (j - jr0) + shift, in [0, 128 + 2 W + 2) for every tap shift in [-(W + 1), W + 1]
      rbase[t] = (unsigned)((int)j - jr0) * (unsigned)ROW + (unsigned)uc;
    }
    v16i acc[PTW];
#pragma unroll
    for (int t = 0; t < PTW; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0;
    // unit k of this wavefront (wave + NW k) of the NEXT region rides under K slab k: loaded a slab ahead, quantised behind the MFMAs
    if (has_next && wave < NU) issue(nx, wave, bufa);
    FQ_PIN();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (mine) {
        // the tap this lane half multiplies in slab s: Cin = 32 - tap s; Cin = 16 - tap 2 s + h (the half slab: tap 8 twice)
        const int ta = CIN == 16 ? 2 * s : s, tb = CIN == 16 ? (2 * s + 1 < 9 ? 2 * s + 1 : 8) : s;
        const int sha = ((ta / 3 - 1) * (int)W + (ta % 3 - 1)) * ROW, shb = ((tb / 3 - 1) * (int)W + (tb % 3 - 1)) * ROW;
        const int shift = h ? shb : sha;
        const int tap = h ? tb : ta;
#pragma unroll
        for (int t = 0; t < PTW; ++t) {
          const v4i raw = *reinterpret_cast<const v4i*>(panel + (unsigned)((int)rbase[t] + shift));
          const bool tv = (tapmask[t] >> tap) & 1u;
          v4i b;
          b[0] = tv ? raw[0] : zb;
          b[1] = tv ? raw[1] : zb;
          b[2] = tv ? raw[2] : zb;
          b[3] = tv ? raw[3] : zb;
          acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[s], b, acc[t], 0, 0, 0);
        }
      }
      FQ_PIN();
      if (has_next) {
        const int u = wave + NW * s;
        if (s < NS - 1 && u + NW < NU) issue(nx, u + NW, (s & 1) ? bufa : bufb);
        FQ_PIN();
        if (u < NU) quant_to_panel(other, u, (s & 1) ? bufb : bufa);
        FQ_PIN();
      }
    }
    if (has_next) {                                                     // a region of more than NW * NS units (wide planes): the rest
      for (int u = wave + NW * NS; u < NU; u += NW) {
        issue(nx, u, bufa);
        quant_to_panel(other, u, bufa);
      }
    }
    FQ_PIN();
    __syncthreads();                                  // the next panel is whole; every wavefront is done reading this one
    if (has_next) rg = nx;
    if (!mine) continue;
    // ---- epilogue: lane = pixel; a window (mma_out_rsrc) from this wavefront's channel tile on; channels past Cout: kOobOffset --
    const int64_t skip = (int64_t)(ch0 + wc * 32) * plane4;
    const fq_rsrc yr = mma_out_rsrc(y, s_base, y_samp, skip, mma_out_bytes(s_base, n_samp, y_samp, skip));
    const int cb = wc * 32 + 4 * h;
    mma_epilogue_dispatch(fbias, has_bn, act, q, std::false_type{},
                          [&](auto bias_c, auto bn_c, auto act_c, auto) __attribute__((always_inline)) {
      constexpr int BIAS_M = decltype(bias_c)::value, BN_M = decltype(bn_c)::value, ACT_M = decltype(act_c)::value;
#pragma unroll
      for (int t = 0; t < PTW; ++t) {
        const unsigned yo = ((smp[t] - s_base) * (unsigned)g.Cout + 4u * h) * plane4 + pp[t] * 4u;
        float m = 0.0f;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int c0 = cb + 8 * gq;
          const v4i zs = *reinterpret_cast<const v4i*>(c_zs + c0);
          const f4 sxw = *reinterpret_cast<const f4*>(c_sxw + c0);
          const f4 bsc = *reinterpret_cast<const f4*>(c_bsc + c0);
          const f4 bsh = *reinterpret_cast<const f4*>(c_bsh + c0);
          f4 bch = (f4){0.f, 0.f, 0.f, 0.f};
          if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) bch = *reinterpret_cast<const f4*>(c_bias + c0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = (float)(acc[t][4 * gq + r] + zs[r]) * sxw[r];
            if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) v = v + bch[r];
            if (BN_M == 1 || (BN_M < 0 && has_bn)) {
              v = v * bsc[r];
              v = v + bsh[r];
            }
            v = ACT_M < 0 ? act_rt(v, act) : act_rt(v, ACT_M);
            const unsigned off = partial ? (8 * gq + 4 * h + r < cvalid ? yo : kOobOffset) : yo;
            buf_st_f32(yr, off, (unsigned)(8 * gq + r) * plane4, v);
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

size_t nr_lds_bytes(int cin, int wc, int nu) {
  return 2 * (size_t)nu * nr_ppu(cin) * nr_row(cin) + (size_t)(32 * wc) * 5 * sizeof(float);
}

template <int CIN, int WC>
int conv3x3_narrow_go(const float* x, const int8_t* wfrag, const float* wscale, const int32_t* wsum, const float* bias, float* y,
                      const NGeom& g, int64_t grid, size_t lds, hipStream_t st, const float* in_stat, int n, const float* in_thr,
                      float levels, int lo_neg, float* out_current_max, const float* bn_scale, const float* bn_shift, int act,
                      float* stat_out) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_narrow_kernel<CIN, WC>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_conv3x3_i8_narrow: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((conv3x3_narrow_kernel<CIN, WC>), dim3((unsigned)grid), dim3(kNrNW * 64), lds, st, x, wfrag, wscale,
                     (const int*)wsum, bias, y, g, in_stat, n, in_thr, levels, lo_neg, kEps, out_current_max, bn_scale,
                     bn_shift, act, stat_out);
  note_launch(FQ_KERNEL_CONV3X3_NARROW, FQ_LAUNCH_CONV3X3_NARROW, {CIN, WC, kNrPT / (kNrNW / WC), g.NB});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_conv3x3_i8_narrow(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                         float* y, int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, const float* in_stat,
                         const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                         const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  FQ_REQUIRE(x && wcodes && wscale && wsum && y, "fq_conv3x3_i8_narrow: null pointer");
  FQ_REQUIRE(n > 0 && cout > 0 && h > 0 && w > 0 && n * h * w < (1ll << 31) - 4096 && w < 4096, "fq_conv3x3_i8_narrow: bad shape");
  FQ_REQUIRE(cin == 16 || cin == 32, "fq_conv3x3_i8_narrow: Cin must be 16 or 32, got %lld (64, 128, 256, 512: fq_conv3x3_i8)",
             (long long)cin);
  FQ_REQUIRE(in_stat != nullptr || in_thr != nullptr, "fq_conv3x3_i8_narrow: give in_stat (online), in_thr (offline) or both "
             "(offline, the statistic only feeds out_current_max)");
  FQ_REQUIRE(in_thr != nullptr || out_current_max != nullptr, "fq_conv3x3_i8_narrow: online mode needs out_current_max");
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "fq_conv3x3_i8_narrow: input width %d does not fit int8 codes", in_width);
  FQ_REQUIRE(!(in_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_conv3x3_i8_narrow: unsupported activation flags");
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_conv3x3_i8_narrow: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_conv3x3_i8_narrow: unknown activation %d", act);
  FQ_REQUIRE(aligned16(wcodes) && aligned16(x), "fq_conv3x3_i8_narrow: x and wcodes must be 16-byte aligned");
  const int64_t hw = h * w, cols = n * hw;
  const int blockpx = 32 * kNrPT;
  // 32-bit lane offsets count from the first sample a block's region (input) or the block itself (output) touches
  FQ_REQUIRE(((blockpx + 2 * w + 2) / hw + 2) * cin * hw * 4 < (1ll << 31) && (blockpx / hw + 2) * cout * hw * 4 < (1ll << 31),
             "fq_conv3x3_i8_narrow: a pixel block and its halo must stay within 2 GiB of their first sample");
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_pad = (9 * cin + 63) / 64 * 64, rows_pad = (cout + 63) / 64 * 64;   // fq_weight_codes' buffer: 192 / 320
  const int8_t* wfrag = wcodes + rows_pad * row_pad;                    // its fragment-major copy
  const int nct = (int)((cout + 31) / 32);
  const int wc = nct >= 2 ? 2 : 1;
  NGeom g;
  g.Cin = (int)cin; g.Cout = (int)cout; g.H = (int)h; g.W = (int)w; g.HW = (int)hw;
  g.CS = (nct + wc - 1) / wc; g.CTM = (int)(rows_pad / 32);
  g.cols = cols; g.nblocks = (cols + blockpx - 1) / blockpx;
  // the band: the largest of four, two and one blocks per workgroup that leaves two workgroups per compute unit - the layers are
  // small and bound by latency, not by arithmetic, and an idle compute unit costs more than a band of one block, which has nothing
  // to load under its multiplies (measured at batch 128: 16 -> 16 @32x32 17.8 / 14.2 / 15.9 us with 4 / 2 / 1, 32 -> 32 @16x16
  // 20.7 / 13.6 / 10.8 us; FQ_C3N_NB: tuning, read per call)
  int nb = 4;
  while (nb > 1 && ((g.nblocks + nb - 1) / nb) * g.CS < 2 * (int64_t)num_cu()) nb >>= 1;
  const int tune = env_int("FQ_C3N_NB", 0);
  if (tune >= 1 && tune <= 64) nb = tune;
  g.NB = nb;
  g.items = ((g.nblocks + nb - 1) / nb) * g.CS;
  const int rp = blockpx + 2 * (int)w + 2;
  g.NU = (rp + nr_ppu((int)cin) - 1) / nr_ppu((int)cin);
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  const int64_t grid = (g.items + 7) / 8 * 8;
  FQ_REQUIRE(grid < (1ll << 31), "fq_conv3x3_i8_narrow: too many pixel blocks");
  const size_t lds = nr_lds_bytes((int)cin, wc, g.NU);
  FQ_REQUIRE(lds <= 150 * 1024, "fq_conv3x3_i8_narrow: two regions of %d pixels x %d channels do not fit LDS", rp, (int)cin);
  const float levels = act_levels(in_width, in_flags);
  const int lo_neg = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  if (stat_out && !prezeroed) FQ_HIP(hipMemsetAsync(stat_out, 0, n * sizeof(float), st));
  ProfScope prof(FQ_KERNEL_CONV3X3_NARROW, 4.0 * ((double)n * cin * hw + (double)n * cout * hw), st);
#define FQ_C3N_CASE(CIN_, WC_)                                                                                          \
  if (cin == CIN_ && wc == WC_)                                                                                         \
    return conv3x3_narrow_go<CIN_, WC_>(x, wfrag, wscale, wsum, bias, y, g, grid, lds, st, in_stat, (int)n, in_thr, levels, \
                                        lo_neg, out_current_max, bn_scale, bn_shift, act, stat_out);
  FQ_C3N_CASE(16, 1) FQ_C3N_CASE(16, 2) FQ_C3N_CASE(32, 1)
#undef FQ_C3N_CASE
  return conv3x3_narrow_go<32, 2>(x, wfrag, wscale, wsum, bias, y, g, grid, lds, st, in_stat, (int)n, in_thr, levels, lo_neg,
                                  out_current_max, bn_scale, bn_shift, act, stat_out);
}

}  // extern "C"
