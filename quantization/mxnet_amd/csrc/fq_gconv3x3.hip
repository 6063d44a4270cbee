// libfakequant — K2g grouped 3x3 convolution (stride 1, pad 1, 4 .. 32 channels per group) on int8 codes: the 3x3 layers of the
// ResNeXt bottlenecks (see fq_common.h for the list of translation units and the design rules)
#include "fq_mma.h"
#include "fq_common.h"

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
struct GCGeom {
  int C, H, W, HW;
  int NSLAB, CS;             // slabs of 32 channels; slab groups = ceil(NSLAB / WC)
  int NB;                    // pixel blocks per band
  int RT, ROW;               // region tiles of 32 pixels; bytes per region pixel in a panel
  int zoff;
  int64_t cols, nblocks, items;   // n * HW; pixel blocks of 128; bands * CS
};

constexpr int kGcPT = 4;                         // pixel tiles of 32 per block
constexpr int kGcNW = 4;

template <int WC>
__global__ __launch_bounds__(kGcNW * 64, 2) void gconv3x3_i8_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, float* __restrict__ y, GCGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out) {
  constexpr int NW = kGcNW, WP = NW / WC, PTW = kGcPT / WP, NCH = WC * 32, KTS = 10;
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;
  float* c_sxw = reinterpret_cast<float*>(gc_smem + 2u * panel_bytes);
  float* c_bsc = c_sxw + NCH;
  float* c_bsh = c_bsc + NCH;
  float* c_bias = c_bsh + NCH;
  int* c_zs = reinterpret_cast<int*>(c_bias + NCH);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HW = (unsigned)g.HW, W = (unsigned)g.W, cols = (unsigned)g.cols;
  const unsigned plane4 = HW * 4u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  unsigned item;
  if (!mma_xcd_item(g.items, item)) return;
  const unsigned band = item / (unsigned)g.CS, sg = item - band * (unsigned)g.CS;
  const int slab0 = (int)sg * WC;                                       // first slab of the workgroup
  const int ch0 = slab0 * 32;
  const unsigned blk0 = band * (unsigned)g.NB;
  const unsigned blk1 = blk0 + (unsigned)g.NB < (unsigned)g.nblocks ? blk0 + (unsigned)g.NB : (unsigned)g.nblocks;
  const unsigned s_band = blk0 * (32u * kGcPT) / HW;                    // first sample the band's OUTPUT touches
  const int64_t samp = (int64_t)g.C * HW * 4;
  const int64_t n_samp = (int64_t)(cols / HW);

  // ---- a block's region -> a panel: units of (region tile of 32 pixels, slab), wave-strided; lane = pixel, 16 channels ------
  const int NU = g.RT * WC;
  struct Region {
    fq_rsrc xr;
    int jr0;
    unsigned n_base;
  };
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) {
    Region r;
    r.jr0 = (int)(blk * (32u * kGcPT)) - (int)W - 1;                    // first pixel of the region (may be < 0)
    r.n_base = (unsigned)(r.jr0 < 0 ? 0 : r.jr0) / HW;                  // first sample the region touches
    r.xr = make_rsrc(reinterpret_cast<const char*>(x) + r.n_base * samp, (n_samp - r.n_base) * samp);
    return r;
  };
  auto unit_ok = [&](int u) __attribute__((always_inline)) { return u < NU && slab0 + u % WC < g.NSLAB; };
  auto issue = [&](const Region& r, int u, float (&v)[16]) __attribute__((always_inline)) {
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
  Region rg = region_of(blk0);
  if (unit_ok(wave)) issue(rg, wave, bufa);                             // in flight during the set-up
  FQ_PIN();
  const float max_ = threshold_finish(treq, in_stat, n, in_thr, cur_max_out, item == 0);
  const QParams q = make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
  const int zoff = g.zoff;
  const float sx = q.scale;
  mma_stat_init(k_stat);
  for (int i = threadIdx.x; i < NCH; i += NW * 64) {
    const bool ok = ch0 + i < g.C;
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
  const fq_rsrc wr = make_rsrc(wfrag + (((int64_t)slab * KTS) << 10), mine ? 9 * 1024 : 0);
  v4i afrag[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) afrag[tap] = buf_ld_v4i(wr, (unsigned)lane * 16u, (unsigned)(tap << 10));
  const int zb = stored_zero4(ubias);                                   // four codes "0" in the stored representation
  const float* fbias = bias;
  FQ_PIN();
  __syncthreads();                                                      // first panel, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* panel = gc_smem + cur * panel_bytes;
    unsigned char* other = gc_smem + (cur ^ 1u) * panel_bytes;
    const bool has_next = blk + 1 < blk1;
    const unsigned j0 = blk * (32u * kGcPT);
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
        for (int t = 0; t < PTW; ++t) {
          const v4i raw = *reinterpret_cast<const v4i*>(panel + (unsigned)((int)rbase[t] + shift));
          const bool tv = (tapmask[t] >> tap) & 1u;
          v4i b;
          b[0] = tv ? raw[0] : zb;
          b[1] = tv ? raw[1] : zb;
          b[2] = tv ? raw[2] : zb;
          b[3] = tv ? raw[3] : zb;
          acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[tap], b, acc[t], 0, 0, 0);
        }
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

template <int WC>
int gconv3x3_go(const float* x, const int8_t* wfrag, const float* wscale, const int32_t* wsum, const float* bias, float* y,
                const GCGeom& g, int64_t grid, size_t lds, hipStream_t st, const float* in_stat, int n, const float* in_thr,
                float levels, int lo_neg, float* out_current_max, const float* bn_scale, const float* bn_shift, int act,
                float* stat_out, int cg) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv3x3_i8_kernel<WC>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_gconv3x3_i8: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((gconv3x3_i8_kernel<WC>), dim3((unsigned)grid), dim3(kGcNW * 64), lds, st, x, wfrag, wscale,
                     (const int*)wsum, bias, y, g, in_stat, n, in_thr, levels, lo_neg, kEps, out_current_max, bn_scale,
                     bn_shift, act, stat_out);
  note_launch(FQ_KERNEL_GCONV3X3, FQ_LAUNCH_GCONV3X3, {WC, kGcPT / (kGcNW / WC), g.NB, cg});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_i8_supported(int64_t cin, int64_t cout, int64_t groups) {
  if (cin != cout || cin <= 0 || cin % 32 != 0 || groups <= 1 || cin % groups != 0) return 0;
  const int64_t cg = cin / groups;
  return (cg == 4 || cg == 8 || cg == 16 || cg == 32) ? 1 : 0;
}

int fq_gconv3x3_i8(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                   float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                   const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                   const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  FQ_REQUIRE(x && wcodes && wscale && wsum && y, "fq_gconv3x3_i8: null pointer");
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && n * h * w < (1ll << 31) - 4096, "fq_gconv3x3_i8: bad shape");
  FQ_REQUIRE(fq_gconv3x3_i8_supported(c, c, groups), "fq_gconv3x3_i8: %lld channels in %lld groups: the channel count must be "
             "a multiple of 32 and a group 4, 8, 16 or 32 channels wide (groups == 1: fq_conv3x3_i8)", (long long)c,
             (long long)groups);
  FQ_REQUIRE(w <= FQ_GCONV3X3_MAX_W, "fq_gconv3x3_i8: planes up to %d pixels wide (got %lld)", FQ_GCONV3X3_MAX_W, (long long)w);
  FQ_REQUIRE(in_stat != nullptr || in_thr != nullptr, "fq_gconv3x3_i8: give in_stat (online), in_thr (offline) or both "
             "(offline, the statistic only feeds out_current_max)");
  FQ_REQUIRE(in_thr != nullptr || out_current_max != nullptr, "fq_gconv3x3_i8: online mode needs out_current_max");
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "fq_gconv3x3_i8: input width %d does not fit int8 codes", in_width);
  FQ_REQUIRE(!(in_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_gconv3x3_i8: unsupported activation flags");
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_gconv3x3_i8: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_gconv3x3_i8: unknown activation %d", act);
  FQ_REQUIRE(aligned16(wcodes) && aligned16(x), "fq_gconv3x3_i8: x and wcodes must be 16-byte aligned");
  const int64_t hw = h * w, cols = n * hw;
  const int blockpx = 32 * kGcPT;
  // 32-bit lane offsets count from the first sample a block's region (input) or the block itself (output) touches
  FQ_REQUIRE(((blockpx + 2 * w + 2) / hw + 2) * c * hw * 4 < (1ll << 31),
             "fq_gconv3x3_i8: a pixel block and its halo must stay within 2 GiB of their first sample");
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_pad = 320, rows_pad = (c + 63) / 64 * 64;            // fq_weight_codes' buffer of the (C, 3, 3, 32) filter
  const int8_t* wfrag = wcodes + rows_pad * row_pad;                    // its fragment-major copy
  const int nslab = (int)(c / 32);
  const int wc = nslab >= 2 ? 2 : 1;
  GCGeom g;
  g.C = (int)c; g.H = (int)h; g.W = (int)w; g.HW = (int)hw;
  g.NSLAB = nslab; g.CS = (nslab + wc - 1) / wc;
  g.cols = cols; g.nblocks = (cols + blockpx - 1) / blockpx;
  // the band: four blocks per workgroup while that leaves two workgroups per compute unit, else two - never one: a band of
  // one block has nothing to load under its multiplies (FQ_GC_NB: tuning, read per call)
  int nb = 4;
  if (((g.nblocks + nb - 1) / nb) * g.CS < 2 * (int64_t)num_cu()) nb = 2;
  const int tune = env_int("FQ_GC_NB", 0);
  if (tune >= 1 && tune <= 64) nb = tune;
  g.NB = nb;
  g.items = ((g.nblocks + nb - 1) / nb) * g.CS;
  const int rp = blockpx + 2 * (int)w + 2;
  g.RT = (rp + 31) / 32; g.ROW = 32 * wc + 16;
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  const int64_t grid = (g.items + 7) / 8 * 8;
  FQ_REQUIRE(grid < (1ll << 31), "fq_gconv3x3_i8: too many pixel blocks");
  const size_t lds = 2 * (size_t)g.RT * 32 * g.ROW + (size_t)(32 * wc) * 5 * sizeof(float);
  FQ_REQUIRE(lds <= 150 * 1024, "fq_gconv3x3_i8: two regions of %d pixels x %d channels do not fit LDS (planes up to %d wide)",
             rp, 32 * wc, FQ_GCONV3X3_MAX_W);
  const float levels = act_levels(in_width, in_flags);
  const int lo_neg = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  if (stat_out && !prezeroed) FQ_HIP(hipMemsetAsync(stat_out, 0, n * sizeof(float), st));
  ProfScope prof(FQ_KERNEL_GCONV3X3, 8.0 * (double)n * c * hw, st);
  const int cg = (int)(c / groups);
  if (wc == 2)
    return gconv3x3_go<2>(x, wfrag, wscale, wsum, bias, y, g, grid, lds, st, in_stat, (int)n, in_thr, levels, lo_neg,
                          out_current_max, bn_scale, bn_shift, act, stat_out, cg);
  return gconv3x3_go<1>(x, wfrag, wscale, wsum, bias, y, g, grid, lds, st, in_stat, (int)n, in_thr, levels, lo_neg,
                        out_current_max, bn_scale, bn_shift, act, stat_out, cg);
}

}  // extern "C"
