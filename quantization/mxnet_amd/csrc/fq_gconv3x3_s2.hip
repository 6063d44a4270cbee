// libfakequant — K2g2 grouped 3x3 convolution with STRIDE 2 (pad 1, 4 .. 32 channels per group) on int8 codes: the three layers
// that open stages 2, 3 and 4 of the ResNeXt nets (see fq_common.h for the list of translation units and the design rules)
#include "fq_mma.h"
#include "fq_common.h"

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
struct GS2Geom {
  int C, H, W, HWi;          // the input plane
  int Ho, Wo, HWo;           // the output plane
  int NSLAB, CS;             // slabs of 32 channels; slab groups = ceil(NSLAB / WC)
  int NB;                    // pixel blocks per band
  int RT, ROW;               // region tiles of 32 positions; bytes per position in a panel
  int zoff, evenw;
  int64_t cols, nblocks, items;   // n * HWo; pixel blocks of 32 * PT; bands * CS
};

constexpr int kGs2NW = 4;

// two neighbouring fp32 values with one buffer_load_dwordx2 (as ONE 64-bit integer: the halves are taken by shifts)
__device__ __forceinline__ uint64_t gs2_ld_b64(fq_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}

template <int WC, int PT>
__global__ __launch_bounds__(kGs2NW * 64, 2) void gconv3x3_s2_i8_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, float* __restrict__ y, GS2Geom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out) {
  constexpr int NW = kGs2NW, WP = NW / WC, PTW = PT / WP, NCH = WC * 32, KTS = 10, BPX = 32 * PT;
  static_assert(PTW >= 1 && PTW * WP == PT, "every wavefront owns whole pixel tiles");
  extern __shared__ __attribute__((aligned(16))) unsigned char gs2_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;      // one phase; a set is four of them
  const unsigned set_bytes = 4u * panel_bytes;
  float* c_sxw = reinterpret_cast<float*>(gs2_smem + 2u * set_bytes);
  float* c_bsc = c_sxw + NCH;
  float* c_bsh = c_bsc + NCH;
  float* c_bias = c_bsh + NCH;
  int* c_zs = reinterpret_cast<int*>(c_bias + NCH);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HWo = (unsigned)g.HWo, Wo = (unsigned)g.Wo, cols = (unsigned)g.cols;
  const unsigned plane4i = (unsigned)g.HWi * 4u, plane4o = HWo * 4u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  const bool evenw = g.evenw != 0;
  unsigned item;
  if (!mma_xcd_item(g.items, item)) return;
  const unsigned band = item / (unsigned)g.CS, sg = item - band * (unsigned)g.CS;
  const int slab0 = (int)sg * WC;                                       // first slab of the workgroup
  const int ch0 = slab0 * 32;
  const unsigned blk0 = band * (unsigned)g.NB;
  const unsigned blk1 = blk0 + (unsigned)g.NB < (unsigned)g.nblocks ? blk0 + (unsigned)g.NB : (unsigned)g.nblocks;
  const unsigned s_band = blk0 * (unsigned)BPX / HWo;                   // first sample the band's OUTPUT touches
  const int64_t samp_i = (int64_t)g.C * g.HWi * 4, samp_o = (int64_t)g.C * HWo * 4;
  const int64_t n_samp = (int64_t)(cols / HWo);

  // ---- a block's region -> a set of four panels: units of (region tile, slab, row parity), wave-strided -------------------------
  const int NU = g.RT * WC * 2;
  struct Region {
    fq_rsrc xr;
    int jr0;
    unsigned n_base;
  };
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) {
    Region r;
    r.jr0 = (int)(blk * (unsigned)BPX) - (int)Wo - 1;                   // first position of the region (may be < 0)
    r.n_base = (unsigned)(r.jr0 < 0 ? 0 : r.jr0) / HWo;                 // first sample the region touches
    r.xr = make_rsrc(reinterpret_cast<const char*>(x) + r.n_base * samp_i, (n_samp - r.n_base) * samp_i);
    return r;
  };
  // (an even-row panel is read at the shifts 0 and -1 only: its tiles in front of position Wo are never looked at)
  auto unit_ok = [&](int u) __attribute__((always_inline)) {
    const int us = u >> 1, rt = us / WC;
    return u < NU && slab0 + (us - rt * WC) < g.NSLAB && ((u & 1) || rt * 32 + 31 >= (int)Wo);
  };
  auto issue = [&](const Region& r, int u, float (&v)[2][16]) __attribute__((always_inline)) {
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
        const uint64_t t = gs2_ld_b64(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
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
  auto quant_to_set = [&](unsigned char* set, int u, const float (&v)[2][16]) __attribute__((always_inline)) {
    const int pr = u & 1, us = u >> 1, rt = us / WC, s = us - rt * WC;
    unsigned char* row = set + (unsigned)(2 * pr) * panel_bytes + (size_t)(rt * 32 + pl) * g.ROW + s * 32 + 16 * h;
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      v4i f;
      if (nonneg) {
#pragma unroll
        for (int d = 0; d < 4; ++d)
          f[d] = fq_pack4<true>(v[pc][4 * d + 0], v[pc][4 * d + 1], v[pc][4 * d + 2], v[pc][4 * d + 3], q, ubias, nn_xor);
      } else {
#pragma unroll
        for (int d = 0; d < 4; ++d)
          f[d] = fq_pack4<false>(v[pc][4 * d + 0], v[pc][4 * d + 1], v[pc][4 * d + 2], v[pc][4 * d + 3], q, ubias, nn_xor);
      }
      asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
      *reinterpret_cast<v4i*>(row + (unsigned)pc * panel_bytes) = f;
    }
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
  const fq_rsrc wr = make_rsrc(wfrag + (((int64_t)slab * KTS) << 10), mine ? 9 * 1024 : 0);
  v4i afrag[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) afrag[tap] = buf_ld_v4i(wr, (unsigned)lane * 16u, (unsigned)(tap << 10));
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
    Region nx = rg;
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
        for (int t = 0; t < PTW; ++t) {
          const v4i raw = *reinterpret_cast<const v4i*>(set + phase + (unsigned)((int)rbase[t] + shift));
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

constexpr size_t kGs2LdsMax = 150 * 1024;

constexpr int gs2_region_tiles(int pt, int wo) { return (32 * pt + wo + 1 + 31) / 32; }
constexpr size_t gs2_lds_bytes(int wc, int pt, int wo) {
  return 2 * 4 * (size_t)gs2_region_tiles(pt, wo) * 32 * (32 * wc + 16) + (size_t)(32 * wc) * 5 * sizeof(float);
}
// FQ_GCONV3X3_S2_MAX_W is the widest plane whose two region sets fit with either instantiation the rule below picks
static_assert(gs2_lds_bytes(2, 2, (FQ_GCONV3X3_S2_MAX_W + 1) / 2) <= kGs2LdsMax &&
              gs2_lds_bytes(1, 4, (FQ_GCONV3X3_S2_MAX_W + 1) / 2) <= kGs2LdsMax,
              "FQ_GCONV3X3_S2_MAX_W does not follow from the LDS budget");

struct Gs2Call {
  const float* x; const int8_t* wfrag; const float* wscale; const int32_t* wsum; const float* bias; float* y;
  const float* in_stat; int n; const float* in_thr; float levels; int lo_neg; float* out_current_max;
  const float* bn_scale; const float* bn_shift; int act; float* stat_out; int cg;
};

template <int WC, int PT>
int gconv3x3_s2_go(const Gs2Call& a, const GS2Geom& g, int64_t grid, size_t lds, hipStream_t st) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv3x3_s2_i8_kernel<WC, PT>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGs2LdsMax) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_gconv3x3_s2_i8: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((gconv3x3_s2_i8_kernel<WC, PT>), dim3((unsigned)grid), dim3(kGs2NW * 64), lds, st, a.x, a.wfrag, a.wscale,
                     (const int*)a.wsum, a.bias, a.y, g, a.in_stat, a.n, a.in_thr, a.levels, a.lo_neg, kEps, a.out_current_max,
                     a.bn_scale, a.bn_shift, a.act, a.stat_out);
  note_launch(FQ_KERNEL_GCONV3X3, FQ_LAUNCH_GCONV3X3S2, {WC, PT, g.NB, a.cg});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_s2_i8_supported(int64_t cin, int64_t cout, int64_t groups) {
  return fq_gconv3x3_i8_supported(cin, cout, groups);
}

int fq_gconv3x3_s2_i8(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                      float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                      const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                      const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  FQ_REQUIRE(x && wcodes && wscale && wsum && y, "fq_gconv3x3_s2_i8: null pointer");
  const int64_t ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && n * ho * wo < (1ll << 31) - 4096, "fq_gconv3x3_s2_i8: bad shape");
  FQ_REQUIRE(fq_gconv3x3_s2_i8_supported(c, c, groups), "fq_gconv3x3_s2_i8: %lld channels in %lld groups: the channel count "
             "must be a multiple of 32 and a group 4, 8, 16 or 32 channels wide", (long long)c, (long long)groups);
  FQ_REQUIRE(w <= FQ_GCONV3X3_S2_MAX_W, "fq_gconv3x3_s2_i8: planes up to %d pixels wide (got %lld)", FQ_GCONV3X3_S2_MAX_W,
             (long long)w);
  FQ_REQUIRE(in_stat != nullptr || in_thr != nullptr, "fq_gconv3x3_s2_i8: give in_stat (online), in_thr (offline) or both "
             "(offline, the statistic only feeds out_current_max)");
  FQ_REQUIRE(in_thr != nullptr || out_current_max != nullptr, "fq_gconv3x3_s2_i8: online mode needs out_current_max");
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "fq_gconv3x3_s2_i8: input width %d does not fit int8 codes", in_width);
  FQ_REQUIRE(!(in_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_gconv3x3_s2_i8: unsupported activation flags");
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_gconv3x3_s2_i8: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_gconv3x3_s2_i8: unknown activation %d", act);
  FQ_REQUIRE(aligned16(wcodes) && aligned16(x), "fq_gconv3x3_s2_i8: x and wcodes must be 16-byte aligned");
  const int64_t hwi = h * w, hwo = ho * wo, cols = n * hwo;
  const int nslab = (int)(c / 32);
  const int wc = nslab >= 2 ? 2 : 1;
  // pixel tiles per block: see the kernel's comment (FQ_GCS2_PT: tuning, read per call, taken where the two sets still fit LDS)
  int pt = wc == 2 ? 2 : 4;
  const int tune_pt = env_int("FQ_GCS2_PT", 0);
  if (wc == 2 && (tune_pt == 2 || tune_pt == 4) && gs2_lds_bytes(wc, tune_pt, (int)wo) <= kGs2LdsMax) pt = tune_pt;
  const int blockpx = 32 * pt;
  // 32-bit lane offsets count from the first sample a block's region (input, blockpx + wo + 1 output positions) or the block
  // itself (output, the smaller plane) touches
  FQ_REQUIRE(((blockpx + wo + 1) / hwo + 2) * c * hwi * 4 < (1ll << 31),
             "fq_gconv3x3_s2_i8: the input of a pixel block and its halo must stay within 2 GiB of their first sample");
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_pad = 320, rows_pad = (c + 63) / 64 * 64;            // fq_weight_codes' buffer of the (C, 3, 3, 32) filter
  GS2Geom g;
  g.C = (int)c; g.H = (int)h; g.W = (int)w; g.HWi = (int)hwi;
  g.Ho = (int)ho; g.Wo = (int)wo; g.HWo = (int)hwo;
  g.NSLAB = nslab; g.CS = (nslab + wc - 1) / wc;
  g.cols = cols; g.nblocks = (cols + blockpx - 1) / blockpx;
  // the band, as the stride-1 form: four blocks per workgroup while that leaves two workgroups per compute unit, else two - never
  // one (FQ_GCS2_NB: tuning, read per call)
  int nb = 4;
  if (((g.nblocks + nb - 1) / nb) * g.CS < 2 * (int64_t)num_cu()) nb = 2;
  const int tune = env_int("FQ_GCS2_NB", 0);
  if (tune >= 1 && tune <= 64) nb = tune;
  g.NB = nb;
  g.items = ((g.nblocks + nb - 1) / nb) * g.CS;
  g.RT = gs2_region_tiles(pt, (int)wo); g.ROW = 32 * wc + 16;
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  g.evenw = w % 2 == 0 ? 1 : 0;                                           // (x is 16-byte aligned: every pair of columns 8-byte)
  const int64_t grid = (g.items + 7) / 8 * 8;
  FQ_REQUIRE(grid < (1ll << 31), "fq_gconv3x3_s2_i8: too many pixel blocks");
  const size_t lds = gs2_lds_bytes(wc, pt, (int)wo);
  FQ_REQUIRE(lds <= kGs2LdsMax, "fq_gconv3x3_s2_i8: two region sets of %d positions x %d channels do not fit LDS (planes up to "
             "%d wide)", blockpx + (int)wo + 1, 32 * wc, FQ_GCONV3X3_S2_MAX_W);
  Gs2Call a;
  a.x = x; a.wfrag = wcodes + rows_pad * row_pad;                         // the fragment-major copy
  a.wscale = wscale; a.wsum = wsum; a.bias = bias; a.y = y;
  a.in_stat = in_stat; a.n = (int)n; a.in_thr = in_thr;
  a.levels = act_levels(in_width, in_flags);
  a.lo_neg = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  a.out_current_max = out_current_max; a.bn_scale = bn_scale; a.bn_shift = bn_shift; a.act = act; a.stat_out = stat_out;
  a.cg = (int)(c / groups);
  if (stat_out && !prezeroed) {                                           // (a kernel, not a memset node: safe under graph capture)
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stat_out, n, 0.0f);
    FQ_LAUNCH_CHECK();
  }
  ProfScope prof(FQ_KERNEL_GCONV3X3, 4.0 * (double)n * c * (hwi + hwo), st);
  if (wc == 1) return gconv3x3_s2_go<1, 4>(a, g, grid, lds, st);
  if (pt == 4) return gconv3x3_s2_go<2, 4>(a, g, grid, lds, st);
  return gconv3x3_s2_go<2, 2>(a, g, grid, lds, st);
}

}  // extern "C"
