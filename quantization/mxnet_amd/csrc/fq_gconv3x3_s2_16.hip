// libfakequant — K2g2c grouped 3x3 convolution with STRIDE 2 (pad 1, 4 .. 32 channels per group) between C16 code tensors
// (fq_gconv3x3_s2_i8_c16): the three layers that open stages 2, 3 and 4 of the ResNeXt nets under stored thresholds
// (see fq_common.h for the list of translation units and the design rules; the fp32 -> fp32 form: fq_gconv3x3_s2.hip)
#include "fq_mma.h"
#include "fq_common.h"

namespace {

// K2g2c.  Weights, slabs, bands, the FOUR PARITY-PHASE PANELS in the output's geometry - row p of panel (pr, pc) holds input
// (2 r + pr, 2 c + pc); a tap is a wave-uniform row shift plus a panel choice; the halo is Wo + 1 positions in front - the clamped
// row H / column W and the nine validity bits per lane and tile are K2g2's (fq_gconv3x3_s2.hip).  The code stores are K2gc's
// (fq_gconv3x3_16.hip).  What is this kernel's own is where the two do not compose:
//   * region fill (IN16).  A unit is K2g2's (region tile of 32 positions, slab, row parity).  In a C16 tensor the two column phases
//     of a position are the two ADJACENT 16-byte vectors (ih, 2 c) and (ih, 2 c + 1) of one block: 32 contiguous bytes, aligned
//     whatever W is, so K2g2's even / odd W split is gone.  The lane of half h loads them from block 2 slab + h with two 16-byte
//     buffer loads - the second clamped to its neighbour where column W does not exist, row H clamped as in K2g2 - and writes them
//     with two plain ds_write_b128, one per column-phase panel: 8 VGPRs and no quantiser per unit where K2g2 holds 32 values and
//     quantises them.  A wavefront issues ALL its units of the next region (UF of them) in one burst before the first tap and
//     writes them behind the sixth; regions of more units (wide planes) take further rounds behind the multiplies.  The even-row
//     panels keep skipping the tiles no tap reads.  fp32 in (codes out only): K2g2's quantising fill, a unit per tap;
//   * the split.  Two sets of four panels are 60 KiB with PT = 2 pixel tiles per block at every ResNeXt plane: two workgroups of
//     four wavefronts per CU whatever the registers allow, so the registers the fill frees (K2g2: 205) cannot buy a third wavefront
//     as they did for K2gc.  They can buy a larger block under the resident A fragments: PT = 4 (half the weight fetches, halo and
//     barriers per pixel; 100 KiB, one workgroup per CU) with four wavefronts of two tiles or eight wavefronts of one.
//     FQ_GCS216_CFG picks among the three for codes on both sides; DESIGN.md 3.11 has the table;
//   * code stores (OUT16): two v_permlane32_swap, then one guarded 16-byte store per lane and tile into [n][C/16][Ho][Wo][16].
// The values are K2g2's bit for bit: same sums, same epilogue chain, then the consumer's quantiser from fq_mma.h.
struct GS216Geom {
  int C, H, W, HWi;          // the input plane
  int Ho, Wo, HWo;           // the output plane
  int NSLAB, CS;             // slabs of 32 channels; slab groups = ceil(NSLAB / WC)
  int NB;                    // pixel blocks per band
  int RT, ROW;               // region tiles of 32 positions; bytes per position in a panel
  int zoff, evenw;
  int CB;                    // 16-channel blocks of a C16 tensor = C / 16
  float out_levels;
  int out_lo_neg, out_zoff;
  int64_t cols, nblocks, items;   // n * HWo; pixel blocks of 32 * PT; bands * CS
};

constexpr size_t kGs216LdsMax = 150 * 1024;
constexpr int gs216_region_tiles(int pt, int wo) { return (32 * pt + wo + 1 + 31) / 32; }
constexpr size_t gs216_lds_bytes(int wc, int pt, int wo) {
  return 2 * 4 * (size_t)gs216_region_tiles(pt, wo) * 32 * (32 * wc + 16) + (size_t)(32 * wc) * 5 * sizeof(float);
}
// the panels are K2g2's, so the widest plane is: both default instantiations must fit
static_assert(gs216_lds_bytes(2, 2, (FQ_GCONV3X3_S2_C16_MAX_W + 1) / 2) <= kGs216LdsMax &&
              gs216_lds_bytes(1, 4, (FQ_GCONV3X3_S2_C16_MAX_W + 1) / 2) <= kGs216LdsMax,
              "FQ_GCONV3X3_S2_C16_MAX_W does not follow from the LDS budget");

// two neighbouring fp32 values with one buffer_load_dwordx2 (as ONE 64-bit integer: the halves are taken by shifts)
__device__ __forceinline__ uint64_t gs216_ld_b64(fq_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}

template <int WC, int PT, int NW, bool IN16, bool OUT16>
__global__ __launch_bounds__(NW * 64, 2) void gconv3x3_s2_c16_kernel(
    const void* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, void* __restrict__ y, GS216Geom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out, const float* __restrict__ out_thr) {
  constexpr int WP = NW / WC, PTW = PT / WP, NCH = WC * 32, KTS = 10, BPX = 32 * PT;
  static_assert(PTW >= 1 && PTW * WP == PT, "every wavefront owns whole pixel tiles");
  constexpr int UF = NW == 8 ? 3 : (PT == 4 && WC == 2 ? 6 : 4);        // IN16: units a wavefront keeps in flight, 8 VGPRs each
  extern __shared__ __attribute__((aligned(16))) unsigned char gs216_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;      // one phase; a set is four of them
  const unsigned set_bytes = 4u * panel_bytes;
  float* c_sxw = reinterpret_cast<float*>(gs216_smem + 2u * set_bytes);
  float* c_bsc = c_sxw + NCH;
  float* c_bsh = c_bsc + NCH;
  float* c_bias = c_bsh + NCH;
  int* c_zs = reinterpret_cast<int*>(c_bias + NCH);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HWo = (unsigned)g.HWo, Wo = (unsigned)g.Wo, cols = (unsigned)g.cols;
  const unsigned plane4i = (unsigned)g.HWi * 4u, plane16i = (unsigned)g.HWi * 16u, plane4o = HWo * 4u, plane16o = HWo * 16u;
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
  const int64_t x_samp = IN16 ? (int64_t)g.CB * plane16i : (int64_t)g.C * plane4i;
  const int64_t y_samp = OUT16 ? (int64_t)g.CB * plane16o : (int64_t)g.C * plane4o;
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
    r.xr = make_rsrc(reinterpret_cast<const char*>(x) + r.n_base * x_samp, (n_samp - r.n_base) * x_samp);
    return r;
  };
  // (an even-row panel is read at the shifts 0 and -1 only: its tiles in front of position Wo are never looked at)
  auto unit_ok = [&](int u) __attribute__((always_inline)) {
    const int us = u >> 1, rt = us / WC;
    return u < NU && slab0 + (us - rt * WC) < g.NSLAB && ((u & 1) || rt * 32 + 31 >= (int)Wo);
  };
  // the lane's input pixel (ih, 2 cc) of sample nr for unit u: row H of an odd plane does not exist - its neighbour
  auto unit_pixel = [&](const Region& r, int u, unsigned& nr, unsigned& ih, unsigned& cc) __attribute__((always_inline)) {
    int jr = r.jr0 + ((u >> 1) / WC) * 32 + pl;
    jr = jr < 0 ? 0 : (jr < (int)cols ? jr : (int)cols - 1);            // outside the tensor: any valid position (masked later)
    nr = (unsigned)jr / HWo;
    const unsigned rem = (unsigned)jr - nr * HWo, rr = rem / Wo;
    cc = rem - rr * Wo;
    ih = 2u * rr + (unsigned)(u & 1);
    ih = ih < (unsigned)g.H ? ih : (unsigned)g.H - 1u;
  };
  auto set_row = [&](unsigned char* set, int u) __attribute__((always_inline)) {
    const int pr = u & 1, us = u >> 1, rt = us / WC, s = us - rt * WC;
    return set + (unsigned)(2 * pr) * panel_bytes + (size_t)(rt * 32 + pl) * g.ROW + s * 32 + 16 * h;
  };
  // IN16: round k0 of a wavefront's units, wave + NW (k0 + k): the two column phases of block 2 slab + h, 16 bytes each
  v4i ub[IN16 ? UF : 1][2];
  auto issue16 = [&](const Region& r, int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < UF; ++k) {
      const int u = wave + NW * (k0 + k);
      if (unit_ok(u)) {
        unsigned nr, ih, cc;
        unit_pixel(r, u, nr, ih, cc);
        const unsigned xo = ((nr - r.n_base) * (unsigned)g.CB + (unsigned)h) * plane16i + (ih * (unsigned)g.W + 2u * cc) * 16u;
        const unsigned so = (unsigned)(2 * (slab0 + (u >> 1) % WC)) * plane16i;
        ub[k][0] = buf_ld_v4i(r.xr, xo, so);
        ub[k][1] = buf_ld_v4i(r.xr, xo + (2u * cc + 1u < (unsigned)g.W ? 16u : 0u), so);      // column W of an odd row: its neighbour
      }
    }
  };
  auto write16 = [&](unsigned char* set, int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < UF; ++k) {
      const int u = wave + NW * (k0 + k);
      if (unit_ok(u)) {
        unsigned char* row = set_row(set, u);
        *reinterpret_cast<v4i*>(row) = ub[k][0];
        *reinterpret_cast<v4i*>(row + panel_bytes) = ub[k][1];
      }
    }
  };
  const int rounds = (NU + NW * UF - 1) / (NW * UF);                    // (one at every ResNeXt plane)
  // fp32 in: K2g2's unit - sixteen channels, both column phases (one 8-byte load per channel when W is even), quantised
  auto issue32 = [&](const Region& r, int u, float (&v)[2][16]) __attribute__((always_inline)) {
    unsigned nr, ih, cc;
    unit_pixel(r, u, nr, ih, cc);
    const int s = (u >> 1) % WC;
    const unsigned xo = ((nr - r.n_base) * (unsigned)g.C + 16u * h) * plane4i + (ih * (unsigned)g.W + 2u * cc) * 4u;
    if (evenw) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint64_t t = gs216_ld_b64(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
        v[0][i] = __builtin_bit_cast(float, (unsigned)t);
        v[1][i] = __builtin_bit_cast(float, (unsigned)(t >> 32));
      }
    } else {
      const unsigned xo1 = xo + (2u * cc + 1u < (unsigned)g.W ? 4u : 0u);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        v[0][i] = buf_ld_f32(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
        v[1][i] = buf_ld_f32(r.xr, xo1, (unsigned)(ch0 + s * 32 + i) * plane4i);
      }
    }
  };
  float bufa[2][IN16 ? 1 : 16], bufb[2][IN16 ? 1 : 16];
  const ThresholdReq treq = threshold_request(in_stat, n, in_thr, item == 0);   // first in the memory queue (fq_common.h)
  FQ_PIN();
  Region rg = region_of(blk0);
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
  auto quant_to_set = [&](unsigned char* set, int u, const float (&v)[2][IN16 ? 1 : 16]) __attribute__((always_inline)) {
    if constexpr (!IN16) {
      unsigned char* row = set_row(set, u);
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
    }
  };
  // IN16: a region's rounds from k0 on, of which round `flying` is in flight already - the first region whole (nothing to hide it
  // under), of the later ones what the burst under the taps did not take
  auto fill16 = [&](const Region& r, unsigned char* set, int k0, int flying) __attribute__((always_inline)) {
    for (int k = k0; k < rounds * UF; k += UF) {
      if (k != flying) issue16(r, k);
      FQ_PIN();
      write16(set, k);
      FQ_PIN();
    }
  };
  if constexpr (IN16) {
    fill16(rg, gs216_smem, 0, 0);
  } else {
    for (int u = wave; u < NU; u += 2 * NW) {                           // the first region, two units in flight
      if (unit_ok(u + NW)) issue32(rg, u + NW, bufb);
      FQ_PIN();
      if (unit_ok(u)) quant_to_set(gs216_smem, u, bufa);
      FQ_PIN();
      if (unit_ok(u + 2 * NW)) issue32(rg, u + 2 * NW, bufa);
      FQ_PIN();
      if (unit_ok(u + NW)) quant_to_set(gs216_smem, u + NW, bufb);
      FQ_PIN();
    }
  }

  // ---- this wavefront's slab: nine A fragments, resident for the whole band ------------------------------------------------------
  const int wc = wave % WC, wp = wave / WC;
  const int slab = slab0 + wc;
  const bool mine = slab < g.NSLAB;                                     // (a slab group wider than the layer: this wavefront
                                                                        // only helps to fill)
  const fq_rsrc wr = make_rsrc(wfrag + (((int64_t)slab * KTS) << 10), mine ? 9 * 1024 : 0);
  v4i afrag[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) afrag[tap] = buf_ld_v4i(wr, (unsigned)lane * 16u, (unsigned)(tap << 10));
  const int zb = stored_zero4(ubias);                                   // four codes "0" in the stored representation
  const float* fbias = bias;
  // the consumer's quantiser of a C16 output (fq_mma.h)
  const QParams q2 = mma_out_qparams<OUT16, false>(out_thr, nullptr, g.out_levels, g.out_lo_neg, eps);
  const int ubias2 = 128 - g.out_zoff;
  FQ_PIN();
  __syncthreads();                                                      // first set, constants, statistic table

  for (unsigned blk = blk0; blk < blk1; ++blk) {
    const unsigned cur = (blk - blk0) & 1u;
    const unsigned char* set = gs216_smem + cur * set_bytes;
    unsigned char* other = gs216_smem + (cur ^ 1u) * set_bytes;
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
    // IN16: the wavefront's first round of the NEXT region is in flight under the taps and lands behind the sixth;
    // fp32: unit k of this wavefront (wave + NW k) rides under tap k, loaded a tap ahead, quantised behind the MFMAs
    if constexpr (IN16) {
      if (has_next) issue16(nx, 0);
    } else {
      if (has_next && unit_ok(wave)) issue32(nx, wave, bufa);
    }
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
      if constexpr (IN16) {
        if (tap == 5 && has_next) {
          write16(other, 0);
          FQ_PIN();
        }
      } else {
        if (has_next) {
          const int u = wave + NW * tap;
          if (tap < 8 && unit_ok(u + NW)) issue32(nx, u + NW, (tap & 1) ? bufa : bufb);
          FQ_PIN();
          if (unit_ok(u)) quant_to_set(other, u, (tap & 1) ? bufb : bufa);
          FQ_PIN();
        }
      }
    }
    if (has_next) {
      if constexpr (IN16) {
        fill16(nx, other, UF, -1);                                      // (the further rounds of a wide plane's region)
      } else {
        for (int u = wave + NW * 9; u < NU; u += NW) {                  // (a region of more than 36 units: the rest, plainly)
          if (unit_ok(u)) {
            issue32(nx, u, bufa);
            quant_to_set(other, u, bufa);
          }
        }
      }
    }
    FQ_PIN();
    __syncthreads();                                  // the next set is whole; every wavefront is done reading this one
    if (has_next) rg = nx;
    if (!mine) continue;
    // ---- epilogue: lane = output pixel; a window (mma_out_rsrc) from this wavefront's slab on - OUT16: from its first block on --
    const int64_t skip = OUT16 ? (int64_t)(2 * slab) * plane16o : (int64_t)slab * 32 * plane4o;
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
        const unsigned yo = ((smp[t] - s_base) * (unsigned)g.C + 4u * h) * plane4o + pp[t] * 4u;
        float m = 0.0f;
        int packed[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          FQ_PIN();                                  // (eight channels' constants at a time, as K2gc: hoisted they cost registers)
          const int c0 = cb + 8 * gq;
          const v4i zs = *reinterpret_cast<const v4i*>(c_zs + c0);
          const f4 sxw = *reinterpret_cast<const f4*>(c_sxw + c0);
          const f4 bsc = *reinterpret_cast<const f4*>(c_bsc + c0);
          const f4 bsh = *reinterpret_cast<const f4*>(c_bsh + c0);
          f4 bch = (f4){0.f, 0.f, 0.f, 0.f};
          if (BIAS_M == 1 || (BIAS_M < 0 && fbias != nullptr)) bch = *reinterpret_cast<const f4*>(c_bias + c0);
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
            if constexpr (!OUT16) buf_st_f32(yr, yo, (unsigned)(8 * gq + r) * plane4o, v);
            m = FOLD ? fmaxf(m, v) : fmaxf(m, fabsf(v));
          }
          if constexpr (OUT16) {
            FQ_PIN();
            packed[gq] = fq_pack4<NN2>(vq[0], vq[1], vq[2], vq[3], qc, ubias2, fq_nonneg_xor(ubias2));
            asm volatile("" : "+v"(packed[gq]));
          }
        }
        if constexpr (OUT16) {
          // lane l <-> lane l + 32: half 0 keeps (gq 0, gq 1) of both halves = block 2 slab, half 1 gets (gq 2, gq 3) = block
          // 2 slab + 1; dword order inside a block: channels 4 h' + 8 (gq & 1)
          const unsigned yo16 = (smp[t] - s_base) * (unsigned)g.CB * plane16o + pp[t] * 16u;
          const auto s01 = __builtin_amdgcn_permlane32_swap((unsigned)packed[0], (unsigned)packed[2], false, false);
          const auto s23 = __builtin_amdgcn_permlane32_swap((unsigned)packed[1], (unsigned)packed[3], false, false);
          const f4 o = (f4){__uint_as_float(s01[0]), __uint_as_float(s01[1]), __uint_as_float(s23[0]), __uint_as_float(s23[1])};
          buf_st_v4f(yr, yo16 + (unsigned)h * plane16o, 0, o);
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

struct Gs216Call {
  const void* x; const int8_t* wfrag; const float* wscale; const int32_t* wsum; const float* bias; void* y;
  const float* in_stat; int n; const float* in_thr; float levels; int lo_neg; float* out_current_max;
  const float* bn_scale; const float* bn_shift; int act; float* stat_out; const float* out_thr; int cg;
};

template <int WC, int PT, int NW, bool IN16, bool OUT16>
int gconv3x3_s2_c16_go(const Gs216Call& a, const GS216Geom& g, int64_t grid, size_t lds, hipStream_t st) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&gconv3x3_s2_c16_kernel<WC, PT, NW, IN16, OUT16>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGs216LdsMax) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_gconv3x3_s2_i8_c16: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((gconv3x3_s2_c16_kernel<WC, PT, NW, IN16, OUT16>), dim3((unsigned)grid), dim3(NW * 64), lds, st, a.x, a.wfrag,
                     a.wscale, (const int*)a.wsum, a.bias, a.y, g, a.in_stat, a.n, a.in_thr, a.levels, a.lo_neg, kEps,
                     a.out_current_max, a.bn_scale, a.bn_shift, a.act, a.stat_out, a.out_thr);
  note_launch(FQ_KERNEL_GCONV3X3, FQ_LAUNCH_GCONV3X3S2_C16, {WC, PT, g.NB, a.cg, IN16 ? 1 : 0, OUT16 ? 1 : 0, NW});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

// three io forms of the default split; the larger blocks are built for codes on both sides, the form the ResNeXt units run
template <int WC, int PT, int NW>
int gconv3x3_s2_c16_io(const Gs216Call& a, const GS216Geom& g, bool in16, bool out16, int64_t grid, size_t lds, hipStream_t st) {
  if (in16 && out16) return gconv3x3_s2_c16_go<WC, PT, NW, true, true>(a, g, grid, lds, st);
  if (in16) return gconv3x3_s2_c16_go<WC, PT, NW, true, false>(a, g, grid, lds, st);
  return gconv3x3_s2_c16_go<WC, PT, NW, false, true>(a, g, grid, lds, st);
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_gconv3x3_s2_i8_c16(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                          const float* bias, void* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w,
                          const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                          const float* bn_scale, const float* bn_shift, int act, float* stat_out, const float* out_thr,
                          int out_width, unsigned out_flags, fqStream_t stream) {
  const bool in16 = x_is_c16 != 0, out16 = out_thr != nullptr;
  FQ_REQUIRE(x && wcodes && wscale && wsum && y, "fq_gconv3x3_s2_i8_c16: null pointer");
  FQ_REQUIRE(in16 || out16, "fq_gconv3x3_s2_i8_c16: neither side is a C16 tensor (use fq_gconv3x3_s2_i8)");
  FQ_REQUIRE(!in16 || in_thr != nullptr, "fq_gconv3x3_s2_i8_c16: a C16 input was quantised with a stored threshold: give in_thr");
  const int64_t ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && n * ho * wo < (1ll << 31) - 4096, "fq_gconv3x3_s2_i8_c16: bad shape");
  FQ_REQUIRE(fq_gconv3x3_s2_i8_supported(c, c, groups), "fq_gconv3x3_s2_i8_c16: %lld channels in %lld groups: the channel count "
             "must be a multiple of 32 and a group 4, 8, 16 or 32 channels wide", (long long)c, (long long)groups);
  FQ_REQUIRE(w <= FQ_GCONV3X3_S2_C16_MAX_W, "fq_gconv3x3_s2_i8_c16: planes up to %d pixels wide (got %lld)",
             FQ_GCONV3X3_S2_C16_MAX_W, (long long)w);
  FQ_REQUIRE(in_stat != nullptr || in_thr != nullptr, "fq_gconv3x3_s2_i8_c16: give in_stat (online), in_thr (offline) or both "
             "(offline, the statistic only feeds out_current_max)");
  FQ_REQUIRE(in_thr != nullptr || out_current_max != nullptr, "fq_gconv3x3_s2_i8_c16: online mode needs out_current_max");
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "fq_gconv3x3_s2_i8_c16: input width %d does not fit int8 codes", in_width);
  FQ_REQUIRE(!(in_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_gconv3x3_s2_i8_c16: unsupported activation flags");
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_gconv3x3_s2_i8_c16: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_gconv3x3_s2_i8_c16: unknown activation %d", act);
  FQ_REQUIRE(aligned16(wcodes) && aligned16(x) && aligned16(y), "fq_gconv3x3_s2_i8_c16: x, y and wcodes must be 16-byte aligned");
  const int64_t hwi = h * w, hwo = ho * wo, cols = n * hwo;
  const int nslab = (int)(c / 32);
  const int wc = nslab >= 2 ? 2 : 1;
  // the block and the wavefronts that share it: see the kernel's comment.  One slab: four tiles, one per wavefront.  Two slabs:
  // two tiles (K2g2's split) unless FQ_GCS216_CFG (tuning, read per call; codes on both sides, where the two sets still fit LDS)
  // names <tiles><wavefronts> = 44 or 48
  int pt = wc == 2 ? 2 : 4, nw = 4;
  const int cfg = env_int("FQ_GCS216_CFG", 0);
  if (wc == 2 && in16 && out16 && (cfg == 44 || cfg == 48) && gs216_lds_bytes(wc, 4, (int)wo) <= kGs216LdsMax) {
    pt = 4;
    nw = cfg % 10;
  }
  const int blockpx = 32 * pt;
  // 32-bit lane offsets count from the first sample a block's region (input, blockpx + wo + 1 output positions) or the block
  // itself (output) touches
  FQ_REQUIRE(((blockpx + wo + 1) / hwo + 2) * c * hwi * (in16 ? 1 : 4) < (1ll << 31) &&
                 (blockpx / hwo + 2) * c * hwo * (out16 ? 1 : 4) < (1ll << 31),
             "fq_gconv3x3_s2_i8_c16: a pixel block and its halo must stay within 2 GiB of their first sample");
  hipStream_t st = (hipStream_t)stream;
  const int64_t row_pad = 320, rows_pad = (c + 63) / 64 * 64;            // fq_weight_codes' buffer of the (C, 3, 3, 32) filter
  GS216Geom g;
  g.C = (int)c; g.H = (int)h; g.W = (int)w; g.HWi = (int)hwi;
  g.Ho = (int)ho; g.Wo = (int)wo; g.HWo = (int)hwo;
  g.NSLAB = nslab; g.CS = (nslab + wc - 1) / wc;
  g.cols = cols; g.nblocks = (cols + blockpx - 1) / blockpx;
  // the band, as K2g2: four blocks per workgroup while that leaves two workgroups per compute unit, else two - never one
  // (FQ_GCS216_NB: tuning, read per call)
  int nb = 4;
  if (((g.nblocks + nb - 1) / nb) * g.CS < 2 * (int64_t)num_cu()) nb = 2;
  const int tune = env_int("FQ_GCS216_NB", 0);
  if (tune >= 1 && tune <= 64) nb = tune;
  g.NB = nb;
  g.items = ((g.nblocks + nb - 1) / nb) * g.CS;
  g.RT = gs216_region_tiles(pt, (int)wo); g.ROW = 32 * wc + 16;
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  g.evenw = w % 2 == 0 ? 1 : 0;                                           // (x is 16-byte aligned: every pair of columns 8-byte)
  g.CB = (int)(c / 16);
  g.out_levels = 0.0f; g.out_lo_neg = 0; g.out_zoff = 0;
  if (out16) {
    FQ_REQUIRE(out_width >= 2 && out_width <= 8, "fq_gconv3x3_s2_i8_c16: output width %d does not fit int8 codes", out_width);
    FQ_REQUIRE(!(out_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_gconv3x3_s2_i8_c16: unsupported output flags");
    g.out_levels = act_levels(out_width, out_flags);
    g.out_lo_neg = (out_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
    g.out_zoff = (out_flags & FQ_ACT_SIGNED) ? 0 : 128;
  }
  const int64_t grid = (g.items + 7) / 8 * 8;
  FQ_REQUIRE(grid < (1ll << 31), "fq_gconv3x3_s2_i8_c16: too many pixel blocks");
  const size_t lds = gs216_lds_bytes(wc, pt, (int)wo);
  FQ_REQUIRE(lds <= kGs216LdsMax, "fq_gconv3x3_s2_i8_c16: two region sets of %d positions x %d channels do not fit LDS (planes up "
             "to %d wide)", blockpx + (int)wo + 1, 32 * wc, FQ_GCONV3X3_S2_C16_MAX_W);
  Gs216Call a;
  a.x = x; a.wfrag = wcodes + rows_pad * row_pad;                         // the fragment-major copy
  a.wscale = wscale; a.wsum = wsum; a.bias = bias; a.y = y;
  a.in_stat = in_stat; a.n = (int)n; a.in_thr = in_thr;
  a.levels = act_levels(in_width, in_flags);
  a.lo_neg = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  a.out_current_max = out_current_max; a.bn_scale = bn_scale; a.bn_shift = bn_shift; a.act = act; a.stat_out = stat_out;
  a.out_thr = out_thr; a.cg = (int)(c / groups);
  if (stat_out && !prezeroed) {                                           // (a kernel, not a memset node: safe under graph capture)
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stat_out, n, 0.0f);
    FQ_LAUNCH_CHECK();
  }
  const double ci = (double)n * c * hwi, co = (double)n * c * hwo;
  ProfScope prof(FQ_KERNEL_GCONV3X3, 4.0 * (ci + co), st, (in16 ? 1.0 : 4.0) * ci + (out16 ? 1.0 : 4.0) * co);
  if (wc == 1) return gconv3x3_s2_c16_io<1, 4, 4>(a, g, in16, out16, grid, lds, st);
  if (pt == 4 && nw == 8) return gconv3x3_s2_c16_go<2, 4, 8, true, true>(a, g, grid, lds, st);
  if (pt == 4) return gconv3x3_s2_c16_go<2, 4, 4, true, true>(a, g, grid, lds, st);
  return gconv3x3_s2_c16_io<2, 2, 4>(a, g, in16, out16, grid, lds, st);
}

}  // extern "C"
