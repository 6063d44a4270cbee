// libfakequant — K2g2c grouped 3x3 convolution with STRIDE 2 (pad 1, 4 .. 32 channels per group) between C16 code tensors
// (fq_gconv3x3_s2_i8_c16): the three layers that open stages 2, 3 and 4 of the ResNeXt nets under stored thresholds
// (see fq_common.h for the list of translation units and the design rules; the fp32 -> fp32 form: fq_gconv3x3_s2.hip; what the
// four grouped kernels share: fq_gconv.h)
#include "fq_gconv.h"

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
template <int WC, int PT, int NW, bool IN16, bool OUT16>
__global__ __launch_bounds__(NW * 64, 2) void gconv3x3_s2_c16_kernel(
    const void* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, void* __restrict__ y, GcGeom g,
    const float* __restrict__ in_stat, int n, const float* __restrict__ in_thr, float levels, int lo_neg_max, float eps,
    float* __restrict__ cur_max_out, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act,
    float* __restrict__ stat_out, const float* __restrict__ out_thr) {
  constexpr int WP = NW / WC, PTW = PT / WP, NCH = WC * 32, BPX = 32 * PT;
  static_assert(PTW >= 1 && PTW * WP == PT, "every wavefront owns whole pixel tiles");
  constexpr int UF = NW == 8 ? 3 : (PT == 4 && WC == 2 ? 6 : 4);        // IN16: units a wavefront keeps in flight, 8 VGPRs each
  extern __shared__ __attribute__((aligned(16))) unsigned char gs216_smem[];
  __shared__ unsigned k_stat[kStatSlots];
  const unsigned panel_bytes = (unsigned)g.RT * 32u * (unsigned)g.ROW;      // one phase; a set is four of them
  const unsigned set_bytes = 4u * panel_bytes;
  const GcTables ct = gc_tables<NCH>(gs216_smem + 2u * set_bytes);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, pl = lane & 31;
  const unsigned HWo = (unsigned)g.HWo, Wo = (unsigned)g.Wo, cols = (unsigned)g.cols;
  const unsigned plane4i = (unsigned)g.HW * 4u, plane16i = (unsigned)g.HW * 16u, plane4o = HWo * 4u, plane16o = HWo * 16u;
  const bool has_bn = bn_scale != nullptr, has_stat = stat_out != nullptr;
  const bool evenw = g.evenw != 0;
  unsigned item, blk0, blk1, s_band;
  int slab0, ch0;
  if (!mma_xcd_item(g.items, item)) return;
  gc_work_item<WC, BPX>(g, HWo, item, slab0, ch0, blk0, blk1, s_band);
  const int64_t x_samp = IN16 ? (int64_t)g.CB * plane16i : (int64_t)g.C * plane4i;
  const int64_t y_samp = OUT16 ? (int64_t)g.CB * plane16o : (int64_t)g.C * plane4o;
  const int64_t n_samp = (int64_t)(cols / HWo);

  // ---- a block's region -> a set of four panels: units of (region tile, slab, row parity), wave-strided -------------------------
  const int NU = g.RT * WC * 2;
  auto region_of = [&](unsigned blk) __attribute__((always_inline)) { return gc_region_of(x, blk, BPX, Wo, HWo, x_samp, n_samp); };
  // (an even-row panel is read at the shifts 0 and -1 only: its tiles in front of position Wo are never looked at)
  auto unit_ok = [&](int u) __attribute__((always_inline)) {
    const int us = u >> 1, rt = us / WC;
    return u < NU && slab0 + (us - rt * WC) < g.NSLAB && ((u & 1) || rt * 32 + 31 >= (int)Wo);
  };
  // the lane's input pixel (ih, 2 cc) of sample nr for unit u: row H of an odd plane does not exist - its neighbour
  auto unit_pixel = [&](const GcRegion& r, int u, unsigned& nr, unsigned& ih, unsigned& cc) __attribute__((always_inline)) {
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
  auto issue16 = [&](const GcRegion& r, int k0) __attribute__((always_inline)) {
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
  auto issue32 = [&](const GcRegion& r, int u, float (&v)[2][16]) __attribute__((always_inline)) {
    unsigned nr, ih, cc;
    unit_pixel(r, u, nr, ih, cc);
    const int s = (u >> 1) % WC;
    const unsigned xo = ((nr - r.n_base) * (unsigned)g.C + 16u * h) * plane4i + (ih * (unsigned)g.W + 2u * cc) * 4u;
    if (evenw) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint64_t t = gc_ld_b64(r.xr, xo, (unsigned)(ch0 + s * 32 + i) * plane4i);
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
  auto quant_to_set = [&](unsigned char* set, int u, const float (&v)[2][IN16 ? 1 : 16]) __attribute__((always_inline)) {
    if constexpr (!IN16) {
      unsigned char* row = set_row(set, u);
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) *reinterpret_cast<v4i*>(row + (unsigned)pc * panel_bytes) = gc_quant16(v[pc], nonneg, q, ubias, nn_xor);
    }
  };
  // IN16: a region's rounds from k0 on, of which round `flying` is in flight already - the first region whole (nothing to hide it
  // under), of the later ones what the burst under the taps did not take
  auto fill16 = [&](const GcRegion& r, unsigned char* set, int k0, int flying) __attribute__((always_inline)) {
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
  v4i afrag[9];
  gc_load_afrag(wfrag, slab, mine, lane, afrag);
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
        for (int t = 0; t < PTW; ++t)
          gc_mma_tap(set + phase + (unsigned)((int)rbase[t] + shift), (tapmask[t] >> tap) & 1u, zb, afrag[tap], acc[t]);
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

constexpr GcEntry kGs216Entry = {"fq_gconv3x3_s2_i8_c16", nullptr, 2, FQ_GCONV3X3_S2_C16_MAX_W, true};

// the panels are K2g2's, so the widest plane is: both default instantiations must fit
static_assert(gc_lds_bytes(2, 2, 2, (FQ_GCONV3X3_S2_C16_MAX_W + 1) / 2) <= kGcLdsMax &&
              gc_lds_bytes(2, 1, 4, (FQ_GCONV3X3_S2_C16_MAX_W + 1) / 2) <= kGcLdsMax,
              "FQ_GCONV3X3_S2_C16_MAX_W does not follow from the LDS budget");

template <int WC, int PT, int NW, bool IN16, bool OUT16>
int gconv3x3_s2_c16_go(const GcCall& a, const GcGeom& g, int64_t grid, size_t lds, hipStream_t st) {
  return gc_launch<&gconv3x3_s2_c16_kernel<WC, PT, NW, IN16, OUT16>>(kGs216Entry.name, NW * 64, FQ_LAUNCH_GCONV3X3S2_C16,
                                                                     {WC, PT, g.NB, a.cg, IN16 ? 1 : 0, OUT16 ? 1 : 0, NW}, a, g, grid,
                                                                     lds, st);
}

// three io forms of the default split; the larger blocks are built for codes on both sides, the form the ResNeXt units run
template <int WC, int PT, int NW>
int gconv3x3_s2_c16_io(const GcCall& a, const GcGeom& g, bool in16, bool out16, int64_t grid, size_t lds, hipStream_t st) {
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
  GcCall a = {x, nullptr, wscale, wsum, bias, y, in_stat, 0, in_thr, 0.0f, 0, out_current_max, bn_scale, bn_shift, act, stat_out,
              out_thr, 0};
  bool prezeroed;
  if (int rc = gc_check(kGs216Entry, a, wcodes, n, c, groups, h, w, in_width, in_flags, prezeroed)) return rc;
  FQ_REQUIRE(in16 || out16, "fq_gconv3x3_s2_i8_c16: neither side is a C16 tensor (use fq_gconv3x3_s2_i8)");
  FQ_REQUIRE(!in16 || in_thr != nullptr, "fq_gconv3x3_s2_i8_c16: a C16 input was quantised with a stored threshold: give in_thr");
  const int wc = gc_slabs_per_group(c), wo = (int)((w - 1) / 2 + 1);
  // the block and the wavefronts that share it: see the kernel's comment.  One slab: four tiles, one per wavefront.  Two slabs:
  // two tiles (K2g2's split) unless FQ_GCS216_CFG (tuning, read per call; codes on both sides, where the two sets still fit LDS)
  // names <tiles><wavefronts> = 44 or 48
  int pt = wc == 2 ? 2 : 4, nw = 4;
  const int cfg = env_int("FQ_GCS216_CFG", 0);
  if (wc == 2 && in16 && out16 && (cfg == 44 || cfg == 48) && gc_lds_bytes(2, wc, 4, wo) <= kGcLdsMax) {
    pt = 4;
    nw = cfg % 10;
  }
  GcGeom g;
  int64_t grid;
  size_t lds;
  // the band, as K2g2: four blocks, else two (FQ_GCS216_NB: tuning, read per call)
  if (int rc = gc_plan(kGs216Entry, a, wcodes, n, c, h, w, in_flags, pt, 4, env_int("FQ_GCS216_NB", 0), in16 ? 1 : 4, out16 ? 1 : 4, g,
                       grid, lds))
    return rc;
  if (int rc = gc_out_quant(kGs216Entry, out16, out_width, out_flags, g)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gc_zero_stat(stat_out, prezeroed, n, st)) return rc;
  const double ci = (double)n * c * g.HW, co = (double)n * c * g.HWo;
  ProfScope prof(FQ_KERNEL_GCONV3X3, 4.0 * (ci + co), st, (in16 ? 1.0 : 4.0) * ci + (out16 ? 1.0 : 4.0) * co);
  if (wc == 1) return gconv3x3_s2_c16_io<1, 4, 4>(a, g, in16, out16, grid, lds, st);
  if (pt == 4 && nw == 8) return gconv3x3_s2_c16_go<2, 4, 8, true, true>(a, g, grid, lds, st);
  if (pt == 4) return gconv3x3_s2_c16_go<2, 4, 4, true, true>(a, g, grid, lds, st);
  return gconv3x3_s2_c16_io<2, 2, 4>(a, g, in16, out16, grid, lds, st);
}

}  // extern "C"
