// libfakequant — K2z: the statistic-only pass of a pointwise (1x1) convolution on int8 codes, the first half of a recompute pair
// (see fq_common.h for the list of translation units and the design rules; what it shares with fq_pwdw.hip: fq_pair.h)
//
// fq_pwconv_i8_stat: stat_out[n] <- max |act(BN(conv))| over the sample, nothing else leaves the chip.  The operand roles of
// fq_pwdw.hip (activations are the A operand: lane = output channel, registers = 16 pixels of a 32-pixel tile), and ONE more
// observation: every step of the epilogue - int32 -> fp32, * sx*sw, + bias, * bn_scale, + bn_shift,
// the activation - is a monotone function of the integer sum (rounding is monotone, a negative factor only turns the order
// round), so the maximum of |act(BN(.))| over a set of pixels is attained at the largest or the smallest INTEGER sum of the
// channel.  The kernel therefore keeps, per channel and sample, max and min of the int32 sums (v_max3 / v_min3: one
// instruction per output value instead of the storing kernel's six) and runs the fp32 epilogue on those two only, once per
// sample: bit for bit the statistic of fq_pwconv_i8.  That turns the pass from instruction-bound (3.5 TB/s as the storing
// kernel without its stores) into a read of x.
// x_codes_out (optional): the codes of x do exist once this pass has quantised them - lane (i32, h) holds, per slab kt, the 16
// codes of ITS pixel's channels 32 kt + 16 h .. + 15 as the bytes of an MFMA A fragment, which is a C16 vector (fakequant.h).  The
// lane stores it at [smp][2 kt + h][p][16]: fq_pwdw_fused's lane of the same pixel and slab loads it back with one instruction
// instead of sixteen loads and sixteen quantisations.  The 32 lanes of a half write 512 contiguous bytes per instruction; the
// lanes of a partial last tile, clamped to the last pixel, rewrite that pixel's own bytes.
#include "fq_dw.h"
#include "fq_pair.h"

namespace {

__device__ __forceinline__ void buf_st_v4i(fq_rsrc r, unsigned voff, v4i v) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, (int)voff, 0, 0);
  asm volatile("s_nop 1" : : "v"(v));
}

struct PwStatGeom {
  int Cin, KTS, Cout, CT, HW;
  int64_t cols, tiles;
  int zoff;
  int table;                 // 1: per-sample maxima through the workgroup's LDS table (few tiles per wavefront)
  FastDiv hw;
};

// FRONT (FEPI >= 0; fq_pwconv_i8_stat with a front layer): x is the output of a stride-1 depthwise 3x3 that was never stored.
// Its INPUT arrives as planar int8 codes (fq_dwconv3x3's statistic pass kept them), and a workgroup recomputes x band by band:
//   1  stencil, lane = (channel, four columns) as in fq_dwconv3x3's four-columns form (that is how the planar codes lie: one
//      dword per lane and row, the horizontal neighbours by DPP from the adjacent lanes - a row of the plane is W / 4 <= 64
//      lanes, so the plane's edge is the segment's edge and takes 0): dequantise (code * scale, once per element and band),
//      the row-major fmaf chain, the layer's epilogue (kEpi* as there) - bit for bit what that kernel stores - then THIS
//      launch's quantiser (the threshold is known: the depthwise pass left its statistic), and the code byte goes to an LDS
//      band buffer of four-channel planes (fq_front_layout.h: the order in which no store and no read meets a bank conflict).
//      The transposition planar -> C16 happens here, on LDS bytes;
//   2  the band buffer is read back as MFMA A fragments (four dword LDS reads per lane, slab and 32-pixel tile: the 16 channels
//      32 kt + 16 h .. + 15 of the lane's pixel are planes 8 kt + 4 h .. + 3) and everything from there on is the kernel's own:
//      the fragment leaves as x_codes_out (block 2 kt + h), max / min of the int32 sums, flush per sample.
// A band is R <= kFrontRows output rows of one sample (all channels, whole rows): R + 2 input rows are dequantised for it
// (front_rows_pick chooses R).  FSIGNED: the input codes are two's complement bytes (FQ_ACT_SIGNED), else 0 .. 255.
struct PwFrontArgs {
  const int8_t* codes;               // [n][Cin][H * W]
  const float *w, *bias, *bn_scale, *bn_shift;
  const float *in_stat, *in_thr;     // the depthwise layer's input quantiser
  float levels;
  int act;
  int H, W, Q, segs, R, bands;       // Q = W / 4 lanes per row, `segs` rows (channels) per wavefront, R output rows per band
  FrontLayout lay;                   // the band buffer's strides for (Q, R)
};

// NW: wavefronts of the workgroup - kBlock / 64 = 4, or (FRONT only) 8 on the same band where the band buffer leaves a CU too few
// workgroups of four to fill its SIMDs (front_waves_pick).  Every wavefront has its own max / min table.
template <int KT, int FEPI = -1, bool FSIGNED = false, int NW = kFrontWaves>
__global__ __launch_bounds__(64 * NW, NW == kFrontWaves ? 3 : 2) void pw_stat_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias, PwStatGeom g, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels, int lo_neg, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out,
    int8_t* __restrict__ x_codes_out, PwFrontArgs fa) {
  constexpr bool FRONT = FEPI >= 0;
  static_assert(!FRONT || KT <= 4, "the front layer is built for up to four 32-channel slabs");
  static_assert(NW * 64 == kBlock || (FRONT && NW == kFrontWavesWide), "four wavefronts; eight only with a front layer");
  constexpr int kThreads = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char pst_smem[];
  v4i* ldsW = reinterpret_cast<v4i*>(pst_smem);                                           // [CT][KT][64]
  int* c_zs = reinterpret_cast<int*>(pst_smem + (size_t)g.CT * KT * 1024);                 // [CT * 32]
  float* c_k = reinterpret_cast<float*>(c_zs + g.CT * 32);                                 // [4][CT * 32]: w scale, bias, BN scale / shift
  int* accs = reinterpret_cast<int*>(c_k + 4 * g.CT * 32);                                 // [NW waves][CT][2][64]
  float* dwk = reinterpret_cast<float*>(accs + NW * g.CT * 128);                            // FRONT: [Cin][12] taps, bias, BN scale / shift
  unsigned char* zbuf = reinterpret_cast<unsigned char*>(dwk + g.Cin * 12);                 // FRONT: [Cin / 4][lay.pl] dwords, band of codes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, i32 = lane & 31;
  const unsigned HW = (unsigned)g.HW, cols = (unsigned)g.cols;
  const int64_t nwaves = (int64_t)gridDim.x * NW, wid = (int64_t)blockIdx.x * NW + wave;
  // the wavefront's 32-pixel tiles - FRONT: the WORKGROUP's bands (band b of sample s is number s * bands + b)
  const int64_t n_bands = FRONT ? (int64_t)(g.cols / g.HW) * fa.bands : 0;
  const int64_t t_begin = FRONT ? n_bands * blockIdx.x / gridDim.x : g.tiles * wid / nwaves;
  const int64_t t_end = FRONT ? n_bands * (blockIdx.x + 1) / gridDim.x : g.tiles * (wid + 1) / nwaves;
  const int pl = mfma_row_pixel(i32);                                     // tile pixel of this lane's MFMA row
  int* my = accs + (size_t)wave * g.CT * 128;
  __shared__ unsigned k_stat[kStatSlots];
  mma_stat_init(k_stat);
  unsigned s_base;                               // first sample of the workgroup's tile range
  if constexpr (FRONT) {
    s_base = (unsigned)((t_begin < n_bands ? t_begin : n_bands - 1) / fa.bands);
  } else {
    const int64_t t0 = g.tiles * ((int64_t)blockIdx.x * NW) / nwaves;
    const unsigned j0 = (unsigned)(t0 < g.tiles ? t0 : g.tiles - 1) * 32u;
    s_base = fast_div(j0 < cols ? j0 : cols - 1, g.hw);
  }

  struct Pix { unsigned smp, p; };
  auto pix_of = [&](int64_t t) __attribute__((always_inline)) {
    unsigned j = (unsigned)t * 32u + (unsigned)pl;
    j = j < cols ? j : cols - 1;                                          // (a copy of the last pixel: changes no maximum)
    Pix r;
    r.smp = fast_div(j, g.hw);
    r.p = j - r.smp * HW;
    return r;
  };
  // slab q of the wave's range = (tile t_begin + q / KT, 32-channel slab q % KT), kept in buffer q % NB; the loads of slab
  // q + NB - 1 leave before slab q is quantised: NB - 1 slabs (4 KB each) in flight per wavefront, three wavefronts per SIMD.  One tile ahead - the first
  // version - left every wavefront waiting a memory latency per tile (3.9 TB/s on the 205 MB tensor of the first pair).
  constexpr int NB = 3;
  const fq_rsrc rs = make_rsrc(x, (int64_t)(cols / HW) * g.Cin * HW * 4);
  auto issue = [&](int64_t t, int kt, float (&v)[16]) __attribute__((always_inline)) {
    if (t >= t_end) return;
    const Pix px = pix_of(t);
    // (a half-slab past Cin: its own offset leaves the buffer's range only in the LAST sample - elsewhere it lands in the next
    // sample's channels - so the lane offset is put out of range outright: the loads return 0, whose code meets zero weight codes)
    const bool ok = kt * 32 + 16 * h < g.Cin;
    const unsigned vo = ok ? (unsigned)(((px.smp * (unsigned)g.Cin + 16u * h) * HW + px.p) * 4u) : 0x80000000u;
    const unsigned so = (unsigned)kt * 32u * HW * 4u;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = buf_ld_f32(rs, vo, so + (unsigned)i * HW * 4u);
  };
  float raw[NB][16];
#pragma unroll
  for (int b2 = 0; b2 < NB; ++b2)
#pragma unroll
    for (int i = 0; i < 16; ++i) raw[b2][i] = 0.0f;
  if constexpr (!FRONT) {
#pragma unroll
    for (int qq = 0; qq < NB - 1; ++qq) issue(t_begin + qq / KT, qq % KT, raw[qq]);
  }
  FQ_PIN();
  // FRONT: the multiply-back scale of the depthwise layer's input quantiser (make_qparams: max_ / levels)
  float fscale = 0.0f;
  if constexpr (FRONT) fscale = input_threshold(fa.in_stat, n, fa.in_thr, nullptr, false) / fa.levels;
  const float max_ = input_threshold(in_stat, n, in_thr, cur_max_out, blockIdx.x == 0);
  const QParams q = make_qparams(max_, levels, lo_neg != 0, eps);
  const int ubias = 128 - g.zoff;
  const unsigned nn_xor = fq_nonneg_xor(ubias);
  const bool wr_codes = x_codes_out != nullptr;
  const fq_rsrc rcodes = make_rsrc(x_codes_out, wr_codes ? (int64_t)(cols / HW) * 2 * KT * HW * 16 : 0);
  for (int idx = threadIdx.x; idx < g.CT * KT * 64; idx += kThreads) {
    const int f = idx >> 6, ct = f / KT, kt = f - ct * KT;
    ldsW[idx] = *reinterpret_cast<const v4i*>(wfrag + (((int64_t)ct * g.KTS + kt) << 10) + ((idx & 63) << 4));
  }
  // (the epilogue's per-channel constants too: read from HBM inside flush() they cost every wavefront a memory latency per
  // channel tile and sample - a fixed 6-25 us that made the pass as slow at batch 32 as at batch 128)
  const int nchs = g.CT * 32;
  for (int i = threadIdx.x; i < nchs; i += kThreads) {
    const bool okc = i < g.Cout;
    c_zs[i] = okc ? g.zoff * wsum[i] : 0;
    c_k[i] = okc ? wscale[i] : 0.0f;
    c_k[nchs + i] = (okc && bias != nullptr) ? bias[i] : 0.0f;
    c_k[2 * nchs + i] = (okc && bn_scale != nullptr) ? bn_scale[i] : 1.0f;
    c_k[3 * nchs + i] = (okc && bn_scale != nullptr) ? bn_shift[i] : 0.0f;
  }
  if constexpr (FRONT)
    for (int i = threadIdx.x; i < g.Cin; i += kThreads) {
#pragma unroll
      for (int t = 0; t < 9; ++t) dwk[i * 12 + t] = fa.w[i * 9 + t];
      dwk[i * 12 + 9] = fa.bias != nullptr ? fa.bias[i] : 0.0f;
      dwk[i * 12 + 10] = fa.bn_scale != nullptr ? fa.bn_scale[i] : 1.0f;
      dwk[i * 12 + 11] = fa.bn_scale != nullptr ? fa.bn_shift[i] : 0.0f;
    }
  auto reset = [&]() __attribute__((always_inline)) {
    for (int ct = 0; ct < g.CT; ++ct) {
      my[ct * 128 + lane] = INT_MIN;
      my[ct * 128 + 64 + lane] = INT_MAX;
    }
  };
  reset();
  __syncthreads();
  const bool has_bn = bn_scale != nullptr;
  // the fp32 epilogue of fq_pwconv_i8 on the two extreme sums of every channel, then the maximum over the wave's channels
  auto flush = [&](unsigned smp) __attribute__((always_inline)) {
    float m = 0.0f;
    for (int ct = 0; ct < g.CT; ++ct) {
      const int c = ct * 32 + i32;
      int hi = my[ct * 128 + lane], lo = my[ct * 128 + 64 + lane];
      // (both halves hold the same channel: pixels 0..15 and 16..31)
      const int ohi = __shfl_xor(hi, 32, 64), olo = __shfl_xor(lo, 32, 64);
      hi = hi > ohi ? hi : ohi;
      lo = lo < olo ? lo : olo;
      if (c < g.Cout && hi >= lo) {
        hi += c_zs[c];
        lo += c_zs[c];
        const float sxw = q.scale * c_k[c];
        const float bch = c_k[nchs + c];
        const float bsc = c_k[2 * nchs + c], bsh = c_k[3 * nchs + c];
        auto f = [&](int a) {
          float v = (float)a * sxw;
          if (bias != nullptr) v = v + bch;
          if (has_bn) {
            v = v * bsc;
            v = v + bsh;
          }
          return fabsf(act_rt(v, act));
        };
        m = fmaxf(m, fmaxf(f(hi), f(lo)));
      }
    }
    m = wave_max_nonneg(m);
    // Where the maximum goes.  Few tiles per wavefront (small batches): into the workgroup's LDS table (fq_mma.h), ONE global
    // atomic per (workgroup, sample) at the end - a first version issued one per wavefront: 3072 atomics on the n floats of
    // stat_out (a single cache line at batch 32) serialise in L2 at ~10 ns each, a fixed 30 us that made the pass as slow at
    // batch 32 as at batch 128.  Many tiles per wavefront: straight to memory - the atomics of a long kernel are spread over
    // its run time and overlap with the other wavefronts' work, while the table's flush would put them all at the end (40
    // against 47 us on the first pair at batch 128).  profiles/r6_pwstat_atomics.txt
    if (lane == 0 && __float_as_uint(m) != 0u) {
      const unsigned slot = smp - s_base;
      if (g.table && slot < (unsigned)kStatSlots) atomicMax(&k_stat[slot], __float_as_uint(m));
      else FQ_STAT_FLUSH_MAX(reinterpret_cast<unsigned*>(stat_out) + smp, __float_as_uint(m));
    }
    reset();
  };
  v4i afrag[KT];
  const FastQuot fqx = make_fast_quot(q.denom);
  // pixels [plo, phi) of the tile (in tile order: this lane's registers are pixels 16 h + r) join the open sample
  auto reduce_tile = [&](int plo, int phi) __attribute__((always_inline)) {
    const bool whole = plo <= 0 && phi >= 32;
#pragma unroll 1
    for (int ct = 0; ct < g.CT; ++ct) {
      v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // (zoff * rowsum joins at the flush: max / min commute with it)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[kt], ldsW[((ct * KT + kt) << 6) + lane], acc, 0, 0, 0);
      int hi = INT_MIN, lo = INT_MAX;
      if (whole) {
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
          hi = max(max(acc[k], acc[k + 1]), hi);
          lo = min(min(acc[k], acc[k + 1]), lo);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int p = 16 * h + k;
          const bool in = p >= plo && p < phi;
          hi = in && acc[k] > hi ? acc[k] : hi;
          lo = in && acc[k] < lo ? acc[k] : lo;
        }
      }
      atomicMax(&my[ct * 128 + lane], hi);
      atomicMin(&my[ct * 128 + 64 + lane], lo);
    }
  };
  unsigned cur = FRONT ? s_base : fast_div((unsigned)((t_begin < g.tiles ? t_begin : g.tiles - 1) * 32), g.hw);
  auto run_tile = [&](int64_t t, auto ph_c, auto nn_c) __attribute__((always_inline)) {
    constexpr int PH = decltype(ph_c)::value;                 // the tile's first slab sits in buffer (PH * KT) % NB
    const Pix px = pix_of(t);
    const unsigned cvo = ((px.smp * (unsigned)(2 * KT) + (unsigned)h) * HW + px.p) * 16u;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int qn = kt + NB - 1;
      issue(t + qn / KT, qn % KT, raw[(PH * KT + kt + NB - 1) % NB]);
      FQ_PIN();
      afrag[kt] = pair_frag16<decltype(nn_c)::value>(raw[(PH * KT + kt) % NB], q, fqx, ubias, nn_xor);
      // (the whole offset in the lane register: with a constant scalar offset the compiler itself keeps the data registers of a
      // 16-byte store untouched for as long as the store reads them - fq_common.h at buf_st_v4f)
      if (wr_codes) buf_st_v4i(rcodes, cvo + (unsigned)(2 * kt) * HW * 16u, afrag[kt]);
      FQ_PIN();
    }
    const unsigned j0 = (unsigned)t * 32u, j1 = j0 + 31u < cols ? j0 + 31u : cols - 1;
    const unsigned s0 = fast_div(j0, g.hw), s1 = fast_div(j1, g.hw);
    if (s0 != cur) {
      flush(cur);
      cur = s0;
    }
    if (s0 == s1) {
      reduce_tile(0, 32);
    } else {                                   // a tile across two samples (planes of at least 32 pixels: never three)
      const int pb = (int)(s1 * HW - j0);
      reduce_tile(0, pb);
      flush(cur);
      cur = s1;
      reduce_tile(pb, 32);
    }
    FQ_PIN();
  };
  auto run_all = [&](auto nn_c) __attribute__((always_inline)) {
    constexpr int U = (KT % NB == 0) ? 1 : NB;                  // tiles per turn: U * KT is a multiple of NB (NB prime)
    using std::integral_constant;
    for (int64_t t = t_begin; t < t_end; t += U) {
      run_tile(t, integral_constant<int, 0>{}, nn_c);
      if (U > 1 && t + 1 < t_end) run_tile(t + 1, integral_constant<int, 1 % U>{}, nn_c);
      if (U > 2 && t + 2 < t_end) run_tile(t + 2, integral_constant<int, 2 % U>{}, nn_c);
      if (U > 3 && t + 3 < t_end) run_tile(t + 3, integral_constant<int, 3 % U>{}, nn_c);
    }
  };
  // FRONT: band by band - recompute the depthwise values into the band buffer as codes, then the tiles of the band
  // (phase 1 has a TWIN, word for word: pw_front_store_kernel's phase1 below - a change to the dequantiser, the tap chain, the
  // epilogue or the quantiser here is a change there, and tests/test_gpu_front_store.py compares that copy with the storing launches)
  auto run_front = [&](auto nn_c) __attribute__((always_inline)) {
    constexpr bool NN = decltype(nn_c)::value;
    constexpr int FE = FRONT ? FEPI : kEpiRuntime;
    const int Q = fa.Q, W = fa.W, H = fa.H;
    const int seg = lane / Q, pos = lane - seg * Q;
    const bool first = pos == 0, last = pos == Q - 1;
    const bool has_fb = fa.bias != nullptr, has_fbn = fa.bn_scale != nullptr;
    QParams qc = q;                               // compile-time epilogue, clip range from 0: ReLU / ReLU6 and the clip are one median
    if (NN && FE != kEpiRuntime) qc.hi = FE == kEpiBnRelu6 ? fminf(q.hi, 6.0f) : q.hi;
    const unsigned* xc32 = reinterpret_cast<const unsigned*>(fa.codes);
    const int z4 = stored_zero4(ubias);
    const v4i zero_frag = (v4i){z4, z4, z4, z4};
    auto deq = [&](unsigned wd, int b) __attribute__((always_inline)) {
      const int code = FSIGNED ? (int)(int8_t)(wd >> (8 * b)) : (int)((wd >> (8 * b)) & 255u);
      return (float)code * fscale;
    };
    for (int64_t bt = t_begin; bt < t_end; ++bt) {
      const unsigned smp = (unsigned)(bt / fa.bands);
      const int r0 = (int)(bt - (int64_t)smp * fa.bands) * fa.R;
      const int Rb = H - r0 < fa.R ? H - r0 : fa.R;
      if (smp != cur) {
        flush(cur);
        cur = smp;
      }
      // ---- 1: the depthwise layer on rows r0 - 1 .. r0 + Rb of `segs` channels per wavefront and turn ----
      for (int c0 = 0; c0 < g.Cin; c0 += NW * fa.segs) {
        const int c = front_channel(c0, wave, fa.segs, seg);
        const bool c_ok = seg < fa.segs && c < g.Cin;
        const int cc = c_ok ? c : 0;
        const float* kc = dwk + cc * 12;
        const float w00 = kc[0], w01 = kc[1], w02 = kc[2], w10 = kc[3], w11 = kc[4], w12 = kc[5], w20 = kc[6], w21 = kc[7],
                    w22 = kc[8], bch = kc[9], bsc = kc[10], bsh = kc[11];
        const unsigned* src = xc32 + ((int64_t)(smp * (unsigned)g.Cin + (unsigned)cc) * H) * Q + pos;
        unsigned raw_c[kFrontRows + 2];           // (unconditional loads from clamped rows, masked: a row outside the plane is zero codes)
#pragma unroll
        for (int k = 0; k < kFrontRows + 2; ++k) {
          const int t = r0 - 1 + k, tc = t < 0 ? 0 : (t > H - 1 ? H - 1 : t);
          raw_c[k] = src[tc * Q] & ((t >= 0 && t < H) ? 0xFFFFFFFFu : 0u);
        }
        // this launch's code of one depthwise sum (the stored byte of the C16 layout)
        auto zcode = [&](float acc) __attribute__((always_inline)) {
          if constexpr (NN) {
            const float v = FE == kEpiRuntime ? dw_finish<kEpiRuntime>(acc, has_fb, bch, has_fbn, bsc, bsh, fa.act)
                                              : dw_finish<FE, false>(acc, false, 0.0f, true, bsc, bsh, 0);
            return (unsigned)fq_code_nonneg(v, qc, fqx) ^ (nn_xor & 255u);
          } else {
            const float v = dw_finish<FE>(acc, has_fb, bch, has_fbn, bsc, bsh, fa.act);
            return (unsigned)(fq_code_int(v, q) + ubias) ^ 0x80u;
          }
        };
        float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // the lane's byte of band pixel (row 0, column 4 pos); a column / a row further on are front_byte's own strides (the map
        // is linear in the row and in the column of a four-column group) - one running address instead of 32
        unsigned dst = (unsigned)front_byte(fa.lay, cc, 4 * pos);
        const unsigned jstep = (unsigned)(front_byte(fa.lay, 0, 1) - front_byte(fa.lay, 0, 0));
        const unsigned rstep = (unsigned)(front_byte(fa.lay, 0, 4 * Q) - front_byte(fa.lay, 0, 0));
#pragma unroll
        for (int k = 0; k < kFrontRows + 2; ++k) {
          if (k <= Rb + 1) {                      // (the same for the whole workgroup)
            float cv[6];
#pragma unroll
            for (int j = 0; j < 4; ++j) cv[j + 1] = deq(raw_c[k], j);
            const float lp = lane_prev(cv[4]), ln = lane_next(cv[1]);      // (taken by every lane, masked afterwards)
            cv[0] = first ? 0.0f : lp;
            cv[5] = last ? 0.0f : ln;
            if (k >= 2) {                         // input row r0 + k - 1 closes output row r0 + k - 2
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const unsigned code = zcode(dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a[j], a[j + 1], a[j + 2], b[j],
                                                    b[j + 1], b[j + 2], cv[j], cv[j + 1], cv[j + 2]));
                if (c_ok) zbuf[dst + j * jstep] = (unsigned char)code;
              }
              dst += rstep;
              asm volatile("" : "+v"(dst));
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
              a[j] = b[j];
              b[j] = cv[j];
            }
          }
        }
      }
      __syncthreads();
      // ---- 2: the band's pixels as 32-pixel tiles (the last one may be short: its lanes past the band repeat the last pixel) ----
      const int npix = Rb * W, ntile = (npix + 31) >> 5;
      for (int tl = wave; tl < ntile; tl += NW) {
        int pp = tl * 32 + pl;
        pp = pp < npix ? pp : npix - 1;
        // channels 32 kt + 16 h .. + 15 of pixel pp: byte 0 of planes 8 kt + 4 h .. + 3 (the half-slab past Cin has no planes)
        const unsigned* zp = reinterpret_cast<const unsigned*>(zbuf + front_byte(fa.lay, g.Cin <= 16 ? 0 : 16 * h, pp));
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          v4i f;
#pragma unroll
          for (int u = 0; u < 4; ++u) f[u] = (int)zp[(8 * kt + u) * fa.lay.pl];
          if (KT == 1 && g.Cin <= 16 && h == 1) f = zero_frag;     // (the half-slab past Cin: the code of 0)
          if (wr_codes)
            buf_st_v4i(rcodes, ((smp * (unsigned)(2 * KT) + (unsigned)(2 * kt + h)) * HW + (unsigned)(r0 * W + pp)) * 16u, f);
          afrag[kt] = f;
        }
        const int valid = npix - tl * 32;
        reduce_tile(0, valid < 32 ? valid : 32);
      }
      __syncthreads();                            // (the next band overwrites the buffer)
    }
  };
  if constexpr (FRONT) {
    if (fq_nonneg(q) && fqx.ok) run_front(std::true_type{});
    else run_front(std::false_type{});
  } else {
    if (fq_nonneg(q) && fqx.ok) run_all(std::true_type{});
    else run_all(std::false_type{});
  }
  if (t_begin < t_end) flush(cur);
  __syncthreads();
  mma_stat_flush(k_stat, stat_out, s_base, cols, HW);
}

// ---- fq_pwconv_i8_front: the STORING 1x1 behind a stride-1 depthwise 3x3 that was never stored --------------------------------
// 256 -> 256 channels (MobileNet1.0's 28 x 28 layers: the fp32 tensor between the two is written once and read once, only to be
// quantised).  Phase 1 is run_front's above, word for word - the band of codes in the fq_front_layout.h buffer.  Phase 2 turns the
// operands round: the WEIGHTS are the A operand and the band's pixels the B operand (the fragment read from the band buffer is the
// same four dwords per slab either way), so lane = pixel, register = channel 8 g + 4 h + r of the tile, and the 32 pixels of a
// channel leave as one 128-byte run - the epilogue and the store pattern of the sample form (fq_pw_sample.hip), whose values
// these are bit for bit.  With lane = channel (the statistic pass's roles) a store would be 16 bytes per lane on 64 planes.
// A wavefront owns CTW = 8 / NW channel tiles and keeps their 8 CTW weight fragments in registers for the whole launch (32 or 64
// VGPRs); it walks all pixel tiles of every band with them.  Beside the band, LDS holds the per-channel constants only.
struct PwFrontStoreGeom {
  int Cin, KTS, Cout, HW, zoff;
  int n;                     // samples
};

template <int FEPI, bool FSIGNED, int NW>
__global__ __launch_bounds__(64 * NW, NW == kFrontWavesWide ? 4 : 2) void pw_front_store_kernel(
    const int8_t* __restrict__ wfrag, const float* __restrict__ wscale, const int* __restrict__ wsum,
    const float* __restrict__ bias, float* __restrict__ y, PwFrontStoreGeom g, const float* __restrict__ in_stat,
    const float* __restrict__ in_thr, float levels, int lo_neg, float eps, float* __restrict__ cur_max_out,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, int act, float* __restrict__ stat_out,
    PwFrontArgs fa) {
  constexpr int KT = 8, CTW = 8 / NW;            // 256 input channels, 256 output channels
  constexpr int kThreads = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char pfs_smem[];
  int* c_zs = reinterpret_cast<int*>(pfs_smem);                                             // [Cout]
  float* c_k = reinterpret_cast<float*>(c_zs + g.Cout);                                     // [4][Cout]: sx * w scale, bias, BN scale / shift
  float* dwk = c_k + 4 * g.Cout;                                                            // [Cin][12] taps, bias, BN scale / shift
  unsigned char* zbuf = reinterpret_cast<unsigned char*>(dwk + g.Cin * 12);                 // [Cin / 4][lay.pl] dwords, band of codes
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = lane >> 5, i32 = lane & 31;
  const unsigned HW = (unsigned)g.HW;
  // the workgroup's bands (band b of sample s is number s * bands + b)
  const int64_t n_bands = (int64_t)g.n * fa.bands;
  const int64_t t_begin = n_bands * blockIdx.x / gridDim.x, t_end = n_bands * (blockIdx.x + 1) / gridDim.x;
  __shared__ unsigned k_stat[kStatSlots];
  mma_stat_init(k_stat);
  const unsigned s_base = (unsigned)((t_begin < n_bands ? t_begin : n_bands - 1) / fa.bands);
  // this wavefront's weight fragments (fq_weight_codes' fragment-major copy: one coalesced 16-byte load each)
  v4i wf[CTW][KT];
#pragma unroll
  for (int c = 0; c < CTW; ++c)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
      wf[c][kt] = *reinterpret_cast<const v4i*>(wfrag + (((int64_t)(wave * CTW + c) * g.KTS + kt) << 10) + (lane << 4));
  const float fscale = input_threshold(fa.in_stat, g.n, fa.in_thr, nullptr, false) / fa.levels;
  const float max_ = input_threshold(in_stat, g.n, in_thr, cur_max_out, blockIdx.x == 0);
  const QParams q = make_qparams(max_, levels, lo_neg != 0, eps);
  const int ubias = 128 - g.zoff;
  const unsigned nn_xor = fq_nonneg_xor(ubias);
  const bool has_bn = bn_scale != nullptr;
  for (int i = threadIdx.x; i < g.Cout; i += kThreads) {
    c_zs[i] = g.zoff * wsum[i];
    c_k[i] = q.scale * wscale[i];
    c_k[g.Cout + i] = bias != nullptr ? bias[i] : 0.0f;
    c_k[2 * g.Cout + i] = has_bn ? bn_scale[i] : 1.0f;
    c_k[3 * g.Cout + i] = has_bn ? bn_shift[i] : 0.0f;
  }
  for (int i = threadIdx.x; i < g.Cin; i += kThreads) {
#pragma unroll
    for (int t = 0; t < 9; ++t) dwk[i * 12 + t] = fa.w[i * 9 + t];
    dwk[i * 12 + 9] = fa.bias != nullptr ? fa.bias[i] : 0.0f;
    dwk[i * 12 + 10] = fa.bn_scale != nullptr ? fa.bn_scale[i] : 1.0f;
    dwk[i * 12 + 11] = fa.bn_scale != nullptr ? fa.bn_shift[i] : 0.0f;
  }
  __syncthreads();
  const FastQuot fqx = make_fast_quot(q.denom);
  const int Q = fa.Q, W = fa.W, H = fa.H;

  // ---- 1: the depthwise layer on rows r0 - 1 .. r0 + Rb of `segs` channels per wavefront and turn (pw_stat_kernel's run_front) ----
  auto phase1 = [&](auto nn_c, unsigned smp, int r0, int Rb) __attribute__((always_inline)) {
    constexpr bool NN = decltype(nn_c)::value;
    const int seg = lane / Q, pos = lane - seg * Q;
    const bool first = pos == 0, last = pos == Q - 1;
    const bool has_fb = fa.bias != nullptr, has_fbn = fa.bn_scale != nullptr;
    QParams qc = q;                               // compile-time epilogue, clip range from 0: ReLU / ReLU6 and the clip are one median
    if (NN && FEPI != kEpiRuntime) qc.hi = FEPI == kEpiBnRelu6 ? fminf(q.hi, 6.0f) : q.hi;
    const unsigned* xc32 = reinterpret_cast<const unsigned*>(fa.codes);
    auto deq = [&](unsigned wd, int b) __attribute__((always_inline)) {
      const int code = FSIGNED ? (int)(int8_t)(wd >> (8 * b)) : (int)((wd >> (8 * b)) & 255u);
      return (float)code * fscale;
    };
    for (int c0 = 0; c0 < g.Cin; c0 += NW * fa.segs) {
      const int c = front_channel(c0, wave, fa.segs, seg);
      const bool c_ok = seg < fa.segs && c < g.Cin;
      const int cc = c_ok ? c : 0;
      const float* kc = dwk + cc * 12;
      const float w00 = kc[0], w01 = kc[1], w02 = kc[2], w10 = kc[3], w11 = kc[4], w12 = kc[5], w20 = kc[6], w21 = kc[7],
                  w22 = kc[8], bch = kc[9], bsc = kc[10], bsh = kc[11];
      const unsigned* src = xc32 + ((int64_t)(smp * (unsigned)g.Cin + (unsigned)cc) * H) * Q + pos;
      unsigned raw_c[kFrontRows + 2];           // (unconditional loads from clamped rows, masked: a row outside the plane is zero codes)
#pragma unroll
      for (int k = 0; k < kFrontRows + 2; ++k) {
        const int t = r0 - 1 + k, tc = t < 0 ? 0 : (t > H - 1 ? H - 1 : t);
        raw_c[k] = src[tc * Q] & ((t >= 0 && t < H) ? 0xFFFFFFFFu : 0u);
      }
      // this launch's code of one depthwise sum (the stored byte of the C16 layout)
      auto zcode = [&](float acc) __attribute__((always_inline)) {
        if constexpr (NN) {
          const float v = FEPI == kEpiRuntime ? dw_finish<kEpiRuntime>(acc, has_fb, bch, has_fbn, bsc, bsh, fa.act)
                                              : dw_finish<FEPI, false>(acc, false, 0.0f, true, bsc, bsh, 0);
          return (unsigned)fq_code_nonneg(v, qc, fqx) ^ (nn_xor & 255u);
        } else {
          const float v = dw_finish<FEPI>(acc, has_fb, bch, has_fbn, bsc, bsh, fa.act);
          return (unsigned)(fq_code_int(v, q) + ubias) ^ 0x80u;
        }
      };
      float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      unsigned dst = (unsigned)front_byte(fa.lay, cc, 4 * pos);
      const unsigned jstep = (unsigned)(front_byte(fa.lay, 0, 1) - front_byte(fa.lay, 0, 0));
      const unsigned rstep = (unsigned)(front_byte(fa.lay, 0, 4 * Q) - front_byte(fa.lay, 0, 0));
#pragma unroll
      for (int k = 0; k < kFrontRows + 2; ++k) {
        if (k <= Rb + 1) {                      // (the same for the whole workgroup)
          float cv[6];
#pragma unroll
          for (int j = 0; j < 4; ++j) cv[j + 1] = deq(raw_c[k], j);
          const float lp = lane_prev(cv[4]), ln = lane_next(cv[1]);      // (taken by every lane, masked afterwards)
          cv[0] = first ? 0.0f : lp;
          cv[5] = last ? 0.0f : ln;
          if (k >= 2) {                         // input row r0 + k - 1 closes output row r0 + k - 2
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const unsigned code = zcode(dw_taps(w00, w01, w02, w10, w11, w12, w20, w21, w22, a[j], a[j + 1], a[j + 2], b[j],
                                                  b[j + 1], b[j + 2], cv[j], cv[j + 1], cv[j + 2]));
              if (c_ok) zbuf[dst + j * jstep] = (unsigned char)code;
            }
            dst += rstep;
            asm volatile("" : "+v"(dst));
          }
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            a[j] = b[j];
            b[j] = cv[j];
          }
        }
      }
    }
  };

  // ---- 2: the band's pixels as 32-pixel tiles, lane = pixel (the last tile may be short: its lanes past the band repeat the last
  // pixel and store nothing); FAST: BatchNorm + ReLU, no bias, fixed at compile time ----
  float m = 0.0f;
  auto phase2 = [&](auto fast_c, unsigned smp, int r0, int Rb) __attribute__((always_inline)) {
    constexpr bool FAST = decltype(fast_c)::value;
    const int npix = Rb * W, ntile = (npix + 31) >> 5;
    const unsigned plane4 = HW * 4u;
    // the wavefront's window on y: its first channel tile of sample smp, to the end of the sample
    const int ch0 = wave * CTW * 32;
    const fq_rsrc yr = make_rsrc(reinterpret_cast<char*>(y) + ((int64_t)smp * g.Cout + ch0) * plane4,
                                 (int64_t)(g.Cout - ch0) * plane4);
    for (int tl = 0; tl < ntile; ++tl) {
      const int pt = tl * 32 + i32;
      const bool ok = pt < npix;
      const int pp = ok ? pt : npix - 1;
      // channels 32 kt + 16 h .. + 15 of pixel pp: byte 0 of planes 8 kt + 4 h .. + 3
      const unsigned* zp = reinterpret_cast<const unsigned*>(zbuf + front_byte(fa.lay, 16 * h, pp));
      v4i bf[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int u = 0; u < 4; ++u) bf[kt][u] = (int)zp[(8 * kt + u) * fa.lay.pl];
      const unsigned po = ok ? (unsigned)(4 * h) * plane4 + (unsigned)(r0 * W + pt) * 4u : kOobOffset;
      // (the constants' offset is made opaque once per tile: they are the same for every tile, and hoisted out of this loop
      // their 20 registers per group of four channels would push the weight fragments out of the register file)
      int kb = ch0 + 4 * h;
      asm volatile("" : "+v"(kb));
#pragma unroll
      for (int c = 0; c < CTW; ++c) {
        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[c][kt], bf[kt], acc, 0, 0, 0);
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int c0 = kb + c * 32 + 8 * gq;
          const v4i zs = *reinterpret_cast<const v4i*>(c_zs + c0);
          const f4 sxw = *reinterpret_cast<const f4*>(c_k + c0);
          const f4 bch = *reinterpret_cast<const f4*>(c_k + g.Cout + c0);
          const f4 bsc = *reinterpret_cast<const f4*>(c_k + 2 * g.Cout + c0);
          const f4 bsh = *reinterpret_cast<const f4*>(c_k + 3 * g.Cout + c0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = (float)(acc[4 * gq + r] + zs[r]);
            v = v * sxw[r];
            if (FAST) {
              v = v * bsc[r];
              v = v + bsh[r];
              v = fmaxf(v, 0.0f);
            } else {
              if (bias != nullptr) v = v + bch[r];
              if (has_bn) {
                v = v * bsc[r];
                v = v + bsh[r];
              }
              v = act_rt(v, act);
            }
            buf_st_f32(yr, po, (unsigned)(c * 32 + 8 * gq + r) * plane4, v);
            m = fmaxf(m, ok ? fabsf(v) : 0.0f);
          }
        }
      }
    }
  };

  const bool nn = fq_nonneg(q) && fqx.ok, fast_epi = bias == nullptr && has_bn && act == FQ_ACT_RELU;
  for (int64_t bt = t_begin; bt < t_end; ++bt) {
    const unsigned smp = (unsigned)(bt / fa.bands);
    const int r0 = (int)(bt - (int64_t)smp * fa.bands) * fa.R;
    const int Rb = H - r0 < fa.R ? H - r0 : fa.R;
    if (nn) phase1(std::true_type{}, smp, r0, Rb);
    else phase1(std::false_type{}, smp, r0, Rb);
    __syncthreads();
    if (fast_epi) phase2(std::true_type{}, smp, r0, Rb);
    else phase2(std::false_type{}, smp, r0, Rb);
    mma_stat_update(k_stat, stat_out, smp, s_base, m);      // (every lane of the wavefront sits in sample smp)
    m = 0.0f;
    __syncthreads();                              // (the next band overwrites the buffer)
  }
  mma_stat_flush(k_stat, stat_out, s_base, (int64_t)g.n * g.HW, HW);
}
}  // namespace

namespace fqi {

// LDS of the statistic pass beside a front layer's (fq_front_layout.h, where the host walk counts it too)
static size_t pw_stat_lds(int kt, int ct, int waves = kFrontWaves) { return stat_fixed_lds(kt, ct, waves); }

bool pw_stat_shape_ok(int64_t n, int64_t cin, int64_t cout, int64_t hw) {
  if (n <= 0 || cin <= 0 || cout <= 0 || hw < 32 || hw >= (1ll << 30) || n * hw >= (1ll << 31) - 512) return false;
  const int kt = (int)((cin + 31) / 32), ct = (int)((cout + 31) / 32);
  if (!(kt == 1 || kt == 2 || kt == 4 || kt == 8) || cin % 16 != 0) return false;
  // (the kernel's one resource spans all of x and its lane offsets are 32-bit: x below 4 GiB.  A half-slab past Cin - Cin % 32
  // == 16 - is masked with the lane offset 2^31, which only lies outside a resource of at most 2 GiB: beyond, the masked lanes
  // would load values of sample n / 2 and x_codes_out would carry their codes in its padding block)
  const int64_t x_bytes = n * cin * hw * 4;
  return pw_stat_lds(kt, ct) <= (size_t)kStatLdsMax && x_bytes < (1ll << 32) && (cin % 32 == 0 || x_bytes <= (1ll << 31));
}

// wavefronts per workgroup, rows per band and LDS of the front-layer mode: front_plan of fq_front_layout.h.
// FQ_PWSTAT_FRONT_ROWS and FQ_PWSTAT_FRONT_WAVES force the first two and are read at every call, so that a test can vary them
// inside one process.
static FrontPlan pw_front_plan(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w) {
  const char* e = getenv("FQ_PWSTAT_FRONT_ROWS");
  const char* ew = getenv("FQ_PWSTAT_FRONT_WAVES");
  static const int wg_env = env_int("FQ_PWSTAT_WG_PER_CU", 0);
  return front_plan(n, cin, cout, h, w, num_cu(), wg_env > 0 ? wg_env : kFrontWgCap, e != nullptr ? atoi(e) : 0,
                    ew != nullptr ? atoi(ew) : 0);
}

bool pw_stat_front_shape_ok(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w) {
  if (h < 1 || w < 4 || w % 4 != 0 || w / 4 > 64 || !(cin == 16 || cin == 32 || cin == 64 || cin == 128) ||
      !pw_stat_shape_ok(n, cin, cout, h * w))
    return false;
  // (the depthwise statistic pass in front must take the plane too: fq_dwconv3x3 without y)
  return pw_front_plan(n, cin, cout, h, w).rows >= 1 && n * cin * ((w / 4 + 61) / 62) < (1ll << 31) - 1024;
}

// one instantiation's launch: it owns the raised dynamic LDS limit, and pw_stat_kernel's argument list is written here only
template <int KT, int FEPI, bool FSIGNED, int NW>
static int pw_stat_go(const PwCall& c, const PwStatGeom& g, const PwFrontArgs& fa, int64_t grid, size_t lds) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_stat_kernel<KT, FEPI, FSIGNED, NW>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_pwconv_i8_stat: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((pw_stat_kernel<KT, FEPI, FSIGNED, NW>), dim3((unsigned)grid), dim3(64 * NW), lds, c.st, c.x, c.wcodes,
                     c.wscale, (const int*)c.wsum, c.bias, g, c.in_stat, (int)c.n, c.in_thr, c.levels, c.lo_neg, kEps,
                     c.out_current_max, c.bn_scale, c.bn_shift, c.act, c.stat_out, (int8_t*)c.x_codes_out, fa);
  note_launch(FQ_KERNEL_PWCONV, FQ_LAUNCH_STAT, {KT, NW, FEPI, g.table});
  return FQ_OK;
}

int pw_stat_launch(const PwCall& c) {
  const int kt = (int)((c.cin + 31) / 32), ct = (int)((c.cout + 31) / 32);
  size_t lds = pw_stat_lds(kt, ct);
  PwFrontArgs fa = {};
  int waves = kFrontWaves;
  if (c.front != nullptr) {
    const PwFront& f = *c.front;
    fa.codes = static_cast<const int8_t*>(f.codes);
    fa.w = f.w; fa.bias = f.bias; fa.bn_scale = f.bn_scale; fa.bn_shift = f.bn_shift;
    fa.in_stat = f.in_stat; fa.in_thr = f.in_thr; fa.levels = f.levels; fa.act = f.act;
    fa.H = (int)f.h; fa.W = (int)f.wdt; fa.Q = fa.W / 4; fa.segs = 64 / fa.Q;
    const FrontPlan plan = pw_front_plan(c.n, c.cin, c.cout, f.h, f.wdt);
    waves = plan.waves;
    fa.R = plan.rows;
    FQ_REQUIRE(fa.R >= 1, "fq_pwconv_i8_stat: no band of the front layer fits the LDS");
    fa.bands = (fa.H + fa.R - 1) / fa.R;
    fa.lay = front_layout(fa.Q, fa.R);
    lds = plan.lds;
  }
  PwStatGeom g;
  g.Cin = (int)c.cin; g.KTS = (int)(c.cin_pad / 32); g.Cout = (int)c.cout; g.CT = ct; g.HW = (int)c.hw;
  g.cols = c.n * c.hw; g.tiles = (g.cols + 31) / 32; g.zoff = c.zoff;
  g.hw = fast_div_for((unsigned)c.hw);
  if (int rc = pw_zero_stat(c)) return rc;
  int per_cu = stat_wg_per_cu(lds, c.front != nullptr ? stat_wg_cap(kFrontWgCap, waves) : 3);
  static const int wg_env = env_int("FQ_PWSTAT_WG_PER_CU", 0);
  if (wg_env > 0) per_cu = wg_env;
  int64_t grid = (int64_t)num_cu() * per_cu;
  const int64_t need = c.front != nullptr ? c.n * fa.bands : (g.tiles + 3) / 4;
  if (grid > need) grid = need;
  const int table_env = env_int("FQ_PWSTAT_TABLE", -1);                 // tuning: 0 / 1, read per call
  g.table = table_env >= 0 ? table_env : (g.tiles < grid * waves * 10 ? 1 : 0);
  int rc = FQ_OK;
  if (c.front != nullptr) {
    FQ_REQUIRE(kt == 1 || kt == 2 || kt == 4, "fq_pwconv_i8_stat: a front layer needs cin <= 128");
    // front layer: the depthwise epilogue at compile time where fq_dwconv3x3 has it so, the signedness of its input codes
    // (eight wavefronts: instantiated where pw_front_plan can choose them, two and four slabs)
    const int epi = (c.front->epi == kEpiBnRelu || c.front->epi == kEpiBnRelu6) ? c.front->epi : kEpiRuntime;
    pair_pick<1, 2, 4>(kt, [&](auto kt_c) {
      pair_pick<kEpiBnRelu, kEpiBnRelu6, kEpiRuntime>(epi, [&](auto epi_c) {
        pair_pick<0, 1>(c.front->is_signed ? 1 : 0, [&](auto sg_c) {
          constexpr int KT = decltype(kt_c)::value, EPI = decltype(epi_c)::value;
          constexpr bool SG = decltype(sg_c)::value != 0;
          if constexpr (KT >= 2) {
            if (waves == kFrontWavesWide) {
              rc = pw_stat_go<KT, EPI, SG, kFrontWavesWide>(c, g, fa, grid, lds);
              return;
            }
          }
          rc = pw_stat_go<KT, EPI, SG, kFrontWaves>(c, g, fa, grid, lds);
        });
      });
    });
  } else if (!pair_pick<1, 2, 4, 8>(kt, [&](auto kt_c) {
               rc = pw_stat_go<decltype(kt_c)::value, -1, false, kFrontWaves>(c, g, fa, grid, lds);
             })) {
    return fail(FQ_ERR_INVALID, "fq_pwconv_i8_stat: K / 32 = %d is not instantiated", kt);
  }
  if (rc != FQ_OK) return rc;
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

// ---- fq_pwconv_i8_front ----------------------------------------------------------------------------------------------------
// front_store_plan of fq_front_layout.h, with the statistic pass's knobs: FQ_PWSTAT_FRONT_ROWS / FQ_PWSTAT_FRONT_WAVES
static FrontPlan pw_front_store_plan(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w) {
  const char* e = getenv("FQ_PWSTAT_FRONT_ROWS");
  const char* ew = getenv("FQ_PWSTAT_FRONT_WAVES");
  return front_store_plan(n, cin, cout, h, w, num_cu(), kFrontWgCap, e != nullptr ? atoi(e) : 0, ew != nullptr ? atoi(ew) : 0);
}

bool pw_front_store_shape_ok(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w) {
  if (n <= 0 || h < 1 || w < 4 || w % 4 != 0 || w / 4 > 64 || cin != 256 || cout != 256) return false;
  if (n * h * w >= (1ll << 31) - 512 || n * cin * h * w * 4 >= (1ll << 32)) return false;
  // (the depthwise statistic pass in front must take the plane too: fq_dwconv3x3 without y)
  return pw_front_store_plan(n, cin, cout, h, w).rows >= 1 && n * cin * ((w / 4 + 61) / 62) < (1ll << 31) - 1024;
}

template <int FEPI, bool FSIGNED, int NW>
static int pw_front_store_go(const PwCall& c, const PwFrontStoreGeom& g, const PwFrontArgs& fa, int64_t grid, size_t lds) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_front_store_kernel<FEPI, FSIGNED, NW>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_pwconv_i8_front: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((pw_front_store_kernel<FEPI, FSIGNED, NW>), dim3((unsigned)grid), dim3(64 * NW), lds, c.st, c.wcodes,
                     c.wscale, (const int*)c.wsum, c.bias, c.y, g, c.in_stat, c.in_thr, c.levels, c.lo_neg, kEps,
                     c.out_current_max, c.bn_scale, c.bn_shift, c.act, c.stat_out, fa);
  return FQ_OK;
}

int pw_front_store_launch(const PwCall& c) {
  const PwFront& f = *c.front;
  PwFrontArgs fa = {};
  fa.codes = static_cast<const int8_t*>(f.codes);
  fa.w = f.w; fa.bias = f.bias; fa.bn_scale = f.bn_scale; fa.bn_shift = f.bn_shift;
  fa.in_stat = f.in_stat; fa.in_thr = f.in_thr; fa.levels = f.levels; fa.act = f.act;
  fa.H = (int)f.h; fa.W = (int)f.wdt; fa.Q = fa.W / 4; fa.segs = 64 / fa.Q;
  const FrontPlan plan = pw_front_store_plan(c.n, c.cin, c.cout, f.h, f.wdt);
  fa.R = plan.rows;
  FQ_REQUIRE(fa.R >= 1, "fq_pwconv_i8_front: no band of the front layer fits the LDS");
  fa.bands = (fa.H + fa.R - 1) / fa.R;
  fa.lay = front_layout(fa.Q, fa.R);
  PwFrontStoreGeom g;
  g.Cin = (int)c.cin; g.KTS = (int)(c.cin_pad / 32); g.Cout = (int)c.cout; g.HW = (int)c.hw; g.zoff = c.zoff; g.n = (int)c.n;
  if (int rc = pw_zero_stat(c)) return rc;
  int64_t grid = (int64_t)num_cu() * stat_wg_per_cu(plan.lds, stat_wg_cap(kFrontWgCap, plan.waves));
  if (grid > c.n * fa.bands) grid = c.n * fa.bands;
  int rc = FQ_OK;
  const int epi = (f.epi == kEpiBnRelu || f.epi == kEpiBnRelu6) ? f.epi : kEpiRuntime;
  pair_pick<kEpiBnRelu, kEpiBnRelu6, kEpiRuntime>(epi, [&](auto epi_c) {
    pair_pick<0, 1>(f.is_signed ? 1 : 0, [&](auto sg_c) {
      constexpr int EPI = decltype(epi_c)::value;
      constexpr bool SG = decltype(sg_c)::value != 0;
      if (plan.waves == kFrontWavesWide) rc = pw_front_store_go<EPI, SG, kFrontWavesWide>(c, g, fa, grid, plan.lds);
      else rc = pw_front_store_go<EPI, SG, kFrontWaves>(c, g, fa, grid, plan.lds);
    });
  });
  if (rc != FQ_OK) return rc;
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

}  // namespace fqi
