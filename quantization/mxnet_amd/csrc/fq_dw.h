// libfakequant — the depthwise 3x3 family: the internal interface between fq_dwconv3x3 (fq_dwconv.hip) and its five kernel
// forms, one translation unit each, and the pieces the forms share, each written here once.  Tap chain and epilogue are also
// taken by the units that recompute or imitate a depthwise layer (fq_pw_stat, fq_pwdw, fq_dwconv16, the first convolutions).
#ifndef FQ_DW_H_
#define FQ_DW_H_

#include "fq_common.h"

namespace fqi {

// One call of fq_dwconv3x3: the arguments and what every form derives from them.
struct DwCall {
  const float *x, *w, *bias;
  float* y;
  int64_t n, c, h, wdt;
  int stride;
  const float *in_stat, *in_thr;
  float* out_current_max;
  const float *bn_scale, *bn_shift;
  int act;
  float* stat_out;
  hipStream_t st;
  bool quant, online, prezeroed;
  int epi;                  // kEpi*: the epilogue fixed at compile time, or the run-time one
  float levels, eps;
  int lo_neg;
  int64_t ho, wo;
  void* x_codes_out;        // y == NULL (the statistic pass): where the codes of x go, or NULL
};

// A form takes the call when *_applies says so (form: FQ_DW_FORM, 0 = by shape) and dw_run_* launches it; fq_dwconv.hip asks
// them in this order, and the tiles take every shape.
bool dw_flat_applies(const DwCall& d, int form), dw_planes_applies(const DwCall& d, int form);      // K2p fq_dw_flat.hip, K2o fq_dw_planes.hip
bool dw_cols4_applies(const DwCall& d, int form), dw_cols_applies(const DwCall& d, int form);       // K2e, K2d fq_dw_cols.hip
bool dw_flat_stat_applies(const DwCall& d);                                                        // ... K2p as a statistic pass (y == NULL)
int dw_run_flat(const DwCall& d), dw_run_planes(const DwCall& d), dw_run_cols4(const DwCall& d), dw_run_cols(const DwCall& d);
int dw_run_tiles(const DwCall& d);                                                                  // K2c fq_dw_tiles.hip
// fq_dwconv.hip: the depthwise layer of nn.Conv2D(quantized=True) (fq_qconv.hip)
int dw_range_call(const float* x, const float* wcodes_f32, float* y, int64_t n, int64_t c, int64_t h, int64_t wdt, int stride,
                  const float* rec, const float* svec, const float* bn_scale, const float* bn_shift, int act,
                  float* stat_out, hipStream_t st);

}  // namespace fqi

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat2(float v) { return (f2){v, v}; }

// The 3x3 sum of one output: rows a, b, c (above, centre, below), each as left / centre / right.  The order of these nine
// operations is the numerical contract of the unit (the oracle emulates exactly this chain).
__device__ __forceinline__ float dw_taps(float w00, float w01, float w02, float w10, float w11, float w12, float w20,
                                         float w21, float w22, float a0, float a1, float a2, float b0, float b1, float b2,
                                         float c0, float c1, float c2) {
  float acc = 0.0f;
  acc = fmaf(w00, a0, acc);
  acc = fmaf(w01, a1, acc);
  acc = fmaf(w02, a2, acc);
  acc = fmaf(w10, b0, acc);
  acc = fmaf(w11, b1, acc);
  acc = fmaf(w12, b2, acc);
  acc = fmaf(w20, c0, acc);
  acc = fmaf(w21, c1, acc);
  acc = fmaf(w22, c2, acc);
  return acc;
}
// Two outputs as ONE chain of packed fp32 FMAs (v_pk_fma_f32: two IEEE FMAs per lane per instruction, same order)
__device__ __forceinline__ f2 dw_taps2(float w00, float w01, float w02, float w10, float w11, float w12, float w20, float w21,
                                       float w22, f2 a0, f2 a1, f2 a2, f2 b0, f2 b1, f2 b2, f2 c0, f2 c1, f2 c2) {
  f2 acc = {0.f, 0.f};
  acc = __builtin_elementwise_fma(splat2(w00), a0, acc);
  acc = __builtin_elementwise_fma(splat2(w01), a1, acc);
  acc = __builtin_elementwise_fma(splat2(w02), a2, acc);
  acc = __builtin_elementwise_fma(splat2(w10), b0, acc);
  acc = __builtin_elementwise_fma(splat2(w11), b1, acc);
  acc = __builtin_elementwise_fma(splat2(w12), b2, acc);
  acc = __builtin_elementwise_fma(splat2(w20), c0, acc);
  acc = __builtin_elementwise_fma(splat2(w21), c1, acc);
  acc = __builtin_elementwise_fma(splat2(w22), c2, acc);
  return acc;
}

// The input quantiser of a launch (a kernel without one keeps `QParams q = {}`).  dw_qparams loads the threshold where it
// stands; dw_qparams_finish turns the loads that threshold_request issued earlier into the same parameters.
template <bool ONLINE>
__device__ __forceinline__ QParams dw_qparams(const float* in_stat, int n, const float* in_thr,
                                              float levels, int lo_neg_max, float eps, float* cur_max_out) {
  const float max_ = input_threshold(in_stat, n, ONLINE ? nullptr : in_thr, cur_max_out, blockIdx.x == 0);
  return make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
}
template <bool ONLINE>
__device__ __forceinline__ QParams dw_qparams_finish(const ThresholdReq& treq, const float* in_stat, int n,
                                                     const float* in_thr, float levels, int lo_neg_max, float eps,
                                                     float* cur_max_out) {
  const float max_ = threshold_finish(treq, in_stat, n, ONLINE ? nullptr : in_thr, cur_max_out, blockIdx.x == 0);
  return make_qparams_rt(max_, levels, lo_neg_max, eps, in_thr);
}

// A workgroup takes a CONTIGUOUS range of blocks (few samples -> a small LDS statistic table, one flush) and its
// wavefronts run through them without barriers.  Index arithmetic is unsigned 32-bit (host: total_segs < 2^31): the
// 64-bit divisions it replaces cost each block 2.3 us (tools/dw_trace.py).
struct DwBlkRange {
  unsigned begin, end;      // blocks of this workgroup
  unsigned n_samples;
  unsigned s_base;          // sample of the first block: slot 0 of the statistic table
};
__device__ __forceinline__ DwBlkRange dw_block_range(unsigned nblk, unsigned tsegs, unsigned segs_per_block, unsigned nsegx,
                                                     unsigned C) {
  DwBlkRange r;
  r.begin = (unsigned)((uint64_t)nblk * blockIdx.x / gridDim.x);
  r.end = (unsigned)((uint64_t)nblk * (blockIdx.x + 1) / gridDim.x);
  r.n_samples = tsegs / nsegx / C;
  const unsigned seg0 = r.begin * segs_per_block;
  r.s_base = (seg0 < tsegs ? seg0 : tsegs - 1) / nsegx / C;
  return r;
}

// Per-sample statistic: the workgroup's LDS table k_stat[kDwStatSlots] holds the maxima of samples s_base .. s_base + 15 as
// bit patterns (|x| >= 0 orders like an unsigned int); samples beyond it go to memory at once.  dw_stat_update is called per
// wavefront and block without a barrier (m: the lane's maximum, counted where is_out), dw_stat_flush once at the end.
// (SampleT: int or unsigned, as the form holds its sample index - the one-type version widens the index differently and costs
// the stride-2 four-columns-per-lane kernels two vector registers)
constexpr int kDwStatSlots = 16;
template <class SampleT>
__device__ __forceinline__ void dw_stat_update(unsigned* k_stat, unsigned s_base, SampleT sample, bool is_out, float m,
                                               int lane, float* stat_out) {
  const unsigned s0 = (unsigned)__builtin_amdgcn_readfirstlane((int)sample);
  const bool wave_uniform = __all(!is_out || (unsigned)sample == s0);
  if (wave_uniform) {
    const float wm = wave_max_nonneg(is_out ? m : 0.0f);
    if (lane == 0 && __float_as_uint(wm) != 0u) {
      const unsigned slot = s0 - s_base;
      if (slot < (unsigned)kDwStatSlots) atomicMax(&k_stat[slot], __float_as_uint(wm));
      else atomic_max_f32(stat_out + s0, wm);
    }
  } else if (is_out) {
    const unsigned slot = (unsigned)sample - s_base;
    if (slot < (unsigned)kDwStatSlots) atomicMax(&k_stat[slot], __float_as_uint(m));
    else atomic_max_f32(stat_out + sample, m);
  }
}
__device__ __forceinline__ void dw_stat_flush(const unsigned* k_stat, unsigned s_base, unsigned n_samples,
                                              float* stat_out) {
  __syncthreads();
  if (threadIdx.x < kDwStatSlots && k_stat[threadIdx.x] != 0u && s_base + threadIdx.x < n_samples)
    FQ_STAT_FLUSH_MAX(reinterpret_cast<unsigned*>(stat_out) + s_base + threadIdx.x, k_stat[threadIdx.x]);
}

// Loads are UNCONDITIONAL from clamped (always valid) addresses and masked afterwards with a bitwise AND — a
// `cond ? load : 0` select is turned back into a predicated load by hipcc (CodeGenPrepare sinks the load under a
// branch), which then waits vmcnt(0) right behind it and the prefetch ring is gone.
__device__ __forceinline__ float keep(float v, bool ok) { return __uint_as_float(__float_as_uint(v) & (ok ? 0xFFFFFFFFu : 0u)); }
__device__ __forceinline__ f4 keep4(f4 v, bool ok) {
  const unsigned mk = ok ? 0xFFFFFFFFu : 0u;
  f4 r;
  r.x = __uint_as_float(__float_as_uint(v.x) & mk);
  r.y = __uint_as_float(__float_as_uint(v.y) & mk);
  r.z = __uint_as_float(__float_as_uint(v.z) & mk);
  r.w = __uint_as_float(__float_as_uint(v.w) & mk);
  return r;
}
// The value the lane on the left / right holds, 0 for the edge lane of a plane.  The shift is taken by EVERY lane and masked
// afterwards: under a branch the edge lanes would be switched off, and a DPP read from a switched-off lane returns 0
__device__ __forceinline__ float left_of(float v, bool first) {
  const float t = lane_prev(v);
  return first ? 0.0f : t;
}
__device__ __forceinline__ float right_of(float v, bool last) {
  const float t = lane_next(v);
  return last ? 0.0f : t;
}

// Lanes of the register forms (one column, four columns, whole planes): a wavefront holds `segs` independent SEGMENTS; a
// segment is `sw` adjacent output columns of one plane plus its halo lanes.
struct DwColGeom {
  int C, H, W, Ho, Wo;
  int sw;       // output columns per segment
  int nsegx;    // segments per plane row
  int SEG;      // lanes per segment (sw + halo lanes)
  int segs;     // segments per wavefront
  int nts;      // cols4 form: nontemporal stores (an output the Infinity Cache cannot hold beside the other batches' tensors)
};

// Eight bytes per lane through a buffer resource (the whole-plane form; fq_common.h has the 4- and 16-byte ones)
__device__ __forceinline__ f2 buf_ld_2f32(fq_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void buf_st_2f32(fq_rsrc r, unsigned voff, unsigned soff, f2 v) {
  typedef unsigned v2u __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, (int)voff, (int)soff, 0);
}

// Epilogue of the depthwise kernels.  EPI 0: bias / BN / activation decided at run time (hipcc turns the wave-uniform
// branches into four selects per output); EPI 1 / 2: the fused-inference case - BN, no bias, ReLU / ReLU6 - in 3 / 4
// instructions.  Same operations in the same order either way.
constexpr int kEpiRuntime = 0, kEpiBnRelu = 1, kEpiBnRelu6 = 2;
// bit of the kernels' `act` argument (set by the library's own callers, run-time epilogue only): the per-channel `bias` vector
// MULTIPLIES the sum instead of being added - the dequantisation factor in_scale * w_scale of nn.Conv2D(quantized=True)'s
// depthwise layer, applied to the exact integer sum before a folded BatchNorm (its own multiply and add stay separate)
constexpr int kActBiasMul = 0x10;
// (ACT = false: a compile-time epilogue WITHOUT its activation - for a code output, where ReLU / ReLU6 and the consumer's clip
// are one median: clip(relu6(v), lo <= 0, hi) == med3(v, 0, min(6, hi)))
template <int EPI, bool ACT = true>
__device__ __forceinline__ float dw_finish(float acc, bool has_bias, float bch, bool has_bn, float bsc, float bsh, int act) {
  if (EPI == kEpiRuntime) {
    if (has_bias) acc = (act & kActBiasMul) ? acc * bch : acc + bch;
    if (has_bn) {
      acc = acc * bsc;
      acc = acc + bsh;
    }
    return act_rt(acc, act & 15);
  }
  acc = acc * bsc;
  acc = acc + bsh;
  if (!ACT) return acc;
  acc = fmaxf(acc, 0.0f);
  return EPI == kEpiBnRelu6 ? fminf(acc, 6.0f) : acc;
}
template <int EPI>
__device__ __forceinline__ f2 dw_finish2(f2 acc, bool has_bias, float bch, bool has_bn, float bsc, float bsh, int act) {
  if (EPI == kEpiRuntime) {
    acc.x = dw_finish<EPI>(acc.x, has_bias, bch, has_bn, bsc, bsh, act);
    acc.y = dw_finish<EPI>(acc.y, has_bias, bch, has_bn, bsc, bsh, act);
    return acc;
  }
  acc = acc * splat2(bsc);
  acc = acc + splat2(bsh);
  acc.x = fmaxf(acc.x, 0.0f);
  acc.y = fmaxf(acc.y, 0.0f);
  if (EPI == kEpiBnRelu6) {
    acc.x = fminf(acc.x, 6.0f);
    acc.y = fminf(acc.y, 6.0f);
  }
  return acc;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// in_flags bit of the library's own callers: `in_thr` is a range record (fq_common.h: kRangeMode), the weights are integer
// codes held in fp32 and the quantiser hands on CODES (multiply-back scale 1): the depthwise layer of nn.Conv2D(quantized=True)
constexpr unsigned kFlagRangeRecord = 0x100u;
constexpr unsigned kFlagBiasMultiplies = 0x200u;      // `bias` is the per-channel dequantisation factor (kActBiasMul)

// The launch of every form: zeroes the statistic, opens the profile scope, turns (quant, online) and epi into template
// arguments and launches kernel_for(quant_c, online_c, epi_c) with `geom...` between y and in_stat.
template <class KernelFor, class... Geom>
int dw_launch(const DwCall& d, int grid, size_t lds, KernelFor kernel_for, Geom... geom) {
  using std::integral_constant;
  if (d.stat_out && !d.prezeroed) FQ_HIP(hipMemsetAsync(d.stat_out, 0, d.n * sizeof(float), d.st));
  // algorithmic bytes: the layer's; moved: the statistic pass reads x and writes at most one byte per element of it
  const double in_bytes = 4.0 * (double)d.n * d.c * d.h * d.wdt, out_bytes = 4.0 * (double)d.n * d.c * d.ho * d.wo;
  ProfScope prof(FQ_KERNEL_DWCONV, in_bytes + out_bytes, d.st,
                 d.y ? -1.0 : in_bytes + (d.x_codes_out ? 0.25 * in_bytes : 0.0));
  float* const y_arg = d.y ? d.y : static_cast<float*>(d.x_codes_out);      // (the statistic pass takes its code buffer there)
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, d.st, d.x, d.w, d.bias, y_arg, geom..., d.in_stat, (int)d.n,
                       d.in_thr, d.levels, d.lo_neg, d.eps, d.out_current_max, d.bn_scale, d.bn_shift, d.act, d.stat_out);
  };
  auto with_epi = [&](auto quant_c, auto online_c) {
    if (d.epi == kEpiBnRelu) launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiBnRelu>{}));
    else if (d.epi == kEpiBnRelu6) launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiBnRelu6>{}));
    else launch(kernel_for(quant_c, online_c, integral_constant<int, kEpiRuntime>{}));
  };
  if (!d.quant) with_epi(std::false_type{}, std::false_type{});
  else if (d.online) with_epi(std::true_type{}, std::true_type{});
  else with_epi(std::true_type{}, std::false_type{});
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}
template <int V>
using dw_int = std::integral_constant<int, V>;

// Persistent grids: a block is what the four wavefronts of a workgroup do in one step (`segs` segments or planes each);
// every workgroup is resident at once and walks a contiguous range of blocks.
inline int64_t dw_blocks(int64_t total_segs, int segs) {
  const int64_t per_block = (int64_t)segs * (kBlock / 64);
  return (total_segs + per_block - 1) / per_block;
}
inline int dw_grid(int64_t nblk, int wg_per_cu) {
  const int64_t cap = (int64_t)num_cu() * wg_per_cu;
  return (int)(nblk < cap ? nblk : cap);
}

// Lanes of the register forms: a plane row of `units` compute lanes is cut into nsegx segments of sw lanes, each with `halo`
// lanes beside them, and a wavefront holds as many segments as fit.
inline DwColGeom dw_col_geom(const DwCall& d, int units, int halo) {
  DwColGeom cg = {};
  cg.C = (int)d.c;
  cg.H = (int)d.h;
  cg.W = (int)d.wdt;
  cg.Ho = (int)d.ho;
  cg.Wo = (int)d.wo;
  const int max_sw = 64 - halo;
  cg.nsegx = (units + max_sw - 1) / max_sw;
  cg.sw = (units + cg.nsegx - 1) / cg.nsegx;
  cg.SEG = cg.sw + halo;
  cg.segs = 64 / cg.SEG;
  return cg;
}
// ---- K2e / K2d, cols4 and cols: the sliding window with four columns / one column per lane ------------------------------------
// Both: every workgroup resident at once, each walking a contiguous range of blocks.  6 per CU: the kernels use ~100 scalar
// registers, and a CU admits 256-thread workgroups 8 at a time only up to 80 (MI355X_MICROARCH.md, residency) - with
// 8 per CU asked for, a quarter of the grid ran as a second, thin round (14x14 layers: 31.7 -> 28.0 us; capping the
// scalar registers at 80 instead makes all 8 resident and is no faster)
inline int dw_cols_grid(int64_t total_segs, const DwColGeom& cg) {
  static const int dw_wg_per_cu = env_int("FQ_DW_WG_PER_CU", 6);
  return dw_grid(dw_blocks(total_segs, cg.segs), dw_wg_per_cu);
}

}  // namespace

#endif  // FQ_DW_H_
