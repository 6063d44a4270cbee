// libfakequant — the pieces the convolution kernels on v_mfma_i32_32x32x32_i8 share: the split 1x1 (fq_pw_split_kernel.h), the
// dense 3x3 (fq_conv3x3_kernel.h) and the folded shortcut (fq_pw_short.hip); the streaming 1x1 (fq_pw_stream.hip) takes the
// constants, the fall-back form (fq_pw_generic.hip) the statistic table.  What the kernels do differently on purpose - where the
// re-centring term joins the sum, scalar or packed fp32, the sliced 3x3's fp64 step - stays in the kernels.
// Everything is __forceinline__ and takes the kernel's own values.  The rule for what may live here: a helper must leave every
// instantiation's VGPR, SGPR, LDS and scratch counts what they were.  profiles/mma_shared_one_of_each.txt is that comparison, and
// lists the sites that keep their inline text because a helper moved a count (the constant tables, the B fragment, and - in the
// 3x3 and the streaming kernel - more).
#ifndef FQ_MMA_H_
#define FQ_MMA_H_

#include "fq_common.h"

namespace {

// ---- per-sample statistic table -------------------------------------------------------------------------------------------
// A workgroup's outputs touch few samples: their maxima are gathered in an LDS table k_stat[] (slot = sample - s_base, the bit
// pattern of a non-negative fp32 orders like an unsigned) and leave as ONE global atomic per touched sample; same-address
// global atomics serialise in L2 (profiles/r6_pwstat_atomics.txt).  A sample past the table goes straight to memory.
constexpr int kStatSlots = 8;

template <int SLOTS>
__device__ __forceinline__ void mma_stat_init(unsigned (&k_stat)[SLOTS]) {
  if (threadIdx.x < SLOTS) k_stat[threadIdx.x] = 0u;
}

// one lane = one pixel of sample `smp` with the maximum `m` >= 0 of its values.  A wavefront whose lanes all sit in one sample
// (the usual case) reduces first and sends one atomic; otherwise every lane sends its own.
template <int SLOTS>
__device__ __forceinline__ void mma_stat_update(unsigned (&k_stat)[SLOTS], float* __restrict__ stat_out, unsigned smp,
                                                unsigned s_base, float m) {
  const unsigned s0 = (unsigned)__builtin_amdgcn_readfirstlane((int)smp);
  if (__all(smp == s0)) {
    const float wm = wave_max_nonneg(m);
    if ((threadIdx.x & 63) == 0) {
      const unsigned slot = s0 - s_base;
      if (slot < (unsigned)SLOTS) atomicMax(&k_stat[slot], __float_as_uint(wm));
      else atomic_max_f32(stat_out + s0, wm);
    }
  } else {
    const unsigned slot = smp - s_base;
    if (slot < (unsigned)SLOTS) atomicMax(&k_stat[slot], __float_as_uint(m));
    else atomic_max_f32(stat_out + smp, m);
  }
}

// after the barrier that closes the updates: slots that hold something, of samples that exist (the last workgroup's table
// reaches past the batch of cols / HW samples; the division is only reached by the few lanes that have something to flush)
template <int SLOTS, class Cols>
__device__ __forceinline__ void mma_stat_flush(unsigned (&k_stat)[SLOTS], float* __restrict__ stat_out, unsigned s_base,
                                               Cols cols, unsigned HW) {
  if (threadIdx.x < SLOTS && k_stat[threadIdx.x] != 0u && s_base + threadIdx.x < (unsigned)(cols / HW))
    FQ_STAT_FLUSH_MAX(reinterpret_cast<unsigned*>(stat_out) + s_base + threadIdx.x, k_stat[threadIdx.x]);
}

// ---- the output's quantiser ---------------------------------------------------------------------------------------------------
// OUT16: y is a C16 code tensor quantised with the CONSUMER's threshold out_thr; DUAL: y stays fp32 and a second output receives
// the codes of the same values under dual_thr.  Neither: all zero (fq_nonneg() is false for it).
template <bool OUT16, bool DUAL>
__device__ __forceinline__ QParams mma_out_qparams(const float* __restrict__ out_thr, const float* __restrict__ dual_thr,
                                                   float levels, int lo_neg, float eps) {
  QParams q2;
  q2.lo = q2.hi = q2.denom = q2.scale = 0.0f;
  q2.rden = 0.0;
  if (OUT16) q2 = make_qparams(out_thr[0], levels, lo_neg != 0, eps);
  if (DUAL) q2 = make_qparams(dual_thr[0], levels, lo_neg != 0, eps);
  return q2;
}

// FOLD - a code output behind a compile-time ReLU / ReLU6: activation and the consumer's clip are ONE median - clip(relu6(v), lo
// <= 0, hi) == med3(v, 0, min(6, hi)) for every v, NaN -> 0 on both sides - and the statistic max_i relu6(v_i) ==
// min(max(0, max_i v_i), 6) is taken from the raw values (m = fmaxf(m, v) from 0) and clamped once, by the kernel (a v_med3
// less per output)
template <int ACT_M, bool FOLD>
__device__ __forceinline__ QParams mma_fold(const QParams& q2) {
  QParams qc = q2;
  if (FOLD) {
    qc.lo = 0.0f;
    if (ACT_M == FQ_ACT_RELU6) qc.hi = fminf(q2.hi, 6.0f);
  }
  return qc;
}

// The epilogue a launch takes: body(bias_c, bn_c, act_c, nn2_c) with integral_constants - BatchNorm, no bias and ReLU / ReLU6 /
// no activation (the fused-inference cases) as compile-time values 0 / 1 / act, everything else as -1 / -1 / -1 = "look at
// fbias / has_bn / act".  Only a kernel that writes codes (CODES) is instantiated twice: nn2_c is true where the values its
// output quantiser clips cannot be negative - a ReLU stands in front of it, or the consumer's range starts at 0 - and the
// five-instruction quantiser of fq_common.h writes them.
template <bool CODES, class Body>
__device__ __forceinline__ void mma_epilogue_dispatch(const float* fbias, bool has_bn, int act, const QParams& q2,
                                                      std::integral_constant<bool, CODES>, Body body) {
  using std::integral_constant;
  auto go = [&](auto bias_c, auto bn_c, auto act_c, bool nn2) __attribute__((always_inline)) {
    if constexpr (CODES) {
      if (nn2) body(bias_c, bn_c, act_c, std::true_type{});
      else body(bias_c, bn_c, act_c, std::false_type{});
    } else {
      body(bias_c, bn_c, act_c, std::false_type{});
    }
  };
  const bool nn2_relu = q2.denom > 0.0f, nn2_any = fq_nonneg(q2);
  if (fbias == nullptr && has_bn && act == FQ_ACT_RELU)
    go(integral_constant<int, 0>{}, integral_constant<int, 1>{}, integral_constant<int, FQ_ACT_RELU>{}, nn2_relu);
  else if (fbias == nullptr && has_bn && act == FQ_ACT_RELU6)
    go(integral_constant<int, 0>{}, integral_constant<int, 1>{}, integral_constant<int, FQ_ACT_RELU6>{}, nn2_relu);
  else if (fbias == nullptr && has_bn && act == FQ_ACT_NONE)
    go(integral_constant<int, 0>{}, integral_constant<int, 1>{}, integral_constant<int, FQ_ACT_NONE>{}, nn2_any);
  else
    go(integral_constant<int, -1>{}, integral_constant<int, -1>{}, integral_constant<int, -1>{}, nn2_any);
}

// ---- work order and output resources ----------------------------------------------------------------------------------------
// XCD-aware order: workgroup b runs on XCD b % 8 (each XCD has its own L2), and a 32-pixel tile of a 14x14 / 7x7 plane is 128
// bytes that are NOT line-aligned, so neighbouring tiles share their first / last cache line of every channel: every XCD gets a
// CONTIGUOUS range of items so that both halves of such a line meet in one L2.  false: this workgroup has nothing to do.
__device__ __forceinline__ bool mma_xcd_item(int64_t items, unsigned& item) {
  const unsigned per = ((unsigned)items + 7u) >> 3;
  item = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  return (blockIdx.x >> 3) < per && item < (unsigned)items;
}

// A wavefront's window on an output-shaped tensor: from (the workgroup's first sample s_base, `skip` bytes into it - the
// wavefront's first channel tile) to the end of the tensor, at most 2 GiB - 1.  Lane offsets are relative to it.  Because it is
// bounded BELOW 2 GiB, the lane offset kOobOffset is out of range whatever the scalar offset adds: that is how the channels past
// Cout of a PARTIAL channel tile are masked - the hardware drops the store and returns 0 for the load, no branch, no exec
// juggling.  The residual operand's loads need the mask as much as the stores: the window runs to the end of the tensor, so
// an unmasked load of a channel past Cout fetches the NEXT sample's channels 0.. and, the channel's constants being all zero,
// carries that foreign value into the statistic.
constexpr unsigned kOobOffset = 0x80000000u;
__device__ __forceinline__ int64_t mma_out_bytes(int64_t s_base, int64_t n_samp, int64_t samp_bytes, int64_t skip) {
  const int64_t b = (n_samp - s_base) * samp_bytes - skip;
  return b < 0x7FFFFFFFll ? b : 0x7FFFFFFFll;
}
// (`bytes`: mma_out_bytes of the same tensor, or 0 for an empty window - the kernel has no such tensor)
__device__ __forceinline__ fq_rsrc mma_out_rsrc(const void* base, int64_t s_base, int64_t samp_bytes, int64_t skip, int64_t bytes) {
  return make_rsrc(reinterpret_cast<const char*>(base) + s_base * samp_bytes + skip, bytes);
}

}  // namespace

#endif  // FQ_MMA_H_
