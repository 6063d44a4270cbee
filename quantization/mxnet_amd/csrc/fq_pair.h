// libfakequant — what the two kernels of a recompute pair share: the fused 1x1 + depthwise 3x3 launch (fq_pwdw.hip) and the
// statistic pass of a 1x1 (fq_pw_stat.hip).  Both take activations as the A operand of v_mfma_i32_32x32x32_i8 - a lane quantises
// sixteen fp32 values of its pixel into one fragment - and both launchers turn run-time values into template arguments.
// fq_mma.h's conventions and its rule: everything is __forceinline__ and takes the kernel's own values, and a helper lives here
// only while every instantiation keeps its VGPR, SGPR, LDS and scratch counts.  profiles/pair_units_one_of_each.txt is that
// comparison; it lists what the two kernels also have in common but keep as inline text, because a helper moved a count of the
// fused kernel: the weight fragments' copy to LDS, the depthwise constants' copy to LDS, the ring-phase loop.
#ifndef FQ_PAIR_H_
#define FQ_PAIR_H_

#include "fq_pw.h"

#include "fq_front_layout.h"
#include "fq_mma.h"

#include <climits>

namespace {

// ---- sixteen fp32 values -> one A fragment --------------------------------------------------------------------------------------
// four codes as the bytes of a dword.  NN: the clip range starts at 0 AND the divisor takes the fp32 quotient (fq_common.h:
// fq_nonneg, make_fast_quot) - five instructions per code; else the general form
template <bool NN>
__device__ __forceinline__ int pair_pack4(float a, float b, float c, float d, const QParams& q, const FastQuot& fq, int ubias,
                                          unsigned nn_xor) {
  if constexpr (NN) {
    unsigned u = (unsigned)fq_code_nonneg(a, q, fq);
    u |= (unsigned)fq_code_nonneg(b, q, fq) << 8;
    u |= (unsigned)fq_code_nonneg(c, q, fq) << 16;
    u |= (unsigned)fq_code_nonneg(d, q, fq) << 24;
    return (int)(u ^ nn_xor);
  } else {
    return fq_pack4<false>(a, b, c, d, q, ubias, nn_xor);
  }
}
// (the empty asm pins the fragment: the compiler otherwise sinks the quantisation below the loads issued after it)
template <bool NN>
__device__ __forceinline__ v4i pair_frag16(const float (&v)[16], const QParams& q, const FastQuot& fq, int ubias, unsigned nn_xor) {
  v4i f;
#pragma unroll
  for (int d = 0; d < 4; ++d) f[d] = pair_pack4<NN>(v[4 * d + 0], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3], q, fq, ubias, nn_xor);
  asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
  return f;
}

// ---- host: a run-time value as a compile-time one ---------------------------------------------------------------------------
// f(integral_constant<int, V>) for the V of Vs... that equals v; false when none does (nothing was called)
template <int... Vs, class F>
inline bool pair_pick(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

}  // namespace

#endif  // FQ_PAIR_H_
