// libfakequant — what the four grouped 3x3 kernels on int8 codes share: K2g (fq_gconv3x3.hip), K2g2 (fq_gconv3x3_s2.hip), K2gc
// (fq_gconv3x3_16.hip) and K2g2c (fq_gconv3x3_s2_16.hip).  Each unit keeps what is its own: the fill schedule of the next
// region, the tap addressing of its panel(s) and its store.  Here: the geometry, the LDS budget, the work-item decode, a block's
// region, the resident A fragments, the constant tables, the sixteen-value quantiser, one (tap, tile) multiply, the call
// description and the launch; and for the four entry points the argument checks, the plan (slabs, bands, grid, LDS) and the
// zeroing of the statistic.
// fq_mma.h's conventions and its rule: device helpers are __forceinline__ and take the kernel's own values, and a helper lives
// here only while every instantiation keeps its VGPR, SGPR, LDS and scratch counts.  profiles/gconv_shared_one_of_each.txt is
// that comparison, and says what the kernels also have in common but keep as inline text (the epilogue bodies).
#ifndef FQ_GCONV_H_
#define FQ_GCONV_H_

#include "fq_mma.h"

namespace {

// ---- geometry and LDS budget ------------------------------------------------------------------------------------------------
// One field set for the four kernels.  Stride 1: the output plane IS the input plane (Ho, Wo, HWo = H, W, HW).  The fp32 forms
// leave the C16 fields zero.  Pixel blocks, positions and cols count OUTPUT pixels.
struct GcGeom {
  int C, H, W, HW;           // the input plane
  int Ho, Wo, HWo;           // the output plane
  int NSLAB, CS;             // slabs of 32 channels; slab groups = ceil(NSLAB / WC)
  int NB;                    // pixel blocks per band
  int RT, ROW;               // region tiles of 32 positions; bytes per position in a panel
  int zoff, evenw;           // evenw (stride 2, fp32 in): both columns of a pair with one 8-byte load
  int CB;                    // 16-channel blocks of a C16 tensor = C / 16
  int st4;                   // K2gc, OUT16: 4-byte pieces instead of whole vectors
  float out_levels;
  int out_lo_neg, out_zoff;
  int64_t cols, nblocks, items;   // n * HWo; pixel blocks of 32 PT; bands * CS
};

constexpr int kGcKTS = 10;                        // weight fragments per channel tile in fq_weight_codes' buffer (nine are fetched)
constexpr size_t kGcLdsMax = 150 * 1024;

// A block's region is the block and its halo: stride 1 reads W + 1 pixels on either side into ONE panel, stride 2 reads Wo + 1
// positions in front into FOUR parity-phase panels.  `wo`: the width of the output plane.
constexpr int gc_halo(int stride, int wo) { return stride == 1 ? 2 * wo + 2 : wo + 1; }
constexpr int gc_region_tiles(int stride, int pt, int wo) { return (32 * pt + gc_halo(stride, wo) + 31) / 32; }
// two regions (the one the multiplies read, the one being filled) and five per-channel constant tables
constexpr size_t gc_lds_bytes(int stride, int wc, int pt, int wo) {
  return 2 * (size_t)(stride == 1 ? 1 : 4) * gc_region_tiles(stride, pt, wo) * 32 * (32 * wc + 16) +
         (size_t)(32 * wc) * 5 * sizeof(float);
}

// ---- device -----------------------------------------------------------------------------------------------------------------
// two neighbouring fp32 values with one buffer_load_dwordx2 (as ONE 64-bit integer: the halves are taken by shifts)
__device__ __forceinline__ uint64_t gc_ld_b64(fq_rsrc r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}

// A work item (mma_xcd_item) is (a band of NB consecutive pixel blocks of BPX output pixels, WC consecutive slabs).  (The
// kernels keep their own early return in front of this: with mma_xcd_item in here K2g2c <2, 2, 4, true, true> took a VGPR more.)
template <int WC, int BPX>
__device__ __forceinline__ void gc_work_item(const GcGeom& g, unsigned HWo, unsigned item, int& slab0, int& ch0, unsigned& blk0,
                                               unsigned& blk1, unsigned& s_band) {
  const unsigned band = item / (unsigned)g.CS, sg = item - band * (unsigned)g.CS;
  slab0 = (int)sg * WC;                                                 // first slab of the workgroup
  ch0 = slab0 * 32;
  blk0 = band * (unsigned)g.NB;
  blk1 = blk0 + (unsigned)g.NB < (unsigned)g.nblocks ? blk0 + (unsigned)g.NB : (unsigned)g.nblocks;
  s_band = blk0 * (unsigned)BPX / HWo;                                  // first sample the band's OUTPUT touches
}

// the five per-channel constant tables of a workgroup's NCH channels, behind the panels in the dynamic LDS
struct GcTables {
  float *sxw, *bsc, *bsh, *bias;
  int* zs;
};
template <int NCH>
__device__ __forceinline__ GcTables gc_tables(unsigned char* behind_panels) {
  GcTables c;
  c.sxw = reinterpret_cast<float*>(behind_panels);
  c.bsc = c.sxw + NCH;
  c.bsh = c.bsc + NCH;
  c.bias = c.bsh + NCH;
  c.zs = reinterpret_cast<int*>(c.bias + NCH);
  return c;
}
template <int NCH, int THREADS>
__device__ __forceinline__ void gc_fill_tables(const GcTables& c, int ch0, int C, float sx, int zoff, const float* wscale, const int* wsum,
                                               const float* bias, const float* bn_scale, const float* bn_shift, bool has_bn) {
  for (int i = threadIdx.x; i < NCH; i += THREADS) {
    const bool ok = ch0 + i < C;
    const int ic = ok ? ch0 + i : 0;
    c.sxw[i] = ok ? sx * wscale[ic] : 0.0f;
    c.zs[i] = ok ? zoff * wsum[ic] : 0;
    c.bias[i] = ok && bias != nullptr ? bias[ic] : 0.0f;
    c.bsc[i] = has_bn && ok ? bn_scale[ic] : (ok ? 1.0f : 0.0f);
    c.bsh[i] = has_bn && ok ? bn_shift[ic] : 0.0f;
  }
}

// The region of block blk: its first position jr0 (may be < 0; Wo + 1 in front of the block), the first sample it touches and a
// window on x from that sample on.  Lane offsets are relative to it.
struct GcRegion {
  fq_rsrc xr;
  int jr0;
  unsigned n_base;
};
__device__ __forceinline__ GcRegion gc_region_of(const void* x, unsigned blk, unsigned bpx, unsigned Wo, unsigned HWo, int64_t x_samp,
                                                 int64_t n_samp) {
  GcRegion r;
  r.jr0 = (int)(blk * bpx) - (int)Wo - 1;
  r.n_base = (unsigned)(r.jr0 < 0 ? 0 : r.jr0) / HWo;
  r.xr = make_rsrc(reinterpret_cast<const char*>(x) + r.n_base * x_samp, (n_samp - r.n_base) * x_samp);
  return r;
}

// a wavefront's nine A fragments - 36 VGPRs, resident for the whole band; a slab past the layer (!mine) reads zeros
__device__ __forceinline__ void gc_load_afrag(const int8_t* wfrag, int slab, bool mine, int lane, v4i (&afrag)[9]) {
  const fq_rsrc wr = make_rsrc(wfrag + (((int64_t)slab * kGcKTS) << 10), mine ? 9 * 1024 : 0);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) afrag[tap] = buf_ld_v4i(wr, (unsigned)lane * 16u, (unsigned)(tap << 10));
}

// sixteen fp32 values of a pixel -> sixteen codes.  Non-negative quotients - unsigned activations - take the 5-instruction
// quantiser of fq_common.h.  (The empty asm pins the codes: the compiler otherwise sinks the quantisation below later loads.)
__device__ __forceinline__ v4i gc_quant16(const float (&v)[16], bool nonneg, const QParams& q, int ubias, unsigned nn_xor) {
  v4i f;
  if (nonneg) {
#pragma unroll
    for (int d = 0; d < 4; ++d) f[d] = fq_pack4<true>(v[4 * d + 0], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3], q, ubias, nn_xor);
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) f[d] = fq_pack4<false>(v[4 * d + 0], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3], q, ubias, nn_xor);
  }
  asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
  return f;
}

// one (tap, pixel tile): the B fragment from the panel row - the code 0 (zb) where the tap leaves the image - and the multiply
__device__ __forceinline__ void gc_mma_tap(const unsigned char* row, bool tv, int zb, const v4i& a, v16i& acc) {
  const v4i raw = *reinterpret_cast<const v4i*>(row);
  v4i b;
  b[0] = tv ? raw[0] : zb;
  b[1] = tv ? raw[1] : zb;
  b[2] = tv ? raw[2] : zb;
  b[3] = tv ? raw[3] : zb;
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
}

// ---- host: the call and its launch ------------------------------------------------------------------------------------------
// what an entry point hands its kernel (x, y: fp32 planes or C16 code tensors; out_thr: the C16 forms only)
struct GcCall {
  const void* x; const int8_t* wfrag; const float* wscale; const int32_t* wsum; const float* bias; void* y;
  const float* in_stat; int n; const float* in_thr; float levels; int lo_neg; float* out_current_max;
  const float* bn_scale; const float* bn_shift; int act; float* stat_out; const float* out_thr; int cg;
};

template <class X, class Y, class... OutThr>
using GcKernel = void (*)(const X*, const int8_t*, const float*, const int*, const float*, Y*, GcGeom, const float*, int, const float*,
                          float, int, float, float*, const float*, const float*, int, float*, OutThr...);

// Launches Kernel (threads per workgroup, the plan's grid and LDS bytes) and notes what ran: `vals` are the family's values of
// fakequant.h, from the template arguments of the instantiation.  OutThr is empty (fp32 forms) or the out_thr pointer.
template <auto Kernel, class X, class Y, class... OutThr>
int gc_launch_as(GcKernel<X, Y, OutThr...>, const char* entry, int threads, int family, std::initializer_list<int> vals, const GcCall& a,
                 const GcGeom& g, int64_t grid, size_t lds, hipStream_t st) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)kGcLdsMax) == hipSuccess;
  FQ_REQUIRE(attr_ok, "%s: cannot raise the dynamic LDS limit", entry);
  static_assert(sizeof...(OutThr) <= 1, "fp32 form, or one out_thr");
  if constexpr (sizeof...(OutThr) == 0)
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds, st, static_cast<const X*>(a.x), a.wfrag, a.wscale,
                       (const int*)a.wsum, a.bias, static_cast<Y*>(a.y), g, a.in_stat, a.n, a.in_thr, a.levels, a.lo_neg, kEps,
                       a.out_current_max, a.bn_scale, a.bn_shift, a.act, a.stat_out);
  else
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds, st, static_cast<const X*>(a.x), a.wfrag, a.wscale,
                       (const int*)a.wsum, a.bias, static_cast<Y*>(a.y), g, a.in_stat, a.n, a.in_thr, a.levels, a.lo_neg, kEps,
                       a.out_current_max, a.bn_scale, a.bn_shift, a.act, a.stat_out, a.out_thr);
  note_launch(FQ_KERNEL_GCONV3X3, family, vals);
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}
template <auto Kernel>
int gc_launch(const char* entry, int threads, int family, std::initializer_list<int> vals, const GcCall& a, const GcGeom& g,
              int64_t grid, size_t lds, hipStream_t st) {
  return gc_launch_as<Kernel>(Kernel, entry, threads, family, vals, a, g, grid, lds, st);
}

// ---- host: what the four entry points check and plan ----------------------------------------------------------------------------
// An entry point: its name (every message begins with it), where a dense layer goes instead (or nullptr), stride, widest plane,
// and whether either side may be a C16 tensor (then y is stored with 16-byte vectors and must be aligned as x is).
struct GcEntry {
  const char* name;
  const char* dense;
  int stride, max_w;
  bool c16;
};

inline int gc_supported(int64_t cin, int64_t cout, int64_t groups) {
  if (cin != cout || cin <= 0 || cin % 32 != 0 || groups <= 1 || cin % groups != 0) return 0;
  const int64_t cg = cin / groups;
  return (cg == 4 || cg == 8 || cg == 16 || cg == 32) ? 1 : 0;
}

// The checks all four share, on the call as the entry point received it (a.act still carries FQ_STAT_PREZEROED: stripped here,
// reported in `prezeroed`).  Also fills the call's quantiser values of the input.
inline int gc_check(const GcEntry& e, GcCall& a, const int8_t* wcodes, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w,
                    int in_width, unsigned in_flags, bool& prezeroed) {
  const int64_t ho = e.stride == 1 ? h : (h - 1) / 2 + 1, wo = e.stride == 1 ? w : (w - 1) / 2 + 1;
  FQ_REQUIRE(a.x && wcodes && a.wscale && a.wsum && a.y, "%s: null pointer", e.name);
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && n * ho * wo < (1ll << 31) - 4096, "%s: bad shape", e.name);
  FQ_REQUIRE(gc_supported(c, c, groups), "%s: %lld channels in %lld groups: the channel count must be a multiple of 32 and a group "
             "4, 8, 16 or 32 channels wide%s%s%s", e.name, (long long)c, (long long)groups, e.dense ? " (groups == 1: " : "",
             e.dense ? e.dense : "", e.dense ? ")" : "");
  FQ_REQUIRE(w <= e.max_w, "%s: planes up to %d pixels wide (got %lld)", e.name, e.max_w, (long long)w);
  FQ_REQUIRE(a.in_stat != nullptr || a.in_thr != nullptr, "%s: give in_stat (online), in_thr (offline) or both (offline, the "
             "statistic only feeds out_current_max)", e.name);
  FQ_REQUIRE(a.in_thr != nullptr || a.out_current_max != nullptr, "%s: online mode needs out_current_max", e.name);
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "%s: input width %d does not fit int8 codes", e.name, in_width);
  FQ_REQUIRE(!(in_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "%s: unsupported activation flags", e.name);
  FQ_REQUIRE((a.bn_scale == nullptr) == (a.bn_shift == nullptr), "%s: bn_scale and bn_shift go together", e.name);
  prezeroed = (a.act & FQ_STAT_PREZEROED) != 0;
  a.act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(a.act >= FQ_ACT_NONE && a.act <= FQ_ACT_RELU6, "%s: unknown activation %d", e.name, a.act);
  FQ_REQUIRE(aligned16(wcodes) && aligned16(a.x) && (!e.c16 || aligned16(a.y)), "%s: x%s and wcodes must be 16-byte aligned", e.name,
             e.c16 ? ", y" : "");
  a.n = (int)n;
  a.levels = act_levels(in_width, in_flags);
  a.lo_neg = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  a.cg = (int)(c / groups);
  return FQ_OK;
}

// a C16 output: the consumer's quantiser into the geometry (the fp32 forms leave it zero)
inline int gc_out_quant(const GcEntry& e, bool out16, int out_width, unsigned out_flags, GcGeom& g) {
  g.out_levels = 0.0f; g.out_lo_neg = 0; g.out_zoff = 0;
  if (!out16) return FQ_OK;
  FQ_REQUIRE(out_width >= 2 && out_width <= 8, "%s: output width %d does not fit int8 codes", e.name, out_width);
  FQ_REQUIRE(!(out_flags & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "%s: unsupported output flags", e.name);
  g.out_levels = act_levels(out_width, out_flags);
  g.out_lo_neg = (out_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  g.out_zoff = (out_flags & FQ_ACT_SIGNED) ? 0 : 128;
  return FQ_OK;
}

// slabs of 32 channels a workgroup takes: two where the layer has them
inline int gc_slabs_per_group(int64_t c) { return c >= 64 ? 2 : 1; }

// The plan of a checked call with blocks of pt pixel tiles: geometry, grid, LDS bytes, and the call's fragment-major weights.
// The band is nb_first blocks per workgroup while that leaves two workgroups per compute unit, else two - never one: a band of
// one block has nothing to load under its multiplies - and `tune` (the entry's own FQ_*_NB knob, read per call) overrides it.
// in_bytes / out_bytes: 4 (fp32 planes) or 1 (C16 codes) per element.
inline int gc_plan(const GcEntry& e, GcCall& a, const int8_t* wcodes, int64_t n, int64_t c, int64_t h, int64_t w, unsigned in_flags,
                   int pt, int nb_first, int tune, int in_bytes, int out_bytes, GcGeom& g, int64_t& grid, size_t& lds) {
  const int64_t ho = e.stride == 1 ? h : (h - 1) / 2 + 1, wo = e.stride == 1 ? w : (w - 1) / 2 + 1;
  const int64_t hwi = h * w, hwo = ho * wo;
  const int blockpx = 32 * pt, wc = gc_slabs_per_group(c), rp = blockpx + gc_halo(e.stride, (int)wo);
  // 32-bit lane offsets count from the first sample a block's region (input) or the block itself (output) touches; stride 1
  // asks the region's span of the output as well, as it always has
  const int64_t in_span = rp / hwo + 2, out_span = e.stride == 1 ? in_span : blockpx / hwo + 2;
  FQ_REQUIRE(in_span * c * hwi * in_bytes < (1ll << 31) && out_span * c * hwo * out_bytes < (1ll << 31),
             "%s: a pixel block and its halo must stay within 2 GiB of their first sample", e.name);
  const int64_t row_pad = 320, rows_pad = (c + 63) / 64 * 64;            // fq_weight_codes' buffer of the (C, 3, 3, 32) filter
  a.wfrag = wcodes + rows_pad * row_pad;                                // its fragment-major copy
  g.C = (int)c; g.H = (int)h; g.W = (int)w; g.HW = (int)hwi;
  g.Ho = (int)ho; g.Wo = (int)wo; g.HWo = (int)hwo;
  g.NSLAB = (int)(c / 32); g.CS = (g.NSLAB + wc - 1) / wc;
  g.cols = n * hwo; g.nblocks = (g.cols + blockpx - 1) / blockpx;
  int nb = nb_first;
  if (((g.nblocks + nb - 1) / nb) * g.CS < 2 * (int64_t)num_cu()) nb = 2;
  if (tune >= 1 && tune <= 64) nb = tune;
  g.NB = nb;
  g.items = ((g.nblocks + nb - 1) / nb) * g.CS;
  g.RT = gc_region_tiles(e.stride, pt, (int)wo); g.ROW = 32 * wc + 16;
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  g.evenw = w % 2 == 0 ? 1 : 0;                                           // (x is 16-byte aligned: every pair of columns 8-byte)
  g.CB = (int)(c / 16); g.st4 = 0;
  g.out_levels = 0.0f; g.out_lo_neg = 0; g.out_zoff = 0;
  grid = (g.items + 7) / 8 * 8;
  FQ_REQUIRE(grid < (1ll << 31), "%s: too many pixel blocks", e.name);
  lds = gc_lds_bytes(e.stride, wc, pt, (int)wo);
  FQ_REQUIRE(lds <= kGcLdsMax, "%s: two regions of %d positions x %d channels do not fit LDS (planes up to %d wide)", e.name, rp,
             32 * wc, e.max_w);
  return FQ_OK;
}

// stat_out starts at zero unless the caller said it is (FQ_STAT_PREZEROED).  A kernel, not a memset node: safe under graph capture.
inline int gc_zero_stat(float* stat_out, bool prezeroed, int64_t n, hipStream_t st) {
  if (stat_out && !prezeroed) {
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stat_out, n, 0.0f);
    FQ_LAUNCH_CHECK();
  }
  return FQ_OK;
}

}  // namespace

#endif  // FQ_GCONV_H_
