/*
 * fakequant_host.h — the SAME entry points as fakequant.h with a `_host` suffix, taking HOST pointers and running on
 * the CPU cores (C++ / OpenMP).  SURVEY.md 8(b)/8(d): "identical-signature *_host CPU entry points for the baseline
 * timing".
 *
 * These are NOT part of the product: they are implemented by oracle/libfq_host.so (built from oracle/fq_host.cpp by
 * oracle/Makefile), a C restatement of the reference's algorithm that is test infrastructure.  Only tests/,
 * __graft_entry__.smoke() and bench.py's `cpu_baseline` leg load it; libfakequant.so has no CPU path and
 * quantization/mxnet_amd refuses host tensors.  Two uses:
 *   - the CPU baseline of bench.py: the reference's arithmetic on all host cores (`cpu_baseline.kind = "port"`);
 *   - a fast oracle for parity checks at BASELINE's full sizes (the numpy oracle needs minutes there); it is itself
 *     pinned bit-for-bit against oracle/fq_oracle.py and the golden vectors in tests/test_host_oracle.py.
 *
 * Conventions as in fakequant.h: int status (0 = ok), `fq_last_error_host()`; `stream` is accepted and ignored; `ws`
 * may be NULL (scratch is allocated internally).  Results are bit-identical to libfakequant.so on the same inputs for
 * every function below; the arithmetic each one restates is documented at its twin in fakequant.h.
 */
#ifndef FAKEQUANT_HOST_H_
#define FAKEQUANT_HOST_H_

#include "fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* fq_last_error_host(void);
int fq_version_host(void);
/* threads OpenMP will use (after fq_set_threads_host(k), k > 0; k <= 0 restores the default = all cores) */
int fq_threads_host(void);
int fq_set_threads_host(int k);

int fq_absmax_per_sample_host(const float* x, int64_t n, int64_t inner, unsigned flags, float* out_max,
                              fqStream_t stream);
int fq_batch_mean_host(const float* v, int64_t n, float* out, fqStream_t stream);
int fq_batch_mean_rows_host(const float* v, int64_t rows, int64_t n, int64_t row_stride, float* out,
                            fqStream_t stream);
int fq_stat_rows_sum_host(const float* v, int64_t rows, int64_t n, int64_t row_stride, double* out, fqStream_t stream);
int fq_mean_from_sums_host(const double* sums, int64_t rows, float* out, fqStream_t stream);
int fq_batch_mean_gathered_host(const float* packs, int world, int64_t stride, float* out, fqStream_t stream);
int fq_fake_quant_online_host(const float* x, float* y, int64_t n, int64_t inner, int width, unsigned flags,
                              float* out_current_max, int32_t* codes, void* ws, fqStream_t stream);
int fq_fake_quant_offline_host(const float* x, float* y, int64_t n, int64_t inner, const float* threshold, int width,
                               unsigned flags, float* out_current_max, int32_t* codes, void* ws, fqStream_t stream);
int fq_fake_quant_online_prestat_host(const float* x, float* y, int64_t n, int64_t inner, const float* stat,
                                      int width, unsigned flags, float* out_current_max, int32_t* codes,
                                      fqStream_t stream);
int fq_bn_act_stat_host(const float* x, float* y, int64_t n, int64_t c, int64_t hw, const float* scale,
                        const float* shift, int act, float* stat_out, fqStream_t stream);
int fq_bn_act_maxpool_stat_host(const float* x, float* y, int64_t n, int64_t c, int64_t h, int64_t w,
                                const float* scale, const float* shift, int act, float* stat_out, fqStream_t stream);
int fq_add_act_stat_host(const float* a, const float* b, float* y, int64_t n, int64_t inner, int act, float* stat_out,
                         fqStream_t stream);
/* (the producers that bin what they store: by definition the pass above followed by fq_histogram_accumulate_host over y) */
int fq_bn_act_stat_hist_host(const float* x, float* y, int64_t n, int64_t c, int64_t hw, const float* scale,
                             const float* shift, int act, float* stat_out, const float* hist_max, int bins, uint64_t* hist,
                             uint32_t* neg_count, fqStream_t stream);
int fq_bn_add_act_stat_host(const float* x, const float* residual, float* y, int64_t n, int64_t c, int64_t hw,
                            const float* scale, const float* shift, int act, float* stat_out, fqStream_t stream);
int fq_bn_add_act_stat_hist_host(const float* x, const float* residual, float* y, int64_t n, int64_t c, int64_t hw,
                                 const float* scale, const float* shift, int act, float* stat_out, const float* hist_max,
                                 int bins, uint64_t* hist, uint32_t* neg_count, fqStream_t stream);
int fq_add_act_stat_hist_host(const float* a, const float* b, float* y, int64_t n, int64_t inner, int act, float* stat_out,
                              const float* hist_max, int bins, uint64_t* hist, uint32_t* neg_count, fqStream_t stream);
int fq_global_avg_pool_stat_host(const float* x, float* y, int64_t n, int64_t c, int64_t hw, int flags,
                                 float* stat_out, fqStream_t stream);
int fq_gemm_i8_codes_host(const int8_t* xcodes, const int8_t* wcodes, const int32_t* wsum, int32_t* out, int64_t n,
                          int64_t l, int64_t k_pad, int64_t cout, int zoff, fqStream_t stream);
int fq_eval_counters_host(const float* logits, const int64_t* labels, int64_t n, int64_t classes, float* counters,
                          fqStream_t stream);
int fq_stem_conv3x3s2_host(const float* x, const float* w_tap_major, const float* bias, float* y, int64_t n,
                           int64_t cin, int64_t cout, int64_t h, int64_t w, const float* bn_scale,
                           const float* bn_shift, int act, float* stat_out, fqStream_t stream);
int fq_stem_conv3x3s2_c16_host(const float* x, const float* w_tap_major, const float* bias, void* y16, int64_t n, int64_t cin,
                               int64_t cout, int64_t h, int64_t w, const float* bn_scale, const float* bn_shift, int act,
                               float* stat_out, const float* out_thr, int out_width, unsigned out_flags, fqStream_t stream);
int fq_stem_conv7x7s2_host(const float* x, const float* w_tap_major, const float* bias, float* y, int64_t n,
                           int64_t cin, int64_t cout, int64_t h, int64_t w, const float* bn_scale,
                           const float* bn_shift, int act, float* stat_out, fqStream_t stream);
int fq_stem_conv7x7s2_pool_host(const float* x, const float* w_tap_major, const float* bias, float* y, int64_t n,
                                int64_t cin, int64_t cout, int64_t h, int64_t w, const float* bn_scale,
                                const float* bn_shift, int act, float* stat_out, fqStream_t stream);
int fq_dwconv3x3_host(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                      int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width,
                      unsigned in_flags, float* out_current_max, const float* bn_scale, const float* bn_shift, int act,
                      float* stat_out, fqStream_t stream);
/* codes: only the row-major half [rows_pad][row_pad] is written / read on the host (no MFMA fragment copy). */
int fq_weight_codes_host(const float* w, int64_t rows, int64_t row_len, int rows_per_scale, int width,
                         int64_t row_pad, int64_t rows_pad, int8_t* codes, float* scales, int32_t* rowsum, void* ws,
                         fqStream_t stream);
int fq_pwconv_i8_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                      const float* bias, float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t hw,
                      const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                      float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                      void* ws, fqStream_t stream);
int fq_pwconv_i8_strided_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                              const float* bias, float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout,
                              int64_t h, int64_t w, int stride, const float* in_stat, const float* in_thr, int in_width,
                              unsigned in_flags, float* out_current_max, const float* bn_scale, const float* bn_shift,
                              int act, float* stat_out, const float* residual, void* ws, fqStream_t stream);
int fq_pwconv_i8_shortcut_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                               float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t hw, const float* in_stat,
                               const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                               const float* bn_scale, const float* bn_shift, int act, float* stat_out, const float* x2,
                               const int8_t* wcodes2, const float* wscale2, const int32_t* wsum2, int64_t cin2, int64_t cin2_pad,
                               const float* in_stat2, const float* in_thr2, int in_width2, unsigned in_flags2,
                               float* out_current_max2, const float* bn_scale2, const float* bn_shift2, fqStream_t stream);
int fq_pwconv_i8_shortcut_c16_host(const void* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                                   float* y, void* y16, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t hw,
                                   const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                                   float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                                   const void* x2, int x2_is_c16, const int8_t* wcodes2, const float* wscale2, const int32_t* wsum2,
                                   int64_t cin2, int64_t cin2_pad, const float* in_stat2, const float* in_thr2, int in_width2,
                                   unsigned in_flags2, float* out_current_max2, const float* bn_scale2, const float* bn_shift2,
                                   const float* out_thr, int out_width, unsigned out_flags, fqStream_t stream);
int fq_pwconv_i8_gap_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                          float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t hw, const float* in_stat,
                          const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                          const float* bn_shift, int act, float* stat_out, const float* residual, void* ws, fqStream_t stream);
int fq_pwconv_i8_sub2_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                           float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t h, int64_t w,
                           const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                           float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                           const float* residual, void* ws, fqStream_t stream);
/* The recompute pair: the two storing twins back to back (the tensor between the layers exists on the host). */
int fq_pwconv_i8_stat_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                           int64_t n, int64_t cin, int64_t cin_pad, int64_t cout_pad, int64_t cout, int64_t hw,
                           const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                           float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                           fqStream_t stream);
int fq_pwdw_fused_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* pw_bias,
                       int64_t n, int64_t cin, int64_t cin_pad, int64_t cout_pad, int64_t cout, int64_t h, int64_t w,
                       const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, const float* pw_bn_scale,
                       const float* pw_bn_shift, int pw_act, const float* mid_stat, const float* mid_thr, int mid_width,
                       unsigned mid_flags, float* mid_current_max, const float* dw_w, const float* dw_bias, int dw_stride,
                       const float* dw_bn_scale, const float* dw_bn_shift, int dw_act, float* y, float* stat_out,
                       fqStream_t stream);
/* fq_pwconv_i8_host on planes of one pixel, then fq_eval_counters_host on the logits it wrote (eval_ws, ws: unused). */
int fq_dense_i8_eval_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                          const float* bias, float* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout,
                          const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                          float* out_current_max, const int64_t* labels, float* counters, void* eval_ws, void* ws,
                          fqStream_t stream);
/* wcodes: row-major [rows_pad][9 * cin] codes of the weights permuted to (cout, 3, 3, cin) (fq_weight_codes_host). */
int fq_conv3x3_i8_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                       const float* bias, float* y, int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w,
                       const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                       float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                       fqStream_t stream);
int fq_pwconv_i8_c16_host(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                          const float* bias, void* y, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t h,
                          int64_t w, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                          float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                          const float* residual, const float* out_thr, int out_width, unsigned out_flags, void* ws,
                          fqStream_t stream);
int fq_pwconv_i8_c16_dual_host(const void* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                               float* y, void* y16, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout, int64_t h, int64_t w,
                               const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                               float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                               const float* residual, const float* out_thr, int out_width, unsigned out_flags, void* ws,
                               fqStream_t stream);
int fq_pwconv_i8_c16_dual_sub2_host(const void* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                                    const float* bias, float* y, void* y16, int64_t n, int64_t cin, int64_t cin_pad, int64_t cout,
                                    int64_t h, int64_t w, const float* in_stat, const float* in_thr, int in_width,
                                    unsigned in_flags, float* out_current_max, const float* bn_scale, const float* bn_shift,
                                    int act, float* stat_out, const float* residual, const float* out_thr, int out_width,
                                    unsigned out_flags, void* ws, fqStream_t stream);
int fq_conv3x3_i8_c16_host(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                           const float* bias, void* y, int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w,
                           const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                           float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                           const float* out_thr, int out_width, unsigned out_flags, fqStream_t stream);
int fq_dwconv3x3_c16_host(const void* x, const float* w, const float* bias, void* y, int64_t n, int64_t c, int64_t h,
                          int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                          float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                          const float* out_thr, int out_width, unsigned out_flags, fqStream_t stream);
int fq_weight_slices_host(const float* w, int64_t rows, int64_t row_len, int64_t row_pad, int64_t rows_pad, int8_t* codes,
                          float* pscale, int32_t* rowsum, void* ws, fqStream_t stream);
int fq_conv3x3_i8_sliced_host(const float* x, const int8_t* wslices, const float* pscale, const int32_t* wsum,
                              const float* bias, float* y, int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w,
                              const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                              float* out_current_max, const float* bn_scale, const float* bn_shift, int act,
                              float* stat_out, fqStream_t stream);
int fq_ste_forward_host(const float* x, float* y, int64_t rows, int64_t row_len, const float* scales, int has_clip,
                        float clip_lo, float clip_hi, float eps, fqStream_t stream);
int fq_weight_fake_quant_host(const float* w, float* w_q, int64_t rows, int64_t row_len, int width,
                              float* scales_out, void* ws, fqStream_t stream);
int fq_wino_weight_fake_quant_host(const float* w, float* w_q, int64_t cout, int64_t cin_g, int t, const float* G,
                                   const float* GI, const float* GTI, int width, float* scales_out, void* ws,
                                   fqStream_t stream);
int fq_ema_update_host(float* state, const float* current, int64_t count, double momentum, fqStream_t stream);
int fq_global_max_host(const float* x, int64_t numel, float* out, fqStream_t stream);
int fq_histogram_accumulate_host(const float* x, int64_t numel, const float* max_dev, int bins, uint64_t* hist,
                                 uint32_t* neg_count, fqStream_t stream);
int fq_hist_to_float_host(const uint64_t* hist, float* out, int64_t count, fqStream_t stream);
int fq_kl_search_host(const float* hist, int64_t L, int bins, int levels, int min_bins, int32_t* out_best, void* ws,
                      fqStream_t stream);
int fq_quantize_codes_host(const float* x, int32_t* codes, int64_t numel, int mode, float* range_dev, void* ws,
                           fqStream_t stream);
int fq_dequantize_host(const int32_t* codes, float* y, int64_t numel, const float* scale_dev, fqStream_t stream);

int fq_qconv_weights_prepare_host(const float* w, int64_t cin, int64_t cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                  int groups, int weight_mode, float w_min, float w_max, void* wbuf, void* ws,
                                  fqStream_t stream);
int fq_qconv2d_forward_host(const float* x, const float* w, const void* wbuf, const float* bias, float* y, int64_t n,
                            int64_t cin, int64_t h, int64_t wdt, int64_t cout, int kh, int kw, int sh, int sw, int ph, int pw,
                            int groups, int input_mode, float in_min, float in_max, const float* in_stat, int act,
                            const float* bn_scale, const float* bn_shift, float* stat_out, void* ws, int force_direct,
                            fqStream_t stream);

/* The reference's UNFUSED op chain for one activation tensor, pass by pass, as MXNet's CPU NDArray ops would run it
 * (convert_conv2d.py:56-66, ste_func.py:41): abs (temp) -> per-sample max -> mean -> clip (temp) -> divide (temp) ->
 * round (temp) -> multiply; each pass an OpenMP loop over the whole tensor.  Same results as
 * fq_fake_quant_online_host; 44 B/elem of memory traffic instead of 12.  tmp: 2 * n * inner floats (or NULL).      */
int fq_unfused_chain_host(const float* x, float* y, int64_t n, int64_t inner, int width, unsigned flags,
                          float* out_current_max, float* tmp, fqStream_t stream);

/* The storing 1x1 with a front layer (fq_pwconv_i8_front): on the host the tensor between the layers exists, so the twin IS the
 * two storing twins back to back - fq_dwconv3x3_host (stride 1) on front_x, the depthwise layer's fp32 INPUT (the host keeps no
 * codes), into z (n * cin * h * w floats of the caller's), then fq_pwconv_i8_host on z with front_stat_out[n] = max|z[n]| as its
 * online statistic when in_stat is NULL.  That composition is the whole contract of the device entry point, which is why the two
 * are DEFINED here (plain, not inline: the one unit that includes this header, oracle/fq_host.cpp, exports them).              */
int fq_pwconv_i8_front_supported_host(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w) {
  return n > 0 && h >= 1 && w >= 4 && w % 4 == 0 && w / 4 <= 64 && cin == 256 && cout == 256 ? 1 : 0;
}
int fq_pwconv_i8_front_host(const float* front_x, float* z, float* front_stat_out, const int8_t* wcodes, const float* wscale,
                            const int32_t* wsum, const float* bias, float* y, int64_t n, int64_t cin, int64_t cin_pad,
                            int64_t cout, int64_t h, int64_t w, const float* in_stat, const float* in_thr, int in_width,
                            unsigned in_flags, float* out_current_max, const float* bn_scale, const float* bn_shift, int act,
                            float* stat_out, const float* front_w, const float* front_bias, const float* front_bn_scale,
                            const float* front_bn_shift, int front_act, const float* front_in_stat, const float* front_in_thr,
                            int front_width, unsigned front_flags, float* front_current_max, fqStream_t stream) {
  int rc = fq_dwconv3x3_host(front_x, front_w, front_bias, z, n, cin, h, w, 1, front_in_stat, front_in_thr, front_width,
                             front_flags, front_current_max, front_bn_scale, front_bn_shift, front_act, front_stat_out, stream);
  if (rc != 0) return rc;
  return fq_pwconv_i8_host(z, wcodes, wscale, wsum, bias, y, n, cin, cin_pad, cout, h * w,
                           in_stat != 0 || in_thr != 0 ? in_stat : front_stat_out, in_thr, in_width, in_flags, out_current_max,
                           bn_scale, bn_shift, act, stat_out, 0, stream);
}

/* The grouped 3x3 convolution on the codes (fq_gconv3x3_i8), restated plainly: codes of x by clip -> IEEE divide -> roundf, the
 * int32 sum of every output channel over its own group's taps read from the EXPANDED code rows (wcodes: rows of 320 bytes, tap
 * t's 32 slab positions at [32 t, 32 t + 32)), one fp32 multiply by sx * wscale[co], bias, BatchNorm, activation, statistic.
 * DEFINED here like the pair above (the one unit that includes this header exports them).                                     */
int fq_gconv3x3_i8_supported_host(int64_t cin, int64_t cout, int64_t groups) {
  if (cin != cout || cin <= 0 || cin % 32 != 0 || groups <= 1 || cin % groups != 0) return 0;
  return cin / groups == 4 || cin / groups == 8 || cin / groups == 16 || cin / groups == 32 ? 1 : 0;
}
int fq_gconv3x3_i8_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                        float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                        const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                        const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  (void)wsum;
  if (!x || !wcodes || !wscale || !y || !fq_gconv3x3_i8_supported_host(c, c, groups) || (!in_stat && !in_thr)) return 1;
  float mean = 0.0f;
  if (in_stat != 0) {
    int rc = fq_batch_mean_host(in_stat, n, &mean, stream);
    if (rc != 0) return rc;
    if (out_current_max != 0) out_current_max[0] = mean;
  }
  const float max_ = in_thr != 0 ? in_thr[0] : mean;
  const int sgn = (in_flags & FQ_ACT_SIGNED) != 0;
  const float levels = sgn ? (float)((1 << (in_width - 1)) - 1) : (float)((1 << in_width) - 1);
  const float lo = (in_flags & FQ_ACT_LO_NEG_MAX) ? -max_ : 0.0f, sx = max_ / levels, den = sx + 1e-10f;
  const int64_t cg = c / groups;
  act &= ~FQ_STAT_PREZEROED;
  for (int64_t s = 0; s < n; ++s) {
    float m = 0.0f;
    for (int64_t co = 0; co < c; ++co) {
      const int64_t ci0 = co / cg * cg, p0 = ci0 % 32;                    /* the group's first channel, its slab position */
      for (int64_t oh = 0; oh < h; ++oh)
        for (int64_t ow = 0; ow < w; ++ow) {
          int32_t acc = 0;
          for (int t = 0; t < 9; ++t) {
            const int64_t ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
            if (ih < 0 || ih >= h || iw < 0 || iw >= w) continue;
            for (int64_t j = 0; j < cg; ++j) {
              float v = x[((s * c + ci0 + j) * h + ih) * w + iw];
              v = v < lo ? lo : (v > max_ ? max_ : v);
              if (v != v) v = lo;
              const float q = v / den, r = (float)(int32_t)(q + (q < 0.0f ? -0.49999997f : 0.49999997f));
              acc += (int32_t)r * (int32_t)wcodes[co * 320 + 32 * t + p0 + j];
            }
          }
          float v = (float)acc * (sx * wscale[co]);
          if (bias != 0) v = v + bias[co];
          if (bn_scale != 0) {
            v = v * bn_scale[co];
            v = v + bn_shift[co];
          }
          if (act == FQ_ACT_RELU || act == FQ_ACT_RELU6) v = v > 0.0f ? v : 0.0f;
          if (act == FQ_ACT_RELU6) v = v < 6.0f ? v : 6.0f;
          y[((s * c + co) * h + oh) * w + ow] = v;
          const float a = v < 0.0f ? -v : v;
          m = a > m ? a : m;
        }
    }
    if (stat_out != 0) stat_out[s] = m;
  }
  return 0;
}

/* ... with stride 2 (fq_gconv3x3_s2_i8), as plainly: output (oh, ow) sums the taps at input (2 oh + dy, 2 ow + dx) that exist;
 * y: (n, c, (h - 1) / 2 + 1, (w - 1) / 2 + 1); the statistic covers these outputs only.  DEFINED here like the pair above.      */
int fq_gconv3x3_s2_i8_supported_host(int64_t cin, int64_t cout, int64_t groups) {
  return fq_gconv3x3_i8_supported_host(cin, cout, groups);
}
int fq_gconv3x3_s2_i8_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                           float* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w, const float* in_stat,
                           const float* in_thr, int in_width, unsigned in_flags, float* out_current_max, const float* bn_scale,
                           const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  (void)wsum;
  if (!x || !wcodes || !wscale || !y || !fq_gconv3x3_s2_i8_supported_host(c, c, groups) || (!in_stat && !in_thr)) return 1;
  float mean = 0.0f;
  if (in_stat != 0) {
    int rc = fq_batch_mean_host(in_stat, n, &mean, stream);
    if (rc != 0) return rc;
    if (out_current_max != 0) out_current_max[0] = mean;
  }
  const float max_ = in_thr != 0 ? in_thr[0] : mean;
  const int sgn = (in_flags & FQ_ACT_SIGNED) != 0;
  const float levels = sgn ? (float)((1 << (in_width - 1)) - 1) : (float)((1 << in_width) - 1);
  const float lo = (in_flags & FQ_ACT_LO_NEG_MAX) ? -max_ : 0.0f, sx = max_ / levels, den = sx + 1e-10f;
  const int64_t cg = c / groups, ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  act &= ~FQ_STAT_PREZEROED;
  for (int64_t s = 0; s < n; ++s) {
    float m = 0.0f;
    for (int64_t co = 0; co < c; ++co) {
      const int64_t ci0 = co / cg * cg, p0 = ci0 % 32;                    /* the group's first channel, its slab position */
      for (int64_t oh = 0; oh < ho; ++oh)
        for (int64_t ow = 0; ow < wo; ++ow) {
          int32_t acc = 0;
          for (int t = 0; t < 9; ++t) {
            const int64_t ih = 2 * oh + t / 3 - 1, iw = 2 * ow + t % 3 - 1;
            if (ih < 0 || ih >= h || iw < 0 || iw >= w) continue;
            for (int64_t j = 0; j < cg; ++j) {
              float v = x[((s * c + ci0 + j) * h + ih) * w + iw];
              v = v < lo ? lo : (v > max_ ? max_ : v);
              if (v != v) v = lo;
              const float q = v / den, r = (float)(int32_t)(q + (q < 0.0f ? -0.49999997f : 0.49999997f));
              acc += (int32_t)r * (int32_t)wcodes[co * 320 + 32 * t + p0 + j];
            }
          }
          float v = (float)acc * (sx * wscale[co]);
          if (bias != 0) v = v + bias[co];
          if (bn_scale != 0) {
            v = v * bn_scale[co];
            v = v + bn_shift[co];
          }
          if (act == FQ_ACT_RELU || act == FQ_ACT_RELU6) v = v > 0.0f ? v : 0.0f;
          if (act == FQ_ACT_RELU6) v = v < 6.0f ? v : 6.0f;
          y[((s * c + co) * ho + oh) * wo + ow] = v;
          const float a = v < 0.0f ? -v : v;
          m = a > m ? a : m;
        }
    }
    if (stat_out != 0) stat_out[s] = m;
  }
  return 0;
}

/* The two ends of a composed C16 twin.  A C16 tensor ([n][C/16][plane][16], fakequant.h) read back as the fp32 values its codes stand
 * for (code * sx, which quantise to the same codes), and an fp32 tensor quantised with a consumer's stored threshold into that layout. */
static void fqh_from_c16(const void* x, float* xf, int64_t n, int64_t c, int64_t hw, const float* thr, int width, unsigned flags) {
  const int sgn = (flags & FQ_ACT_SIGNED) != 0;
  const float sx = thr[0] / (sgn ? (float)((1 << (width - 1)) - 1) : (float)((1 << width) - 1));
  const unsigned char* xb = (const unsigned char*)x;
  for (int64_t s = 0; s < n; ++s)
    for (int64_t ch = 0; ch < c; ++ch)
      for (int64_t p = 0; p < hw; ++p) {
        const int b = xb[((s * (c / 16) + ch / 16) * hw + p) * 16 + ch % 16] ^ 0x80;      /* (code + 128 - zoff) mod 256 */
        xf[(s * c + ch) * hw + p] = (float)(sgn ? (int)(signed char)(unsigned char)(b - 128) : b) * sx;
      }
}
static void fqh_to_c16(const float* yf, void* y, int64_t n, int64_t c, int64_t hw, const float* thr, int width, unsigned flags) {
  const int sgn = (flags & FQ_ACT_SIGNED) != 0;
  const float max_ = thr[0], levels = sgn ? (float)((1 << (width - 1)) - 1) : (float)((1 << width) - 1);
  const float lo = (flags & FQ_ACT_LO_NEG_MAX) ? -max_ : 0.0f, den = max_ / levels + 1e-10f;
  unsigned char* yb = (unsigned char*)y;
  for (int64_t s = 0; s < n; ++s)
    for (int64_t ch = 0; ch < c; ++ch)
      for (int64_t p = 0; p < hw; ++p) {
        float v = yf[(s * c + ch) * hw + p];
        v = v < lo ? lo : (v > max_ ? max_ : v);
        if (v != v) v = lo;
        const float q = v / den;
        const int code = (int32_t)(q + (q < 0.0f ? -0.49999997f : 0.49999997f));
        yb[((s * (c / 16) + ch / 16) * hw + p) * 16 + ch % 16] = (unsigned char)(((code + (sgn ? 128 : 0)) & 255) ^ 0x80);
      }
}

/* ... between C16 code tensors (fq_gconv3x3_i8_c16, fq_gconv3x3_s2_i8_c16), composed of the two twins above and the two ends.
 * DEFINED here like the pair above (C++ only: the one unit that includes this header is).                                      */
int fq_gconv3x3_i8_c16_host(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                            const float* bias, void* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w,
                            const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                            const float* bn_scale, const float* bn_shift, int act, float* stat_out, const float* out_thr,
                            int out_width, unsigned out_flags, fqStream_t stream) {
  if (!x || !y || (!x_is_c16 && !out_thr) || (x_is_c16 && !in_thr) || c % 16 != 0) return 1;
  const int64_t hw = h * w, numel = n * c * hw;
  float* xf = x_is_c16 ? new float[numel] : 0;
  float* yf = out_thr ? new float[numel] : 0;
  if (x_is_c16) fqh_from_c16(x, xf, n, c, hw, in_thr, in_width, in_flags);
  int rc = fq_gconv3x3_i8_host(x_is_c16 ? xf : (const float*)x, wcodes, wscale, wsum, bias, out_thr ? yf : (float*)y, n, c, groups,
                               h, w, in_stat, in_thr, in_width, in_flags, out_current_max, bn_scale, bn_shift, act, stat_out, stream);
  if (rc == 0 && out_thr) fqh_to_c16(yf, y, n, c, hw, out_thr, out_width, out_flags);
  delete[] xf;
  delete[] yf;
  return rc;
}

int fq_gconv3x3_s2_i8_c16_host(const void* x, int x_is_c16, const int8_t* wcodes, const float* wscale, const int32_t* wsum,
                               const float* bias, void* y, int64_t n, int64_t c, int64_t groups, int64_t h, int64_t w,
                               const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                               const float* bn_scale, const float* bn_shift, int act, float* stat_out, const float* out_thr,
                               int out_width, unsigned out_flags, fqStream_t stream) {
  if (!x || !y || (!x_is_c16 && !out_thr) || (x_is_c16 && !in_thr) || c % 16 != 0) return 1;
  const int64_t hwi = h * w, hwo = ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
  float* xf = x_is_c16 ? new float[n * c * hwi] : 0;
  float* yf = out_thr ? new float[n * c * hwo] : 0;
  if (x_is_c16) fqh_from_c16(x, xf, n, c, hwi, in_thr, in_width, in_flags);
  int rc = fq_gconv3x3_s2_i8_host(x_is_c16 ? xf : (const float*)x, wcodes, wscale, wsum, bias, out_thr ? yf : (float*)y, n, c,
                                  groups, h, w, in_stat, in_thr, in_width, in_flags, out_current_max, bn_scale, bn_shift, act,
                                  stat_out, stream);
  if (rc == 0 && out_thr) fqh_to_c16(yf, y, n, c, hwo, out_thr, out_width, out_flags);
  delete[] xf;
  delete[] yf;
  return rc;
}

/* The dense 3x3 convolution on the codes for 16 and 32 input channels (fq_conv3x3_i8_narrow), restated plainly on the DEVICE's
 * weight buffer: rows of row_pad = 192 / 320 bytes, tap t's cin codes at [cin t, cin t + cin).  A tap outside the image
 * contributes x = 0, whose code is 0 in either signedness.  DEFINED here like the grouped twins above.                        */
int fq_conv3x3_i8_narrow_host(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* bias,
                              float* y, int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, const float* in_stat,
                              const float* in_thr, int in_width, unsigned in_flags, float* out_current_max,
                              const float* bn_scale, const float* bn_shift, int act, float* stat_out, fqStream_t stream) {
  (void)wsum;
  if (!x || !wcodes || !wscale || !y || (cin != 16 && cin != 32) || cout < 1 || (!in_stat && !in_thr)) return 1;
  float mean = 0.0f;
  if (in_stat != 0) {
    int rc = fq_batch_mean_host(in_stat, n, &mean, stream);
    if (rc != 0) return rc;
    if (out_current_max != 0) out_current_max[0] = mean;
  }
  const float max_ = in_thr != 0 ? in_thr[0] : mean;
  const int sgn = (in_flags & FQ_ACT_SIGNED) != 0;
  const float levels = sgn ? (float)((1 << (in_width - 1)) - 1) : (float)((1 << in_width) - 1);
  const float lo = (in_flags & FQ_ACT_LO_NEG_MAX) ? -max_ : 0.0f, sx = max_ / levels, den = sx + 1e-10f;
  const int64_t row_pad = (9 * cin + 63) / 64 * 64;
  act &= ~FQ_STAT_PREZEROED;
  for (int64_t s = 0; s < n; ++s) {
    float m = 0.0f;
    for (int64_t co = 0; co < cout; ++co)
      for (int64_t oh = 0; oh < h; ++oh)
        for (int64_t ow = 0; ow < w; ++ow) {
          int32_t acc = 0;
          for (int t = 0; t < 9; ++t) {
            const int64_t ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
            if (ih < 0 || ih >= h || iw < 0 || iw >= w) continue;
            for (int64_t ci = 0; ci < cin; ++ci) {
              float v = x[((s * cin + ci) * h + ih) * w + iw];
              v = v < lo ? lo : (v > max_ ? max_ : v);
              if (v != v) v = lo;
              const float q = v / den, r = (float)(int32_t)(q + (q < 0.0f ? -0.49999997f : 0.49999997f));
              acc += (int32_t)r * (int32_t)wcodes[co * row_pad + cin * t + ci];
            }
          }
          float v = (float)acc * (sx * wscale[co]);
          if (bias != 0) v = v + bias[co];
          if (bn_scale != 0) {
            v = v * bn_scale[co];
            v = v + bn_shift[co];
          }
          if (act == FQ_ACT_RELU || act == FQ_ACT_RELU6) v = v > 0.0f ? v : 0.0f;
          if (act == FQ_ACT_RELU6) v = v < 6.0f ? v : 6.0f;
          y[((s * cout + co) * h + oh) * w + ow] = v;
          const float a = v < 0.0f ? -v : v;
          m = a > m ? a : m;
        }
    if (stat_out != 0) stat_out[s] = m;
  }
  return 0;
}

#ifdef __cplusplus
}
#endif
#endif /* FAKEQUANT_HOST_H_ */
