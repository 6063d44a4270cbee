// libfakequant — fq_dwconv3x3, the depthwise 3x3 with quantise-on-load: argument checks, the call description and the choice
// between the five kernel forms (fq_dw.h; one translation unit each: fq_dw_flat, fq_dw_planes, fq_dw_cols, fq_dw_tiles)
// (see fq_common.h for the list of translation units and the design rules)
#include "fq_dw.h"

static int dwconv3x3_impl(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                          int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                          float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                          fqStream_t stream, void* x_codes_out = nullptr) {
  FQ_REQUIRE(x && w && (y || stat_out), "fq_dwconv3x3: null pointer");
  FQ_REQUIRE(y || !x_codes_out || (in_width <= 8 && !(in_flags & kFlagRangeRecord) &&
                                   ((in_flags & FQ_ACT_SIGNED) || !(in_flags & FQ_ACT_LO_NEG_MAX))),
             "fq_dwconv3x3: x_codes_out keeps codes that fit a byte (at most 8 bits; unsigned levels with a clip range from 0)");
  FQ_REQUIRE(!(y && x_codes_out), "fq_dwconv3x3: x_codes_out belongs to the statistic pass (y == NULL)");
  FQ_REQUIRE(n > 0 && c > 0 && h > 0 && wdt > 0 && n * c < (1ll << 31) && h * wdt < (1ll << 28),
             "fq_dwconv3x3: bad shape (n=%lld c=%lld h=%lld w=%lld)", (long long)n, (long long)c, (long long)h,
             (long long)wdt);
  FQ_REQUIRE(stride == 1 || stride == 2, "fq_dwconv3x3: stride must be 1 or 2, got %d", stride);
  // in_stat alone: online; in_thr alone: offline; both: offline, the statistic only feeds out_current_max
  FQ_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "fq_dwconv3x3: bn_scale and bn_shift go together");
  const bool prezeroed = (act & FQ_STAT_PREZEROED) != 0;
  act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(act >= FQ_ACT_NONE && act <= FQ_ACT_RELU6, "fq_dwconv3x3: unknown activation %d", act);
  const bool quant = in_stat != nullptr || in_thr != nullptr;
  if (quant) FQ_REQUIRE(in_width >= 2 && in_width <= 16, "fq_dwconv3x3: width %d out of range", in_width);
  if (in_flags & kFlagBiasMultiplies) act |= kActBiasMul;   // (after the range check; bias != NULL: run-time epilogue)
  static const int epi_on = env_int("FQ_DW_EPI", 1);    // 0: always the run-time epilogue (A/B)

  DwCall d = {};
  d.x = x; d.w = w; d.bias = bias; d.y = y; d.x_codes_out = x_codes_out;
  d.n = n, d.c = c, d.h = h, d.wdt = wdt, d.stride = stride;
  d.in_stat = in_stat, d.in_thr = in_thr, d.out_current_max = out_current_max;
  d.bn_scale = bn_scale, d.bn_shift = bn_shift, d.act = act, d.stat_out = stat_out;
  d.st = (hipStream_t)stream;
  d.quant = quant, d.online = quant && in_thr == nullptr, d.prezeroed = prezeroed;
  d.epi = (epi_on && bn_scale != nullptr && bias == nullptr)
              ? (act == FQ_ACT_RELU ? kEpiBnRelu : act == FQ_ACT_RELU6 ? kEpiBnRelu6 : kEpiRuntime)
              : kEpiRuntime;
  d.levels = act_levels(in_width, in_flags);
  d.lo_neg = (in_flags & kFlagRangeRecord) ? kRangeMode : ((in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0);
  d.eps = (in_flags & FQ_ACT_NO_EPS) ? 0.0f : kEps;
  d.ho = (h - 1) / stride + 1, d.wo = (wdt - 1) / stride + 1;

  // 0 auto, 1 LDS tiles, 2 one column per lane, 3 four columns per lane, 4 whole planes, 5 flat.  A forced form that does
  // not take the shape falls through to the next one that does.
  static const int form = env_int("FQ_DW_FORM", 0);
  if (y == nullptr) {         // the statistic pass: the flat form on 28 x 28 planes, else the four-columns form
    if (stride == 1 && dw_flat_stat_applies(d)) return dw_run_flat(d);
    FQ_REQUIRE(quant && stride == 1 && dw_cols4_applies(d, 3),
               "fq_dwconv3x3: without y (statistic pass) only stride 1, a quantised input and rows of a multiple of 4 floats, "
               "16-byte aligned, are taken (n=%lld c=%lld h=%lld w=%lld stride %d)", (long long)n, (long long)c, (long long)h,
               (long long)wdt, stride);
    return dw_run_cols4(d);
  }
  if (dw_flat_applies(d, form)) return dw_run_flat(d);
  if (dw_planes_applies(d, form)) return dw_run_planes(d);
  if (dw_cols4_applies(d, form)) return dw_run_cols4(d);
  if (dw_cols_applies(d, form)) return dw_run_cols(d);
  return dw_run_tiles(d);
}

namespace fqi {
// depthwise 3x3 of nn.Conv2D(quantized=True): x quantised on load with the range record `rec` (codes, not values, enter the
// sums), wcodes_f32 = the int8 weight codes as fp32, y = act(sum * svec[c]) with svec = in_scale * w_scale, or - a BatchNorm
// folded behind the block - y = act((sum * svec[c]) * bn_scale[c] + bn_shift[c]), every step separately rounded
int dw_range_call(const float* x, const float* wcodes_f32, float* y, int64_t n, int64_t c, int64_t h, int64_t wdt, int stride,
                  const float* rec, const float* svec, const float* bn_scale, const float* bn_shift, int act,
                  float* stat_out, hipStream_t st) {
  return dwconv3x3_impl(x, wcodes_f32, svec, y, n, c, h, wdt, stride, nullptr, rec, 8, kFlagRangeRecord | kFlagBiasMultiplies,
                        nullptr, bn_scale, bn_shift, act, stat_out, (fqStream_t)st);
}
}  // namespace fqi

extern "C" {

int fq_dwconv3x3(const float* x, const float* w, const float* bias, float* y, int64_t n, int64_t c, int64_t h,
                 int64_t wdt, int stride, const float* in_stat, const float* in_thr, int in_width, unsigned in_flags,
                 float* out_current_max, const float* bn_scale, const float* bn_shift, int act, float* stat_out,
                 fqStream_t stream, void* x_codes_out) {
  FQ_REQUIRE(!(in_flags & ~(FQ_ACT_SIGNED | FQ_ACT_LO_NEG_MAX | FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_dwconv3x3: unknown flags");
  return dwconv3x3_impl(x, w, bias, y, n, c, h, wdt, stride, in_stat, in_thr, in_width, in_flags, out_current_max, bn_scale,
                        bn_shift, act, stat_out, stream, x_codes_out);
}

}  // extern "C"
