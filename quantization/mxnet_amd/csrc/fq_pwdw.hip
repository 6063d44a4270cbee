// libfakequant — K2y: a pointwise (1x1) convolution on int8 codes AND the depthwise 3x3 behind it in one launch
// (see fq_common.h for the list of translation units and the design rules; what it shares with fq_pw_stat.hip: fq_pair.h)
//
// Why (round 6): under ONLINE thresholds every fused producer writes its output in fp32 only for the next launch to read it
// back - the batch statistic that scales the consumer's quantiser (convert_conv2d.py:56-58: mean over the batch of the
// per-sample maxima of the WHOLE tensor) is not known before the producer's last workgroup has finished, so codes cannot be
// handed over.  But nothing forbids computing the producer twice: a statistic-only pass (fq_pwconv_i8_stat: the pointwise
// kernel without its stores) leaves the per-sample maxima, and this kernel then recomputes the pointwise outputs from the
// SAME input - bit for bit the same fp32 values: exact int32 sums, the same epilogue - quantises them with the now known
// threshold and feeds the depthwise stencil without the tensor ever reaching HBM.  A MobileNet pair (x -> 1x1 -> y -> 3x3 -> z,
// y twice as many channels as x) moves 4x + 4x + 4z bytes instead of 4x + 4y + 4y + 4z: 0.31 instead of 1.13 GB on the first
// pair of MobileNet1.0 at batch 128.  (The other direction - depthwise into pointwise - saves one tensor of x's size per pair;
// this one saves the EXPANDED tensor twice.)
//
// Form.  v_mfma_i32_32x32x32_i8 with the ACTIVATIONS as the A operand and the weight fragment as B, i.e. D = pixels x
// channels: lane l owns output channel (l & 31) and its 16 registers are 16 PIXELS.  The 32 MFMA rows are given to the
// pixels of a 32-column strip of one image row in an order that makes those 16 pixels consecutive columns (row i = 8g + 4h +
// i' holds pixel 16h + 4g + i'; the loads of a channel still cover one 128-byte line), so a lane holds columns 16h .. 16h+15 of
// ITS channel: the depthwise stencil's horizontal neighbours are neighbouring registers (one v_permlane32_swap per row hands
// column 15 / 16 across the two lane halves), its weights and both BatchNorms are 15 per-lane registers instead of LDS reads,
// and the vertical neighbours are the same registers one input row later: a wavefront walks its strip down a band of rows and
// keeps, per pixel, the partial sums of the output rows still open (stride 1: two, stride 2: one), adding each input row's
// three products in the order of the row-major 3x3 chain (fq_dwconv3x3's arithmetic: fmaf by fmaf from +0).
// A workgroup = all strips of a band x the channel groups; finished output rows go through an LDS row buffer (two rows) and
// leave as whole rows, 16 bytes per lane.
#include "fq_dw.h"
#include "fq_pair.h"

namespace {

struct PwDwGeom {
  int Cin, KTS, Cout, H, W, Ho, Wo;   // KTS: 32-channel slabs per row of the fragment-major weight copy (cin_pad / 32)
  int strips, ctg, bands, RB;         // column strips per row, channel groups (Cout / 32 / CW), row bands, output rows per band
  int zoff, pitch;                    // pitch: floats per channel in the LDS row buffer (odd: conflict-free lane = channel writes)
  int vw;                             // floats per lane of the row store: 4, 2 or 1 (Wo % vw == 0)
  FastDiv qv;                         // Wo / vw
};

constexpr int kRowSlack = 8;          // floats in front of each row buffer (a strip's invalid first column lands there)

// The launch's dynamic LDS in bytes: [ct][kt][64] weight fragments; two row buffers of slack + cout * pitch floats with one more
// slack in front (none of it in the statistic mode, which stores no rows); at stride 1 the depthwise layer's constants, 13
// floats per channel.  The plan and the launcher size the launch with it; the kernel's pointers (ldsW, rowbuf, ldsK at its
// top) are this order written out - taking the offsets from here keeps every count but changes 64 instruction sequences
// (profiles/pair_units_one_of_each.txt).
inline size_t pwdw_lds(int ct, int kt, int cout, int pitch, int stride, bool stat_mode) {
  const size_t rows = stat_mode ? 0 : (size_t)(kRowSlack + 2 * (cout * pitch + kRowSlack)) * 4;
  return (size_t)ct * kt * 1024 + rows + (stride == 1 ? (size_t)cout * 13 * 4 : 0);
}

// slabs in flight per lane: a ring of NB buffers of 16 values, the loads of slab q + NB - 1 issued before slab q is quantised
// (stride 1 keeps 32 more partial sums per channel tile: two buffers there)
template <int KT, int S> struct PwDwRing {
  static constexpr int NB = S == 1 ? 2 : (KT <= 2 ? 3 : 4);
  // code input (CODES below): a slab is ONE 16-byte load per lane, so the ring holds whole rows - KT fragments each, 4 KT
  // registers - and the loads of row t + NR - 1 leave before row t is multiplied: a row's arithmetic covers their latency
  static constexpr int NR = 2;
};

// FAST 0: every epilogue decided at run time, general quantisers; 1: the fused-inference case - no bias, BatchNorm and ReLU
// (ReLU6 when `relu6`) behind both convolutions, unsigned activations (both clip ranges start at 0)
// CODES 1: the input arrives as the codes the statistic pass left behind (`xc`: [n][2 KT][H * W][16] bytes, a lane's A fragment
// of a pixel and a slab is one 16-byte vector of it) - x is not read, nothing is quantised on the input side
// NS 1 (stride 1, code input): the STATISTIC mode of the launch - the depthwise output is computed, its per-sample maximum is
// taken from the finished sums and nothing of it is stored (no LDS row buffer, no barrier per row); instead the codes of the
// pointwise output, which the launch has just made for the stencil, leave as planar int8 (`y` is that buffer: [n][Cout][H * W]
// bytes, 0 .. 255 or two's complement, what fq_dwconv3x3's statistic pass keeps of ITS input) for the front layer of the next
// pair's statistic pass (pw_stat_kernel of fq_pw_stat.hip), which recomputes the depthwise values from them.
template <int KT, int CW, int S, int LZ, int FAST, int CODES, int NS = 0>
__global__ __launch_bounds__(512) void pwdw_kernel(
    const float* __restrict__ x, const int8_t* __restrict__ xc, const int8_t* __restrict__ wfrag, const float* __restrict__ wscale,
    const int* __restrict__ wsum, const float* __restrict__ bias1, PwDwGeom g, const float* __restrict__ in_stat, int n,
    const float* __restrict__ in_thr, float levels1, int lo_neg1, float eps, const float* __restrict__ bn1_scale,
    const float* __restrict__ bn1_shift, int act1, const float* __restrict__ mid_stat, const float* __restrict__ mid_thr,
    float levels2, int lo_neg2, float* __restrict__ mid_cur_out, const float* __restrict__ dww,
    const float* __restrict__ bias2, const float* __restrict__ bn2_scale, const float* __restrict__ bn2_shift, int act2,
    float* __restrict__ y, float* __restrict__ stat_out) {
  constexpr int NB = CODES ? 1 : PwDwRing<KT, S>::NB, NR = CODES ? PwDwRing<KT, S>::NR : 1;
  static_assert(!NS || (S == 1 && CODES == 1), "the statistic mode is built for stride 1 on code input");
  extern __shared__ __attribute__((aligned(16))) unsigned char pwdw_smem[];
  __shared__ float red[8];
  const int CT = g.ctg * CW;
  v4i* ldsW = reinterpret_cast<v4i*>(pwdw_smem);                                    // [CT][KT][64] fragments
  const int rb_stride = g.Cout * g.pitch + kRowSlack;
  float* rowbuf = reinterpret_cast<float*>(pwdw_smem + (size_t)CT * KT * 1024) + kRowSlack;     // [2][slack + Cout * pitch]
  // stride 1 keeps two open sums per pixel: the depthwise layer's per-channel constants stay in LDS there (13 floats per channel:
  // an odd stride, every lane its own bank) and are read where they are used
  constexpr bool kDwLds = S == 1;
  float* ldsK = NS ? reinterpret_cast<float*>(pwdw_smem + (size_t)CT * KT * 1024) : rowbuf + 2 * rb_stride;   // [Cout][13]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, i32 = lane & 31;
  const int s = wave % g.strips, cgi = wave / g.strips;
  const int band = (int)(blockIdx.x % (unsigned)g.bands);
  const int smp = n - 1 - (int)(blockIdx.x / (unsigned)g.bands);                    // last samples first: what the statistic pass
                                                                                    // read last is what the caches still hold
  const int HW = g.H * g.W;

  // ---- geometry of this wave's strip ----------------------------------------------------------------------------------------
  // local pixel p = 0 .. 31 of the strip is input column c0 + p - 1.  Stride 1: 30 outputs per strip (p = 1 .. 30); the LAST
  // strip is anchored at the right edge (c0 = W - 30: the columns it shares with its neighbour come out the same from both), so
  // the zero column right of the image is always p = 31; a plane narrower than 30 is one strip whose zero column LEFT of the
  // image is p = LZ = 30 - W.  Stride 2 (even W): 15 outputs per strip, centre p = 2 oc + 1; only the left zero column exists.
  int c0;
  if (S == 1) c0 = (s == g.strips - 1) ? g.W - 30 : 30 * s;      // (W < 30: one strip, c0 = -LZ)
  else c0 = 30 * s;
  const int pl = mfma_row_pixel(i32);                             // A-operand pixel of this lane (MFMA row i32)
  int col_ld = c0 + pl - 1;
  col_ld = col_ld < 0 ? 0 : (col_ld >= g.W ? g.W - 1 : col_ld);
  const fq_rsrc rs = CODES ? make_rsrc(xc + (int64_t)smp * 2 * KT * HW * 16, (int64_t)2 * KT * HW * 16)
                           : make_rsrc(x + (int64_t)smp * g.Cin * HW, (int64_t)g.Cin * HW * 4);
  const unsigned voff = CODES ? (unsigned)((h * HW + col_ld) * 16) : (unsigned)((16 * h * HW + col_ld) * 4);
  // LDS float offset of this lane's output 0 inside a channel row: stride 1 - own pixel k is output column c0 + 16 h + k - 1
  // (k = 0 of the lower half and k = 15 of the upper half are no outputs); stride 2 - output oc = 8 h + c is column 15 s + oc
  // (c = 7 of the upper half is no output).  Columns past the plane fall into the row's padding.
  const int obase = S == 1 ? c0 + 16 * h - 1 : 15 * s + 8 * h;

  const int ro0 = band * g.RB;
  const int ro1 = ro0 + g.RB < g.Ho ? ro0 + g.RB : g.Ho;
  const int t_first = S == 1 ? ro0 - 1 : 2 * ro0 - 1;
  const int t_last = S == 1 ? ro1 : 2 * (ro1 - 1) + 1;            // inclusive (may be H: a zero row)
  float* yb = y + (int64_t)smp * g.Cout * g.Ho * g.Wo;
  // NS: where this lane's codes of a row go.  A lane holds the 16 columns c0 + 16 h - 1 .. c0 + 16 h + 14 of its channel, one
  // column off a dword boundary, and permlane32_swap brings the column on either side.  c0 is even, W a multiple of four:
  //   c0 = 0 mod 4:  own pixels 1 .. 12 are three aligned dwords at column c0 + 16 h; pixels 13 .. 15 and the upper half's
  //                  pixel 0 a fourth one for the lower half, pixels 13, 14 an aligned pair for the upper half (column c0 + 30 is
  //                  the next strip's);
  //   c0 = 2 mod 4:  own pixels 3 .. 14 are three aligned dwords at column c0 + 2 + 16 h; the lower half's pixel 15 and pixels
  //                  0 .. 2 a fourth one for the upper half, pixels 1, 2 an aligned pair for the lower half (column c0 - 1 is the
  //                  previous strip's).
  // Strips alternate between the two (c0 = 30 s), the anchored last one (c0 = W - 30) and the narrow plane (c0 = -2) are of the
  // second kind: every column of the plane is written, the ones two strips share by both with the same byte, and the stencil's
  // zero columns left and right of the plane (c0 - 1 < 0, c0 + 30 = W) by none.  Whole dwords / pairs lie inside a row or
  // outside it (masked); the buffer descriptor covers this sample's planes only.
  const bool ns_par2 = (c0 & 2) != 0;
  const int ns_col3 = c0 + 16 * h + (ns_par2 ? 2 : 0);                       // the three dwords
  const int ns_colx = ns_par2 ? (h ? c0 + 14 : c0) : c0 + 16 * h + 12;       // the fourth dword (ns_x4) or the pair
  const bool ns_x4 = ns_par2 ? h == 1 : h == 0;
  const bool ns_ok3 = ns_col3 >= 0 && ns_col3 + 12 <= g.W;
  const bool ns_okx = ns_colx >= 0 && ns_colx + (ns_x4 ? 4 : 2) <= g.W;
  const fq_rsrc rsy = make_rsrc(NS ? reinterpret_cast<int8_t*>(y) + (int64_t)smp * g.Cout * HW : nullptr,
                                NS ? (int64_t)g.Cout * HW : 0);

  // slab q of the band = (row t_first + q / KT, 32-channel slab q % KT); buffer q % NB
  float raw[NB][16];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 16; ++i) raw[b][i] = 0.0f;
  auto issue = [&](int t, int kt, float (&v)[16]) __attribute__((always_inline)) {
    if (t < 0 || t >= g.H || t > t_last) return;
    const unsigned so = (unsigned)((kt * 32 * HW + t * g.W) * 4);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = buf_ld_f32(rs, voff, so + (unsigned)(i * HW * 4));
  };
  // code input: row t's fragments, channel block 2 kt + h of this lane's pixel (rows outside the image or past the band are
  // neither requested nor used, as above)
  v4i crow[NR][KT];
#pragma unroll
  for (int b = 0; b < NR; ++b)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) crow[b][kt] = (v4i){0, 0, 0, 0};
  auto issue_row = [&](int t, v4i (&v)[KT]) __attribute__((always_inline)) {
    if (t < 0 || t >= g.H || t > t_last) return;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) v[kt] = buf_ld_v4i(rs, voff, (unsigned)((2 * kt * HW + t * g.W) * 16));
  };
  if constexpr (CODES) {
#pragma unroll
    for (int r = 0; r < NR - 1; ++r) issue_row(t_first + r, crow[r]);
  } else {
#pragma unroll
    for (int q = 0; q < NB - 1; ++q) issue(t_first + q / KT, q % KT, raw[q]);
  }
  FQ_PIN();

  // ---- thresholds: the pointwise input's (statistic of x) and the depthwise input's (statistic of the pointwise output) ----
  const float max1 = input_threshold(in_stat, n, in_thr, nullptr, false);
  const float max2 = input_threshold(mid_stat, n, mid_thr, mid_cur_out, blockIdx.x == 0);
  const QParams q1 = make_qparams(max1, levels1, lo_neg1 != 0, eps);
  const QParams q2 = make_qparams(max2, levels2, lo_neg2 != 0, eps);
  const int ubias1 = 128 - g.zoff;
  const unsigned nn_xor1 = fq_nonneg_xor(ubias1);
  const bool relu6 = act1 == FQ_ACT_RELU6;                        // (FAST: both activations are the same)
  const float top = relu6 ? 6.0f : INFINITY;

  // ---- weights -> LDS (already in fragment order in HBM) ----------------------------------------------------------------
  for (int idx = threadIdx.x; idx < CT * KT * 64; idx += blockDim.x) {
    const int f = idx >> 6, ct = f / KT, kt = f - ct * KT;
    ldsW[idx] = *reinterpret_cast<const v4i*>(wfrag + (((int64_t)ct * g.KTS + kt) << 10) + ((idx & 63) << 4));
  }

  // ---- per-lane constants: this lane's channel of each of the wave's CW channel tiles -------------------------------------
  float k_sxw[CW], k_b1[CW], k_bsc1[CW], k_bsh1[CW], k_w[CW][9], k_b2[CW], k_bsc2[CW], k_bsh2[CW];
  int k_zs[CW];
  const bool has_b1 = bias1 != nullptr, has_bn1 = bn1_scale != nullptr, has_b2 = bias2 != nullptr, has_bn2 = bn2_scale != nullptr;
#pragma unroll
  for (int j = 0; j < CW; ++j) {
    const int c = (cgi * CW + j) * 32 + i32;
    k_sxw[j] = q1.scale * wscale[c];
    k_zs[j] = g.zoff * wsum[c];
    k_b1[j] = has_b1 ? bias1[c] : 0.0f;
    k_bsc1[j] = has_bn1 ? bn1_scale[c] : 1.0f;
    k_bsh1[j] = has_bn1 ? bn1_shift[c] : 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) k_w[j][t] = kDwLds ? 0.0f : dww[c * 9 + t];
    k_b2[j] = (has_b2 && !kDwLds) ? bias2[c] : 0.0f;
    k_bsc2[j] = (has_bn2 && !kDwLds) ? bn2_scale[c] : 1.0f;
    k_bsh2[j] = (has_bn2 && !kDwLds) ? bn2_shift[c] : 0.0f;
  }
  if (kDwLds)
    for (int c = threadIdx.x; c < g.Cout; c += blockDim.x) {
#pragma unroll
      for (int t = 0; t < 9; ++t) ldsK[c * 13 + t] = dww[c * 9 + t];
      ldsK[c * 13 + 9] = has_b2 ? bias2[c] : 0.0f;
      ldsK[c * 13 + 10] = has_bn2 ? bn2_scale[c] : 1.0f;
      ldsK[c * 13 + 11] = has_bn2 ? bn2_shift[c] : 0.0f;
    }
  const bool zero_left = (S == 1 && LZ != 0) ? (h == (LZ >> 4)) : (s == 0 && h == 0);       // lanes holding the column left of the image
  const bool zero_right = S == 1 && s == g.strips - 1 && h == 1;                             // ... right of it (p = 31)
  __syncthreads();                                                // weights in LDS
  FQ_PIN();

  float m = 0.0f;
  const FastQuot fq1 = make_fast_quot(q1.denom), fq2 = make_fast_quot(q2.denom);
  // NN: both clip ranges start at 0 AND both divisors take the fp32 quotient (fq_common.h: fast_quot); else the general forms
  auto body = [&](auto nn_c) __attribute__((always_inline)) {
    constexpr bool NN = decltype(nn_c)::value;
    // open partial sums: stride 1 - A (output row t-1: has its first two tap rows) and B (output row t: its first);
    // stride 2 - A only (8 outputs per lane)
    constexpr int NO = S == 1 ? 16 : 8;
    float sumA[CW][NO], sumB[S == 1 ? CW : 1][NO];
#pragma unroll
    for (int j = 0; j < CW; ++j)
#pragma unroll
      for (int k = 0; k < NO; ++k) {
        sumA[j][k] = 0.0f;
        if (S == 1) sumB[j][k] = 0.0f;
      }
    QParams qc = q2;                               // FAST: ReLU / ReLU6 and the clip as one median (clip range starts at 0)
    if (FAST) qc.hi = fminf(q2.hi, top);

    // one input row; PH: its first slab is slab (PH * KT) mod NB of the ring (code input: the row is row PH mod NR of its ring)
    auto row = [&](int t, auto ph_c) __attribute__((always_inline)) {
      constexpr int PH = decltype(ph_c)::value;
      const bool row_ok = t >= 0 && t < g.H;
      v4i afrag[KT];
      if constexpr (CODES) {
        issue_row(t + NR - 1, crow[(PH + NR - 1) % NR]);             // into the row freed last
        FQ_PIN();
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) afrag[kt] = crow[PH % NR][kt];
      } else {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          const int qn = kt + NB - 1;                                  // the slab NB - 1 ahead goes into the buffer freed last
          issue(t + qn / KT, qn % KT, raw[(PH * KT + kt + NB - 1) % NB]);
          FQ_PIN();
          afrag[kt] = pair_frag16<NN>(raw[(PH * KT + kt) % NB], q1, fq1, ubias1, nn_xor1);
          FQ_PIN();
        }
      }
      const int r_emit = S == 1 ? t - 1 : (t - 1) >> 1;          // output row an odd (S = 2) / any (S = 1) input row closes
      const bool emits = (S == 1 || (t & 1)) && r_emit >= ro0 && r_emit < ro1;
      float* rbuf = rowbuf + (r_emit & 1) * rb_stride;
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        const int ct = cgi * CW + j;
        const float* kc = ldsK + (ct * 32 + i32) * 13;
        // a finished row of this lane's channel -> LDS row buffer (the statistic is taken when the row leaves it)
        auto finish_store = [&](const float (&sum)[NO]) __attribute__((always_inline)) {
          if (!emits) return;
          float* dst = rbuf + (ct * 32 + i32) * g.pitch + obase;
          float mrow = 0.0f;                        // NS: the row's maximum over this lane's true outputs
          const float b2 = kDwLds ? kc[9] : k_b2[j], bsc2 = kDwLds ? kc[10] : k_bsc2[j], bsh2 = kDwLds ? kc[11] : k_bsh2[j];
#pragma unroll
          for (int k = 0; k < NO; ++k) {
            float o;
            if (FAST == 0) {
              o = dw_finish<kEpiRuntime>(sum[k], has_b2, b2, has_bn2, bsc2, bsh2, act2);
            } else {
              o = sum[k] * bsc2;
              o = o + bsh2;
              o = __builtin_amdgcn_fmed3f(o, 0.0f, top);      // = min(max(o, 0), top), a NaN gives 0 either way
            }
            if constexpr (NS != 0) {
              // (own pixel 0 is an output of the upper half only, pixel 15 of the lower half only; the narrow plane's columns
              // left of the image - pixels 0 .. LZ of the lower half - are none)
              const bool is_out = k == 0 ? h == 1 : (k == NO - 1 ? h == 0 : (LZ == 0 || k > LZ || h == 1));
              mrow = fmaxf(mrow, is_out ? fabsf(o) : 0.0f);
            } else if (S == 1 && k == 0) {
              if (h == 1) dst[k] = o;
            } else if (k == NO - 1) {
              if (h == 0) dst[k] = o;
            } else {
              dst[k] = o;
            }
          }
          if constexpr (NS != 0) m = fmaxf(m, mrow);
        };
        if (!row_ok) {
          // a row of zero padding adds nothing to any sum (every product is +-0 and the sums are never -0): the row it
          // closes leaves, the open sums move up
          if (S == 1) {
            finish_store(sumA[j]);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              sumA[j][k] = sumB[j][k];
              sumB[j][k] = 0.0f;
            }
          } else if (t & 1) {
            finish_store(sumA[j]);
#pragma unroll
            for (int c = 0; c < 8; ++c) sumA[j][c] = 0.0f;
          }
          FQ_PIN();
          continue;
        }
        float e[18];                                // dequantised pointwise outputs: e[k + 1] = own pixel k, e[0] / e[17] the neighbours'
        float cf[NS ? 18 : 1];                      // NS: their codes (whole numbers), the same places
        {
          // (the re-centring term zoff * rowsum joins AFTER the multiplication: as the accumulator's initial value it is a
          // loop-invariant 16-register splat per channel tile, which the compiler keeps alive across the whole row loop)
          v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          int wl = lane;                             // (opaque per row: the weight fragments are re-read from LDS, not kept in
          asm volatile("" : "+v"(wl));               //  CW * KT * 4 registers across the row loop)
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[kt], ldsW[((ct * KT + kt) << 6) + wl], acc, 0, 0, 0);
          // (the fused-inference chain two pixels at a time as packed fp32 instructions - 64 instead of 128 per channel tile and
          // row - was measured 2 % SLOWER: pair 1 98.0 against 95.9 us, the step -0.36 %, profiles/r6_pwdw_packed_ab.txt)
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            float v = (float)(acc[k] + k_zs[j]) * k_sxw[j];
            if (FAST == 0) {
              if (has_b1) v = v + k_b1[j];
              if (has_bn1) {
                v = v * k_bsc1[j];
                v = v + k_bsh1[j];
              }
              v = act_rt(v, act1);
              const float code = NN ? truncf(fast_quot(fq_clip(v, q2), fq2) + 0.49999997f) : fq_code(v, q2);
              e[k + 1] = code * q2.scale;
              if constexpr (NS != 0) cf[k + 1] = code;
            } else {
              v = v * k_bsc1[j];
              v = v + k_bsh1[j];
              // clip(relu(v), 0, hi) = med3(v, 0, hi); the quotient is non-negative: roundf = trunc(Q + pred(0.5))
              const float code = NN ? truncf(fast_quot(fq_clip(v, qc), fq2) + 0.49999997f)
                                    : fq_code(act_rt(v, relu6 ? FQ_ACT_RELU6 : FQ_ACT_RELU), q2);
              e[k + 1] = code * q2.scale;
              if constexpr (NS != 0) cf[k + 1] = code;
            }
          }
          if constexpr (NS != 0) {
            // the codes leave (above: which columns go where).  NN: they are 0 .. 255 and v_cvt_pk_u8_f32 puts one into its
            // byte; else the low byte of the integer (two's complement for a signed quantiser)
            const auto sc = __builtin_amdgcn_permlane32_swap(__float_as_uint(cf[1]), __float_as_uint(cf[16]), false, false);
            cf[0] = __uint_as_float(sc[0]);
            cf[17] = __uint_as_float(sc[1]);
            auto pk4 = [&](float a, float b, float c, float d) __attribute__((always_inline)) {
              if constexpr (NN) {
                unsigned u = __builtin_amdgcn_cvt_pk_u8_f32(a, 0, 0u);
                u = __builtin_amdgcn_cvt_pk_u8_f32(b, 1, u);
                u = __builtin_amdgcn_cvt_pk_u8_f32(c, 2, u);
                return (int)__builtin_amdgcn_cvt_pk_u8_f32(d, 3, u);
              } else {
                return (int)(((unsigned)(int)a & 255u) | (((unsigned)(int)b & 255u) << 8) | (((unsigned)(int)c & 255u) << 16) |
                             ((unsigned)(int)d << 24));
              }
            };
            typedef int v3i __attribute__((ext_vector_type(3)));
            typedef unsigned v3u __attribute__((ext_vector_type(3)));
            v3i d3;
            int dx;
            if (ns_par2) {
              d3 = (v3i){pk4(cf[4], cf[5], cf[6], cf[7]), pk4(cf[8], cf[9], cf[10], cf[11]), pk4(cf[12], cf[13], cf[14], cf[15])};
              dx = pk4(h ? cf[0] : cf[2], h ? cf[1] : cf[3], cf[2], cf[3]);
            } else {
              d3 = (v3i){pk4(cf[2], cf[3], cf[4], cf[5]), pk4(cf[6], cf[7], cf[8], cf[9]), pk4(cf[10], cf[11], cf[12], cf[13])};
              dx = pk4(cf[14], cf[15], cf[16], cf[17]);
            }
            const unsigned rowb = (unsigned)((ct * 32 + i32) * HW + t * g.W);
            if (ns_ok3) {
              __builtin_amdgcn_raw_buffer_store_b96(__builtin_bit_cast(v3u, d3), rsy, (int)(rowb + (unsigned)ns_col3), 0, 0);
              asm volatile("s_nop 1" : : "v"(d3));         // (fq_common.h at buf_st_v4f: the data registers of a wide store)
            }
            if (ns_okx) {
              if (ns_x4) __builtin_amdgcn_raw_buffer_store_b32((unsigned)dx, rsy, (int)(rowb + (unsigned)ns_colx), 0, 0);
              else __builtin_amdgcn_raw_buffer_store_b16((unsigned short)dx, rsy, (int)(rowb + (unsigned)ns_colx), 0, 0);
            }
          }
          // the zero padding of the depthwise layer: columns left / right of the image
          e[1 + (LZ & 15)] = zero_left ? 0.0f : e[1 + (LZ & 15)];
          if (S == 1) e[16] = zero_right ? 0.0f : e[16];
          // column 16 h - 1 and 16 h + 16: the other half's pixel 15 / pixel 0
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(e[1]), __float_as_uint(e[16]), false, false);
          e[0] = __uint_as_float(sw[0]);             // upper half: the lower half's pixel 15 (lower half: its own pixel 0, unused)
          e[17] = __uint_as_float(sw[1]);            // lower half: the upper half's pixel 0 (upper half: its own pixel 15, unused)
        }
        float w[9];
        if (!kDwLds) {
#pragma unroll
          for (int t = 0; t < 9; ++t) w[t] = k_w[j][t];
        }
        if (S == 1) {
          // A: += tap row 2 -> output row t - 1 complete; B: += tap row 1; C (new): tap row 0 from +0
          w[6] = kc[6]; w[7] = kc[7]; w[8] = kc[8];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            float a = sumA[j][k];
            a = fmaf(w[6], e[k], a);
            a = fmaf(w[7], e[k + 1], a);
            a = fmaf(w[8], e[k + 2], a);
            sumA[j][k] = a;
          }
          finish_store(sumA[j]);
          w[0] = kc[0]; w[1] = kc[1]; w[2] = kc[2]; w[3] = kc[3]; w[4] = kc[4]; w[5] = kc[5];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            float b = sumB[j][k];
            b = fmaf(w[3], e[k], b);
            b = fmaf(w[4], e[k + 1], b);
            b = fmaf(w[5], e[k + 2], b);
            float c = 0.0f;
            c = fmaf(w[0], e[k], c);
            c = fmaf(w[1], e[k + 1], c);
            c = fmaf(w[2], e[k + 2], c);
            sumA[j][k] = b;
            sumB[j][k] = c;
          }
        } else {
          // output oc = 8 h + c: columns p = 2c, 2c + 1, 2c + 2 of the own 16 (+ the neighbour's first) = e[2c + 1 .. 2c + 3]
          if (t & 1) {                              // t = 2r + 1: tap row 2 of output r, then tap row 0 of output r + 1
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              float a = sumA[j][c];
              a = fmaf(w[6], e[2 * c + 1], a);
              a = fmaf(w[7], e[2 * c + 2], a);
              a = fmaf(w[8], e[2 * c + 3], a);
              sumA[j][c] = a;
            }
            finish_store(sumA[j]);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              float a = 0.0f;
              a = fmaf(w[0], e[2 * c + 1], a);
              a = fmaf(w[1], e[2 * c + 2], a);
              a = fmaf(w[2], e[2 * c + 3], a);
              sumA[j][c] = a;
            }
          } else {                                  // t = 2r: tap row 1 of output r
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              float a = sumA[j][c];
              a = fmaf(w[3], e[2 * c + 1], a);
              a = fmaf(w[4], e[2 * c + 2], a);
              a = fmaf(w[5], e[2 * c + 3], a);
              sumA[j][c] = a;
            }
          }
        }
        FQ_PIN();                                   // (one channel tile after the other: their registers need not coexist)
      }
      // ---- a finished output row leaves: LDS row buffer -> whole rows, 16 / 8 / 4 bytes per lane; its maximum on the way ----
      if (NS == 0 && emits) {
        __syncthreads();
        const unsigned per_row = g.qv.d;                      // vectors per channel row
        const int vecs = g.Cout * (int)per_row;
        float* yr = yb + (int64_t)r_emit * g.Wo;
        for (int idx = threadIdx.x; idx < vecs; idx += blockDim.x) {
          const unsigned c = fast_div((unsigned)idx, g.qv), qd = (unsigned)idx - c * per_row;
          if (g.vw == 4) {
            const float* src = rbuf + c * g.pitch + 4 * qd;
            const f4 v = (f4){src[0], src[1], src[2], src[3]};
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            *reinterpret_cast<f4*>(yr + (int64_t)c * g.Ho * g.Wo + 4 * qd) = v;
          } else if (g.vw == 2) {
            const float* src = rbuf + c * g.pitch + 2 * qd;
            const float2 v = make_float2(src[0], src[1]);
            m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
            *reinterpret_cast<float2*>(yr + (int64_t)c * g.Ho * g.Wo + 2 * qd) = v;
          } else {
            const float v = rbuf[c * g.pitch + qd];
            m = fmaxf(m, fabsf(v));
            yr[(int64_t)c * g.Ho * g.Wo + qd] = v;
          }
        }
      }
    };
    // rows in groups whose ring phases are static: U rows per turn, U * KT a multiple of NB
    constexpr int U = CODES ? NR : ((KT % NB == 0) ? 1 : ((2 * KT) % NB == 0 ? 2 : NB));
    static_assert(U <= 3, "the row loop below unrolls at most three phases");
    using std::integral_constant;
    for (int t = t_first; t <= t_last; t += U) {
      row(t, integral_constant<int, 0>{});
      if (U > 1 && t + 1 <= t_last) row(t + 1, integral_constant<int, 1 % U>{});
      if (U > 2 && t + 2 <= t_last) row(t + 2, integral_constant<int, 2 % U>{});
    }
  };
  using std::false_type;
  using std::true_type;
  if (fq_nonneg(q1) && fq_nonneg(q2) && fq1.ok && fq2.ok) body(true_type{});
  else body(false_type{});

  if (stat_out != nullptr) {
    m = wave_max_nonneg(m);
    __syncthreads();
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      float mm = 0.0f;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) mm = fmaxf(mm, red[w]);
      if (__float_as_uint(mm) != 0u) FQ_STAT_FLUSH_MAX(reinterpret_cast<unsigned*>(stat_out) + smp, __float_as_uint(mm));
    }
  }
}

// test hook (fq_debug_fast_quotient): the quotient the recompute kernels divide with, element by element
__global__ void fast_quotient_kernel(const float* __restrict__ c, int64_t n, const float* __restrict__ d, float* __restrict__ out,
                                     int* __restrict__ ok_out) {
  const FastQuot f = make_fast_quot(d[0]);
  const double rden = 1.0 / (double)d[0];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) ok_out[0] = f.ok ? 1 : 0;
  if (i < n) out[i] = f.ok ? fast_quot(c[i], f) : ieee_div_by(c[i], rden);
}

struct PwDwPlan {
  int kt, cw, lz, strips, ctg, bands, rb, pitch, threads;
  size_t lds;
  bool ok;
};

PwDwPlan pwdw_plan(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, int stride) {
  PwDwPlan p;
  memset(&p, 0, sizeof(p));
  if (n <= 0 || cin <= 0 || cout <= 0 || h < 3 || w < 8 || (stride != 1 && stride != 2)) return p;
  if (cout % 32 != 0 || (stride == 2 && (w % 2 != 0 || h % 2 != 0))) return p;
  const int kt = (int)((cin + 31) / 32), ct = (int)(cout / 32);
  if (!(kt == 1 || kt == 2 || kt == 4 || kt == 8)) return p;
  const int wo = (int)((w - 1) / stride + 1), ho = (int)((h - 1) / stride + 1);
  p.kt = kt;
  p.cw = ct % 2 == 0 ? 2 : 1;
  p.strips = (int)((w + 29) / 30);
  p.lz = (stride == 1 && p.strips == 1) ? (int)(30 - w) : 0;
  if (!(p.lz == 0 || p.lz == 2)) return p;                  // (instantiated: planes from 30 columns up, and 28)
  p.ctg = ct / p.cw;
  p.threads = 64 * p.strips * p.ctg;
  if (p.threads > 512) return p;
  // row-buffer pitch: the widest column any lane writes (invalid outputs past the plane included) + the columns left of it
  const int reach = stride == 1 ? (int)w + 2 + p.lz : 15 * p.strips + 1;
  p.pitch = (reach > wo ? reach : wo) + p.lz;
  p.pitch |= 1;
  p.lds = pwdw_lds(ct, kt, (int)cout, p.pitch, stride, false);     // (the storing launch's: it admits the shape and sizes the bands)
  if (p.lds + 10 * 1024 > (size_t)max_lds_bytes()) return p;
  // rows per band: the bands of all samples should fill the chip's workgroup slots (two wavefronts per SIMD by registers, the
  // row buffers by LDS) in as few rounds as possible, a band re-computing the one or two pointwise rows above / below it.
  // (MobileNet1.0 at batch 128: 14 rows per band on the 56-row outputs - 512 workgroups - and 7 on the 28-row ones; measured
  // with 14 / 10 / 7: profiles/r6_pwdw_bands.txt)
  // (FQ_PWDW_RB forces them; read at every call, like FQ_PWSTAT_FRONT_ROWS, so that a test can vary it inside one process)
  const char* rb_e = getenv("FQ_PWDW_RB");
  const int rb_env = rb_e != nullptr ? atoi(rb_e) : 0;
  {
    const int waves = p.threads / 64;
    int occ = (int)((160 * 1024) / (p.lds + 512));
    const int by_regs = 8 / waves > 0 ? 8 / waves : 1;
    occ = occ < by_regs ? occ : by_regs;
    occ = occ < 1 ? 1 : occ;
    const double slots = (double)num_cu() * occ;
    double best = 1e30;
    int best_rb = ho;
    for (int b = 1; b <= ho; ++b) {
      const int rb = (ho + b - 1) / b, bands = (ho + rb - 1) / rb;
      const double wgs = (double)n * bands, rounds = ceil(wgs / slots), fill = wgs < slots ? wgs / slots : 1.0;
      const double cost = rounds * (stride * rb + 2) / fill;
      if (cost < best - 1e-9) {
        best = cost;
        best_rb = rb;
      }
    }
    p.rb = rb_env > 0 ? (rb_env < ho ? rb_env : ho) : best_rb;
  }
  p.bands = (ho + p.rb - 1) / p.rb;
  if (n * cin * h * w * 4 >= (1ll << 32) || n * cout * ho * wo >= (1ll << 31)) return p;
  p.ok = true;
  return p;
}

}  // namespace

using namespace fqi;

extern "C" {

int fq_debug_fast_quotient(const float* c, int64_t n, const float* d, float* out, int* took_fast_path, fqStream_t stream) {
  FQ_REQUIRE(c && d && out && took_fast_path && n > 0, "fq_debug_fast_quotient: null pointer");
  hipLaunchKernelGGL(fast_quotient_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, n, d, out,
                     took_fast_path);
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}

int fq_pwdw_fused_supported(int64_t n, int64_t cin, int64_t cout, int64_t h, int64_t w, int stride, int stat_mode) {
  if (stat_mode != 0 && !(stride == 1 && w % 4 == 0 && n * cout * h * w < (1ll << 31))) return 0;
  return pwdw_plan(n, cin, cout, h, w, stride).ok ? 1 : 0;
}

}  // extern "C"

// one instantiation's launch: it owns the raised dynamic LDS limit; `args` are pwdw_kernel's, written out by the one caller
template <int KT, int CW, int S, int LZ, int FAST, int CODES, int NS, class... Args>
static int pwdw_go(unsigned grid, int threads, size_t lds, hipStream_t st, int rb, Args... args) {
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&pwdw_kernel<KT, CW, S, LZ, FAST, CODES, NS>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) == hipSuccess;
  FQ_REQUIRE(attr_ok, "fq_pwdw_fused: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((pwdw_kernel<KT, CW, S, LZ, FAST, CODES, NS>), dim3(grid), dim3((unsigned)threads), lds, st, args...);
  note_launch(FQ_KERNEL_DWCONV, FQ_LAUNCH_PAIR, {KT, CW, S, LZ, FAST, CODES, NS, rb});
  return FQ_OK;
}

// fq_pwdw_fused: y, or mid_codes_out instead of y - the statistic mode, NS of pwdw_kernel
extern "C" int fq_pwdw_fused(const float* x, const int8_t* wcodes, const float* wscale, const int32_t* wsum, const float* pw_bias,
                             int64_t n, int64_t cin, int64_t cin_pad, int64_t cout_pad, int64_t cout, int64_t h, int64_t w,
                             const float* in_stat, const float* in_thr, int in_width, unsigned in_flags, const float* pw_bn_scale,
                             const float* pw_bn_shift, int pw_act, const float* mid_stat, const float* mid_thr, int mid_width,
                             unsigned mid_flags, float* mid_current_max, const float* dw_w, const float* dw_bias, int dw_stride,
                             const float* dw_bn_scale, const float* dw_bn_shift, int dw_act, float* y, float* stat_out,
                             const void* x_codes, fqStream_t stream, void* mid_codes_out) {
  const bool ns = mid_codes_out != nullptr;
  FQ_REQUIRE((x || x_codes) && wcodes && wscale && wsum && dw_w && (y || ns), "fq_pwdw_fused: null pointer");
  if (ns) {
    FQ_REQUIRE(y == nullptr && stat_out && x_codes && dw_stride == 1 && aligned16(mid_codes_out),
               "fq_pwdw_fused: the statistic mode (mid_codes_out) wants y == NULL, stat_out, x_codes, stride 1 and a 16-byte aligned buffer");
    FQ_REQUIRE(w % 4 == 0 && mid_width <= 8 && ((mid_flags & FQ_ACT_SIGNED) || !(mid_flags & FQ_ACT_LO_NEG_MAX)) &&
                   n * cout * h * w < (1ll << 31) && cout * h * w < (1ll << 31) - 64,
               "fq_pwdw_fused: statistic mode: shape or quantiser not taken (rows of whole dwords, codes that fit a byte): see "
               "fq_pwdw_fused_supported(..., stat_mode = 1)");
  }
  FQ_REQUIRE(in_stat != nullptr || in_thr != nullptr, "fq_pwdw_fused: give in_stat (online) or in_thr (offline)");
  FQ_REQUIRE(mid_stat != nullptr || mid_thr != nullptr, "fq_pwdw_fused: give mid_stat (the per-sample maxima of the pointwise "
             "output, from fq_pwconv_i8_stat) or mid_thr (a stored threshold)");
  FQ_REQUIRE(in_width >= 2 && in_width <= 8, "fq_pwdw_fused: input width %d does not fit int8 codes", in_width);
  FQ_REQUIRE(mid_width >= 2 && mid_width <= 16, "fq_pwdw_fused: bad width %d of the depthwise input", mid_width);
  FQ_REQUIRE(!((in_flags | mid_flags) & (FQ_ACT_NO_ABS | FQ_ACT_NO_EPS)), "fq_pwdw_fused: unsupported activation flags");
  FQ_REQUIRE((pw_bn_scale == nullptr) == (pw_bn_shift == nullptr) && (dw_bn_scale == nullptr) == (dw_bn_shift == nullptr),
             "fq_pwdw_fused: a BatchNorm's scale and shift go together");
  FQ_REQUIRE(cin_pad >= cin && cin_pad % 64 == 0 && cout_pad >= cout && cout_pad % 32 == 0,
             "fq_pwdw_fused: cin_pad / cout_pad must be those of fq_weight_codes");
  const bool prezeroed = (dw_act & FQ_STAT_PREZEROED) != 0;
  dw_act &= ~FQ_STAT_PREZEROED;
  FQ_REQUIRE(pw_act >= FQ_ACT_NONE && pw_act <= FQ_ACT_RELU6 && dw_act >= FQ_ACT_NONE && dw_act <= FQ_ACT_RELU6,
             "fq_pwdw_fused: unknown activation");
  FQ_REQUIRE(aligned16(wcodes) && (x_codes ? aligned16(x_codes) : aligned16(x)) && (ns || aligned16(y)),
             "fq_pwdw_fused: x (x_codes when given), wcodes and y must be 16-byte aligned");
  const PwDwPlan p = pwdw_plan(n, cin, cout, h, w, dw_stride);
  FQ_REQUIRE(p.ok, "fq_pwdw_fused: shape not taken (n=%lld cin=%lld cout=%lld %lldx%lld stride %d): see fq_pwdw_fused_supported",
             (long long)n, (long long)cin, (long long)cout, (long long)h, (long long)w, dw_stride);
  hipStream_t st = (hipStream_t)stream;
  const int64_t ho = (h - 1) / dw_stride + 1, wo = (w - 1) / dw_stride + 1;
  if (stat_out && !prezeroed) FQ_HIP(hipMemsetAsync(stat_out, 0, n * sizeof(float), st));
  PwDwGeom g;
  g.Cin = (int)cin; g.KTS = (int)(cin_pad / 32); g.Cout = (int)cout; g.H = (int)h; g.W = (int)w; g.Ho = (int)ho; g.Wo = (int)wo;
  g.strips = p.strips; g.ctg = p.ctg; g.bands = p.bands; g.RB = p.rb;
  g.zoff = (in_flags & FQ_ACT_SIGNED) ? 0 : 128;
  g.pitch = p.pitch;
  g.vw = wo % 4 == 0 ? 4 : (wo % 2 == 0 ? 2 : 1);
  g.qv = fast_div_for((unsigned)(wo / g.vw));
  const int8_t* wfrag = wcodes + cout_pad * cin_pad;
  const float levels1 = act_levels(in_width, in_flags), levels2 = act_levels(mid_width, mid_flags);
  const int lo1 = (in_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0, lo2 = (mid_flags & FQ_ACT_LO_NEG_MAX) ? 1 : 0;
  // the fused-inference case as a compile-time epilogue
  int fast = 0;
  if (!pw_bias && !dw_bias && pw_bn_scale && dw_bn_scale && !lo1 && !lo2 && pw_act == dw_act &&
      (pw_act == FQ_ACT_RELU || pw_act == FQ_ACT_RELU6))
    fast = 1;
  static const int no_fast = env_int("FQ_PWDW_NO_FAST", 0);
  if (no_fast) fast = 0;
  // algorithmic bytes: those of the depthwise layer this launch stands for (its input is never written: SURVEY.md 8d counts
  // what the layer's arithmetic needs); moved: what the launch really reads and writes
  const double in_elems = (double)n * cin * h * w, mid_elems = (double)n * cout * h * w, out_elems = (double)n * cout * ho * wo;
  // (code input: 16 bytes per pixel and 16-channel block of whole 32-channel slabs instead of 4 per element)
  // (the statistic mode stands for the same layer - the algorithmic bytes stay the layer's, DESIGN 3.7 - and moves the codes
  // of its input out, the halo rows of every band twice, where the storing mode moves the output)
  const double in_moved = x_codes ? 32.0 * p.kt * (double)n * h * w : 4.0 * in_elems;
  const double out_moved = ns ? (double)n * cout * w * (h + 2.0 * (p.bands - 1)) : 4.0 * out_elems;
  ProfScope prof(FQ_KERNEL_DWCONV, 4.0 * (mid_elems + out_elems), st, in_moved + out_moved);
  const int8_t* xc = static_cast<const int8_t*>(x_codes);
  const unsigned grid = (unsigned)(n * p.bands);
  // (the statistic mode has no row buffers: weight fragments and the depthwise layer's constants only)
  const size_t lds = ns ? pwdw_lds((int)(cout / 32), p.kt, (int)cout, p.pitch, dw_stride, true) : p.lds;
  float* const y_arg = ns ? static_cast<float*>(mid_codes_out) : y;
  // the instantiations: every (KT, CW) x (stride 1 with LZ 0 / 2, stride 2) x epilogue x input kind, and the statistic mode
  // for stride 1 on code input (what the checks above and pwdw_plan admit)
  int rc = FQ_OK;
  pair_pick<1, 2, 4, 8>(p.kt, [&](auto kt_c) {
    pair_pick<1, 2>(p.cw, [&](auto cw_c) {
      pair_pick<1, 2>(dw_stride, [&](auto s_c) {
        pair_pick<0, 2>(p.lz, [&](auto lz_c) {
          pair_pick<0, 1>(fast, [&](auto fast_c) {
            pair_pick<0, 1>(xc != nullptr ? 1 : 0, [&](auto codes_c) {
              pair_pick<0, 1>(ns ? 1 : 0, [&](auto ns_c) {
                constexpr int KT = decltype(kt_c)::value, CW = decltype(cw_c)::value, S = decltype(s_c)::value,
                              LZ = decltype(lz_c)::value, FAST = decltype(fast_c)::value, CODES = decltype(codes_c)::value,
                              NS = decltype(ns_c)::value;
                if constexpr ((S == 1 || LZ == 0) && (NS == 0 || (S == 1 && CODES == 1)))
                  rc = pwdw_go<KT, CW, S, LZ, FAST, CODES, NS>(
                      grid, p.threads, lds, st, p.rb, x, xc, wfrag, wscale, (const int*)wsum, pw_bias, g, in_stat, (int)n, in_thr,
                      levels1, lo1, kEps, pw_bn_scale, pw_bn_shift, pw_act, mid_stat, mid_thr, levels2, lo2, mid_current_max,
                      dw_w, dw_bias, dw_bn_scale, dw_bn_shift, dw_act, y_arg, stat_out);
              });
            });
          });
        });
      });
    });
  });
  if (rc != FQ_OK) return rc;
  FQ_LAUNCH_CHECK();
  return FQ_OK;
}
