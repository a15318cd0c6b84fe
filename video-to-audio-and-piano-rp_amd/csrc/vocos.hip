// The Vocos vocoder (mel variant, padding = "center"): mel frames -> wave, the decoder behind `E2TTS.vocos` of a model whose latents are
// log-mel frames (Vocos.from_pretrained('charactr/vocos-mel-24khz'), e2_tts_crossatt.py:1324, e2_tts_crossatt6.py:1469; x3:2275-2287).
//
// Activations are time-major fp32 rows; frame t of clip b is row b * rows_per_clip + t with rows_per_clip = T + 6, so that the embed
// convolution (k = 7, zero pad 3) is an exact-fp32 v2a_gemm over overlapping rows of the staged input (lda = C_pad, K = 7 C_pad: the
// Encodec encoder's trick).  The six rows between two clips are computed by the GEMMs and never read.  The GEMMs (embed, pwconv1,
// pwconv2, head, inverse DFT against a host basis) and the two plain LayerNorms (v2a_clip_layernorm) are the library's.  The exact-fp32
// GEMM adds its K products in one chain whose error grows with K (at K = 1536 a block of the 24 kHz network came out 4.5 times further from
// float64 than torch's CPU fp32; at K <= 224 level with it), so vocos.py cuts every K into chunks of 256, chunk c added to the sum of the
// chunks before it by the RESID epilogue -- which leaves GELU and the layer scale to two pointwise kernels.  Six kernels stand around:
//   * stage_in:    (B, C, T) channel-major -> rows of C_pad floats with a 3-row zero border per clip, through a 32 x 32 LDS transpose
//                  (reads run along time, writes along channels).  Channels >= C and frames >= lens[b] are zero.
//   * dwconv_ln:   the depthwise 7-tap convolution, zero padded at each clip's own ends, and the LayerNorm behind it.  A workgroup
//                  stages a tile of frames plus 6 halo rows in LDS (16-byte loads); a wave takes a frame, a lane 4 channels per 256; the
//                  taps are one fmaf chain in tap order from the bias, mean and centred variance go through wave reductions.
//   * gelu, scale_residual: x = gelu(x) in place (exact erf form); out = fma(gamma, p, resid), layer scale and residual.  16-byte accesses.
//   * spectrum:    head logits -> interleaved (re, im) rows: min(exp(m), 100) (cos p + i sin p), evaluated in double from the fp32
//                  logits and rounded once, K pad zeroed.
//   * overlap_add: torch.istft's overlap-add in gather form, one thread per output sample: frames (already windowed by the basis)
//                  added in ascending t, divided by the envelope summed in the same loop from a w^2 table.
// No atomics anywhere: a value depends on its clip's frames alone, not on the batch, the tile or the other clips.
#include "v2a_common.h"

#include <math.h>

namespace {

constexpr int VOC_THREADS = 256;
constexpr int VOC_TAPS = 7, VOC_HALO = 3;
constexpr int VOC_TF_MAX = 16;                      // frames of a dwconv_ln tile: 22 rows of 512 floats = 44 KB of LDS
constexpr int VOC_LDS_FLOATS = 16384;               // 64 KB: (tf + 6) * d floats must fit
constexpr int VOC_NV = V2A_VOCOS_MAX_DIM / 256;     // float4 groups of a lane at the widest d; 2 of them serve d <= 512

__global__ __launch_bounds__(VOC_THREADS) void vocos_stage_in_kernel(const float* __restrict__ x, int64_t xbs, int64_t xcs, int32_t C, int32_t T,
                                                                     const int32_t* __restrict__ lens, float* __restrict__ out, int32_t c_pad) {
  __shared__ float tile[32][33];
  const int clip = blockIdx.z;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;              // staged row (frame + 3) and channel of the tile's corner
  int len = lens ? lens[clip] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += VOC_THREADS / 32) {                  // lanes along time
    const int c = c0 + i, t = r0 + tx - VOC_HALO;
    tile[i][tx] = (c < C && t >= 0 && t < len) ? x[clip * xbs + c * xcs + t] : 0.0f;
  }
  __syncthreads();
  const int64_t rows = (int64_t)T + 2 * VOC_HALO;
  for (int i = ty; i < 32; i += VOC_THREADS / 32) {                  // lanes along channels
    const int r = r0 + i, c = c0 + tx;
    if (r < rows && c < c_pad) out[(clip * rows + r) * c_pad + c] = tile[tx][i];
  }
}

struct DwLnParams {
  const float *x, *wt, *bias, *gamma, *beta;
  const int32_t* lens;
  float* y;
  int64_t ldx, ldy, rows_per_clip;
  int32_t T, d, tf;
  float eps;
};

template <int NV>        // float4 groups of a lane: d <= 256 NV
__global__ __launch_bounds__(VOC_THREADS) void vocos_dwconv_ln_kernel(DwLnParams P) {
  extern __shared__ __attribute__((aligned(16))) float xs[];          // [tf + 6][d]: frames t0 - 3 .. t0 + tf + 2, zero outside [0, len)
  const int clip = blockIdx.y, t0 = blockIdx.x * P.tf, d = P.d;
  int len = P.lens ? P.lens[clip] : P.T;
  len = len < 0 ? 0 : (len > P.T ? P.T : len);
  const int nf = P.T - t0 < P.tf ? P.T - t0 : P.tf;                  // rows of this tile inside the clip's T rows
  const int64_t row0 = (int64_t)clip * P.rows_per_clip;
  const int d4 = d >> 2;
  if (t0 < len) {
    for (int i = threadIdx.x; i < (nf + 2 * VOC_HALO) * d4; i += VOC_THREADS) {
      const int r = i / d4, c = (i - r * d4) << 2, t = t0 + r - VOC_HALO;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < len) v = *reinterpret_cast<const f32x4*>(P.x + (row0 + t) * P.ldx + c);
      *reinterpret_cast<f32x4*>(xs + r * d + c) = v;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_d = 1.0f / (float)d;
  for (int f = wave; f < nf; f += VOC_THREADS / V2A_WAVE) {
    float* yrow = P.y + (row0 + t0 + f) * P.ldy;
    if (t0 + f >= len) {                                             // behind the clip's frames: a defined operand row, never read back
      for (int c = lane << 2; c < d; c += 256) *reinterpret_cast<f32x4*>(yrow + c) = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    f32x4 v[NV];
    float s = 0.0f;
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int c = (g * 64 + lane) << 2;
      v[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < d) {
        f32x4 acc = *reinterpret_cast<const f32x4*>(P.bias + c);
#pragma unroll
        for (int j = 0; j < VOC_TAPS; ++j) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(P.wt + j * d + c);
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + (f + j) * d + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(w[e], xv[e], acc[e]);
        }
        v[g] = acc;
        s += (acc[0] + acc[1]) + (acc[2] + acc[3]);
      }
    }
    const float mean = wave_sum(s) * inv_d;
    float q = 0.0f;
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int c = (g * 64 + lane) << 2;
      if (c < d) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[g][e] -= mean;
          q = __fmaf_rn(v[g][e], v[g][e], q);
        }
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + P.eps);
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int c = (g * 64 + lane) << 2;
      if (c < d) {
        const f32x4 ga = *reinterpret_cast<const f32x4*>(P.gamma + c), be = *reinterpret_cast<const f32x4*>(P.beta + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fmaf_rn(v[g][e] * rstd, ga[e], be[e]);
        *reinterpret_cast<f32x4*>(yrow + c) = o;
      }
    }
  }
}

// MODE 0: x = gelu(x) (exact erf form), in place.  MODE 1: out = fma(gamma[c], p, resid): layer scale and residual.
template <int MODE>
__global__ __launch_bounds__(VOC_THREADS) void vocos_pointwise_kernel(const float* p, int64_t ldp, const float* gamma, const float* resid, int64_t ldr,
                                                                      float* out, int64_t ldo,      // out may be p (MODE 0) or resid (MODE 1)
                                                                      int64_t rows, int32_t n4) {
  const int64_t i = (int64_t)blockIdx.x * VOC_THREADS + threadIdx.x;
  if (i >= rows * n4) return;
  const int64_t m = i / n4;
  const int c = (int)(i - m * n4) << 2;
  f32x4 v = *reinterpret_cast<const f32x4*>(p + m * ldp + c);
  if (MODE == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
  } else {
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), r = *reinterpret_cast<const f32x4*>(resid + m * ldr + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(g[e], v[e], r[e]);
  }
  *reinterpret_cast<f32x4*>(out + m * ldo + c) = v;
}

__global__ __launch_bounds__(VOC_THREADS) void vocos_spectrum_kernel(const float* __restrict__ logits, int64_t ldl, int64_t rows, int32_t n_bins,
                                                                     float* __restrict__ spec, int64_t lds_, int32_t kpairs) {
  const int64_t i = (int64_t)blockIdx.x * VOC_THREADS + threadIdx.x;
  if (i >= rows * kpairs) return;
  const int64_t m = i / kpairs;
  const int k = (int)(i - m * kpairs);
  f32x2 o = {0.f, 0.f};
  if (k < n_bins) {
    const double lm = (double)logits[m * ldl + k], ph = (double)logits[m * ldl + n_bins + k];
    const double mag = fmin(exp(lm), 100.0);                         // the clip before the product
    o[0] = (float)(mag * cos(ph));
    o[1] = (float)(mag * sin(ph));
  }
  *reinterpret_cast<f32x2*>(spec + m * lds_ + 2 * k) = o;
}

__global__ __launch_bounds__(VOC_THREADS) void vocos_overlap_add_kernel(const float* __restrict__ frames, int64_t ldf, int64_t rows_per_clip,
                                                                        const float* __restrict__ wsq, int32_t T, int32_t n_fft, int32_t hop,
                                                                        const int32_t* __restrict__ lens, float* __restrict__ out, int64_t obs) {
  const int clip = blockIdx.y;
  int len = lens ? lens[clip] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  const int64_t n = (int64_t)blockIdx.x * VOC_THREADS + threadIdx.x;
  if (n >= (int64_t)(len - 1) * hop) return;
  const int64_t p = n + n_fft / 2;                                   // position in the untrimmed overlap-add
  int64_t tlo = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;    // ceil((p - n_fft + 1) / hop)
  int64_t thi = p / hop;
  if (thi > len - 1) thi = len - 1;
  const float* f = frames + (int64_t)clip * rows_per_clip * ldf;
  float acc = 0.0f, env = 0.0f;
  for (int64_t t = tlo; t <= thi; ++t) {
    const int64_t j = p - t * hop;                                   // 0 <= j < n_fft
    acc = __fadd_rn(acc, f[t * ldf + j]);
    env = __fadd_rn(env, wsq[j]);
  }
  out[clip * obs + n] = __fdiv_rn(acc, env);
}

}  // namespace

extern "C" int v2a_vocos_stage_in(const float* x, int64_t x_batch_stride, int64_t x_chan_stride, int32_t B, int32_t C, int32_t T, const int32_t* lens,
                                  float* out, int32_t c_pad, v2a_stream_t stream) {
  V2A_REQUIRE(x && out && x != out, "v2a_vocos_stage_in: null / aliased pointer");
  V2A_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && T >= 1 && T <= V2A_VOCOS_MAX_FRAMES && c_pad >= C && c_pad % 16 == 0 && c_pad <= 65535 * 32,
              "v2a_vocos_stage_in: B=%d C=%d T=%d c_pad=%d (1 <= B <= 65535, 1 <= T <= %d, c_pad >= C a multiple of 16: the K granularity of the "
              "exact-fp32 GEMM behind it)", B, C, T, c_pad, V2A_VOCOS_MAX_FRAMES);
  V2A_REQUIRE(x_chan_stride >= T && x_batch_stride >= (int64_t)(C - 1) * x_chan_stride + T,
              "v2a_vocos_stage_in: x_chan_stride=%lld x_batch_stride=%lld (channels of T=%d frames, clips of C=%d channels)", (long long)x_chan_stride,
              (long long)x_batch_stride, T, C);
  V2A_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 15) == 0 && (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vocos_stage_in: alignment (16 bytes for out)");
  const dim3 grid((unsigned)((T + 2 * VOC_HALO + 31) / 32), (unsigned)((c_pad + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(vocos_stage_in_kernel, grid, dim3(VOC_THREADS), 0, (hipStream_t)stream, x, x_batch_stride, x_chan_stride, C, T, lens, out, c_pad);
  return v2a_check_launch("v2a_vocos_stage_in");
}

extern "C" int v2a_vocos_dwconv_ln(const float* x, int64_t ldx, const float* wt, const float* bias, const float* gamma, const float* beta, float eps,
                                   int32_t B, int32_t T, int64_t rows_per_clip, int32_t d, const int32_t* lens, float* y, int64_t ldy,
                                   v2a_stream_t stream) {
  V2A_REQUIRE(x && wt && bias && gamma && beta && y && x != y, "v2a_vocos_dwconv_ln: null / aliased pointer");
  V2A_REQUIRE(d >= 16 && d % 16 == 0 && d <= V2A_VOCOS_MAX_DIM, "v2a_vocos_dwconv_ln: d=%d (a multiple of 16, 16 .. %d)", d, V2A_VOCOS_MAX_DIM);
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= V2A_VOCOS_MAX_FRAMES && rows_per_clip >= T && ldx >= d && ldy >= d && ldx % 4 == 0 && ldy % 4 == 0,
              "v2a_vocos_dwconv_ln: B=%d T=%d rows_per_clip=%lld ldx=%lld ldy=%lld (1 <= B <= 65535, 1 <= T <= %d, rows_per_clip >= T, row strides "
              ">= d and multiples of 4)", B, T, (long long)rows_per_clip, (long long)ldx, (long long)ldy, V2A_VOCOS_MAX_FRAMES);
  V2A_REQUIRE(eps > 0.0f, "v2a_vocos_dwconv_ln: eps=%g", (double)eps);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) == 0 &&
                  (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vocos_dwconv_ln: alignment (16 bytes)");
  DwLnParams P;
  P.x = x, P.wt = wt, P.bias = bias, P.gamma = gamma, P.beta = beta, P.lens = lens, P.y = y;
  P.ldx = ldx, P.ldy = ldy, P.rows_per_clip = rows_per_clip;
  P.T = T, P.d = d, P.eps = eps;
  const int fit = VOC_LDS_FLOATS / d - 2 * VOC_HALO;                 // >= 2 for d <= 2048
  P.tf = fit < VOC_TF_MAX ? fit : VOC_TF_MAX;
  const size_t lds = (size_t)(P.tf + 2 * VOC_HALO) * d * sizeof(float);
  const dim3 grid((unsigned)((T + P.tf - 1) / P.tf), (unsigned)B);
  if (d <= 512)
    hipLaunchKernelGGL(vocos_dwconv_ln_kernel<2>, grid, dim3(VOC_THREADS), lds, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL(vocos_dwconv_ln_kernel<VOC_NV>, grid, dim3(VOC_THREADS), lds, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vocos_dwconv_ln");
}

extern "C" int v2a_vocos_gelu(float* x, int64_t ldx, int64_t rows, int32_t n, v2a_stream_t stream) {
  V2A_REQUIRE(x != nullptr, "v2a_vocos_gelu: null pointer");
  V2A_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31) && n >= 4 && n % 4 == 0 && n <= (1 << 20) && ldx >= n && ldx % 4 == 0,
              "v2a_vocos_gelu: rows=%lld n=%d ldx=%lld (1 <= rows < 2^31, n a multiple of 4 up to 2^20, ldx >= n a multiple of 4)", (long long)rows, n,
              (long long)ldx);
  V2A_REQUIRE(((uintptr_t)x & 15) == 0, "v2a_vocos_gelu: alignment (16 bytes)");
  const int64_t blocks = (rows * (n / 4) + VOC_THREADS - 1) / VOC_THREADS;
  V2A_REQUIRE(blocks < ((int64_t)1 << 31), "v2a_vocos_gelu: rows=%lld x n=%d is more than one launch takes", (long long)rows, n);
  hipLaunchKernelGGL(vocos_pointwise_kernel<0>, dim3((unsigned)blocks), dim3(VOC_THREADS), 0, (hipStream_t)stream, x, ldx, nullptr, nullptr, 0, x, ldx, rows,
                     n / 4);
  return v2a_check_launch("v2a_vocos_gelu");
}

extern "C" int v2a_vocos_scale_residual(const float* p, int64_t ldp, const float* gamma, const float* resid, int64_t ldr, float* out, int64_t ldo,
                                        int64_t rows, int32_t n, v2a_stream_t stream) {
  V2A_REQUIRE(p && gamma && resid && out && out != p, "v2a_vocos_scale_residual: null / aliased pointer");
  V2A_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31) && n >= 4 && n % 4 == 0 && n <= (1 << 20) && ldp >= n && ldr >= n && ldo >= n && ldp % 4 == 0 &&
                  ldr % 4 == 0 && ldo % 4 == 0,
              "v2a_vocos_scale_residual: rows=%lld n=%d ldp=%lld ldr=%lld ldo=%lld (1 <= rows < 2^31, n a multiple of 4 up to 2^20, row strides >= n and "
              "multiples of 4)", (long long)rows, n, (long long)ldp, (long long)ldr, (long long)ldo);
  V2A_REQUIRE((((uintptr_t)p | (uintptr_t)gamma | (uintptr_t)resid | (uintptr_t)out) & 15) == 0, "v2a_vocos_scale_residual: alignment (16 bytes)");
  const int64_t blocks = (rows * (n / 4) + VOC_THREADS - 1) / VOC_THREADS;
  V2A_REQUIRE(blocks < ((int64_t)1 << 31), "v2a_vocos_scale_residual: rows=%lld x n=%d is more than one launch takes", (long long)rows, n);
  hipLaunchKernelGGL(vocos_pointwise_kernel<1>, dim3((unsigned)blocks), dim3(VOC_THREADS), 0, (hipStream_t)stream, p, ldp, gamma, resid, ldr, out, ldo, rows,
                     n / 4);
  return v2a_check_launch("v2a_vocos_scale_residual");
}

extern "C" int v2a_vocos_spectrum(const float* logits, int64_t ld_logits, int64_t rows, int32_t n_fft, float* spec, int64_t ld_spec, v2a_stream_t stream) {
  V2A_REQUIRE(logits && spec && logits != spec, "v2a_vocos_spectrum: null / aliased pointer");
  V2A_REQUIRE(n_fft >= 4 && n_fft % 4 == 0 && n_fft <= V2A_VOCOS_MAX_FFT, "v2a_vocos_spectrum: n_fft=%d (a multiple of 4, 4 .. %d)", n_fft, V2A_VOCOS_MAX_FFT);
  V2A_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31) && ld_logits >= n_fft + 2 && ld_spec >= n_fft + 2 && ld_spec % 2 == 0,
              "v2a_vocos_spectrum: rows=%lld ld_logits=%lld ld_spec=%lld (1 <= rows < 2^31, rows of n_fft + 2 = %d logits, ld_spec even and >= n_fft + 2)",
              (long long)rows, (long long)ld_logits, (long long)ld_spec, n_fft + 2);
  V2A_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)spec & 7) == 0, "v2a_vocos_spectrum: alignment (8 bytes for spec)");
  const int32_t kpairs = (int32_t)(ld_spec / 2);
  const int64_t blocks = (rows * kpairs + VOC_THREADS - 1) / VOC_THREADS;
  V2A_REQUIRE(blocks < ((int64_t)1 << 31), "v2a_vocos_spectrum: rows=%lld x ld_spec=%lld is more than one launch takes", (long long)rows, (long long)ld_spec);
  hipLaunchKernelGGL(vocos_spectrum_kernel, dim3((unsigned)blocks), dim3(VOC_THREADS), 0, (hipStream_t)stream, logits, ld_logits, rows, n_fft / 2 + 1, spec,
                     ld_spec, kpairs);
  return v2a_check_launch("v2a_vocos_spectrum");
}

extern "C" int v2a_vocos_overlap_add(const float* frames, int64_t ld_frames, int64_t rows_per_clip, const float* wsq, int32_t B, int32_t T, int32_t n_fft,
                                     int32_t hop, const int32_t* lens, float* out, int64_t out_batch_stride, v2a_stream_t stream) {
  V2A_REQUIRE(frames && wsq && out && frames != out, "v2a_vocos_overlap_add: null / aliased pointer");
  V2A_REQUIRE(n_fft >= 4 && n_fft % 4 == 0 && n_fft <= V2A_VOCOS_MAX_FFT && hop >= 1 && hop <= n_fft,
              "v2a_vocos_overlap_add: n_fft=%d hop=%d (n_fft a multiple of 4, 4 .. %d; 1 <= hop <= n_fft)", n_fft, hop, V2A_VOCOS_MAX_FFT);
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 2 && T <= V2A_VOCOS_MAX_FRAMES && rows_per_clip >= T && ld_frames >= n_fft,
              "v2a_vocos_overlap_add: B=%d T=%d rows_per_clip=%lld ld_frames=%lld (1 <= B <= 65535, 2 <= T <= %d, rows_per_clip >= T, ld_frames >= n_fft)",
              B, T, (long long)rows_per_clip, (long long)ld_frames, V2A_VOCOS_MAX_FRAMES);
  const int64_t n_out = (int64_t)(T - 1) * hop;
  V2A_REQUIRE(out_batch_stride >= n_out, "v2a_vocos_overlap_add: out_batch_stride=%lld < (T - 1) hop = %lld", (long long)out_batch_stride, (long long)n_out);
  V2A_REQUIRE((((uintptr_t)frames | (uintptr_t)wsq | (uintptr_t)out) & 3) == 0 && (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vocos_overlap_add: alignment");
  const dim3 grid((unsigned)((n_out + VOC_THREADS - 1) / VOC_THREADS), (unsigned)B);
  hipLaunchKernelGGL(vocos_overlap_add_kernel, grid, dim3(VOC_THREADS), 0, (hipStream_t)stream, frames, ld_frames, rows_per_clip, wsq, T, n_fft, hop, lens,
                     out, out_batch_stride);
  return v2a_check_launch("v2a_vocos_overlap_add");
}
