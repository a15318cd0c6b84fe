// The HiFi-GAN generator (AudioLDM's 16 kHz / 64-mel vocoder): mel frames -> wave, the second half of `VaeWrapper.decode`
// (x3:470-490; `decode_to_waveform` -> `vocoder_infer`, src/audioldm/hifigan/utilities.py:76-86, around `Generator.forward`,
// src/audioldm/hifigan/models.py:163-180).
//
// Activations are time-major fp32 rows of C floats; frame t of clip b is row b * rows_per_clip + t.  The wide stages (C >= 256), and
// every stage under fused=False, are exact-fp32 v2a_gemm launches over overlapping rows of an operand buffer (hifigan.py); three kernels
// stand around them:
//   * act_pad: (s0 + s1) + s2, divided (the MRF mean), leaky ReLU, written into an operand buffer whose every clip has `halo` zero rows in
//              front and zero rows behind its own length -- the zero padding of every convolution, per clip of a ragged batch.
//   * post:    conv_post (C -> 1, k = 7) as one fmaf chain per sample from the bias, tap then channel, then tanh; fp32 wave and / or the
//              truncating int16 of wave * 32768, saturated.  A block stages its samples + 6 rows in LDS (row pitch C + 1: a lane per
//              sample walks its rows without bank conflicts).
//   * conv:    the direct dilated Conv1d of the narrow stages (C = 32, 64, 128) on v_mfma_f32_16x16x4_f32.  A workgroup of four waves owns
//              V2A_HIFIGAN_TILE = 128 frames of one clip and all C outputs.  It stages 128 + (k - 1) d input rows in LDS once, leaky ReLU
//              applied, rows outside [0, len) zero by predicate (no padded buffer, no activation pass); every tap reads that tile at its own
//              row offset.  The MFMA's A operand is the weight (rows = output channels), its B operand the input (columns = frames), so a
//              lane ends with four consecutive output channels of one frame: 16-byte bias / residual loads and stores.  Weights come packed in
//              fragment order by the host (hifigan.py `pack_conv_fragments`): one 16-byte load per lane gives four k steps of a 16-channel
//              output tile, 1 KB per wave and coalesced.  LDS rows have a pitch of C + 4 floats: the 16 frames x 4 channels a wave reads per
//              k step fall in 64 distinct banks.
//              Order of the sum of one output: per tap one MFMA chain from zero over the input channels in ascending order (the k slots of
//              an MFMA are added in ascending order too), the taps' sums added in ascending tap order, then the bias, then the residual.
//              It depends on (k, C) alone, never on the tile, the clip's place in the batch or the other clips.
// No atomics anywhere.
#include "v2a_common.h"

#include <math.h>

namespace {

constexpr int HG_THREADS = 256;
constexpr int HG_TILE = V2A_HIFIGAN_TILE;
constexpr size_t HG_LDS_MAX = 160 * 1024;
constexpr int HG_POST_TAPS = 7, HG_POST_HALO = 3;

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : __fmul_rn(v, slope); }

__device__ __forceinline__ int clip_len(const int32_t* lens, int clip, int T) {
  int len = lens ? lens[clip] : T;
  return len < 0 ? 0 : (len > T ? T : len);
}

struct ActPadParams {
  const float *s0, *s1, *s2;
  const int32_t* lens;
  float* out;
  int64_t src_pitch, lds, out_pitch;
  int32_t T, C4, halo;
  float div, slope;
};

__global__ __launch_bounds__(HG_THREADS) void hifigan_act_pad_kernel(ActPadParams P) {
  const int clip = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * HG_THREADS + threadIdx.x;
  if (i >= P.out_pitch * P.C4) return;
  const int64_t r = i / P.C4;
  const int c = (int)(i - r * P.C4) << 2;
  const int64_t t = r - P.halo;
  const int len = clip_len(P.lens, clip, P.T);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t >= 0 && t < len) {
    const int64_t off = ((int64_t)clip * P.src_pitch + t) * P.lds + c;
    v = *reinterpret_cast<const f32x4*>(P.s0 + off);
    if (P.s1) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(P.s1 + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], b[e]);
    }
    if (P.s2) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(P.s2 + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], b[e]);
    }
    if (P.div != 1.0f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fdiv_rn(v[e], P.div);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = leaky(v[e], P.slope);
  }
  *reinterpret_cast<f32x4*>(P.out + ((int64_t)clip * P.out_pitch + r) * (P.C4 << 2) + c) = v;
}

struct PostParams {
  const float *a, *w, *bias;
  const int32_t* lens;
  float *wave, *pre;
  int16_t* pcm;
  int64_t pitch, obs;
  int32_t T, C, ts;
};

__global__ __launch_bounds__(HG_THREADS) void hifigan_post_kernel(PostParams P) {
  extern __shared__ __attribute__((aligned(16))) float xs[];          // [ts + 6][C + 1]: frames t0 - 3 .. t0 + ts + 2, zero outside [0, len)
  const int clip = blockIdx.y, t0 = blockIdx.x * P.ts, C = P.C, LD = C + 1;
  const int len = clip_len(P.lens, clip, P.T);
  if (t0 >= len) return;
  const float* base = P.a + (int64_t)clip * P.pitch * C;
  for (int i = threadIdx.x; i < (P.ts + 2 * HG_POST_HALO) * C; i += HG_THREADS) {
    const int r = i / C, c = i - r * C, t = t0 + r - HG_POST_HALO;
    xs[r * LD + c] = (t >= 0 && t < len) ? base[(int64_t)t * C + c] : 0.0f;
  }
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if ((int)threadIdx.x >= P.ts || t >= len) return;
  float acc = P.bias[0];
  for (int j = 0; j < HG_POST_TAPS; ++j) {
    const float* xr = xs + (threadIdx.x + j) * LD;
    const float* wr = P.w + j * C;
    for (int c = 0; c < C; ++c) acc = __fmaf_rn(wr[c], xr[c], acc);
  }
  const float y = tanhf(acc);
  const int64_t o = (int64_t)clip * P.obs + t;
  if (P.pre) P.pre[o] = acc;
  if (P.wave) P.wave[o] = y;
  if (P.pcm) {
    float q = truncf(__fmul_rn(y, 32768.0f));                          // numpy's astype("int16") truncates; +-32768 saturates
    q = q > 32767.0f ? 32767.0f : (q < -32768.0f ? -32768.0f : q);
    P.pcm[o] = (int16_t)(int)q;
  }
}

struct ConvParams {
  const float *x, *wp, *bias, *resid;
  const int32_t* lens;
  float* out;
  int64_t ldx, ldr, ldo, pitch;
  int32_t T, k, d;
  float slope;
};

template <int NT>        // C = 16 NT output (and input) channels
__global__ __launch_bounds__(HG_THREADS) void hifigan_conv_kernel(ConvParams P) {
  extern __shared__ __attribute__((aligned(16))) float xs[];          // [HG_TILE + (k - 1) d][C + 4]
  constexpr int C = 16 * NT, C4 = C / 4, LD = C + 4;
  const int clip = blockIdx.y, t0 = blockIdx.x * HG_TILE;
  const int len = clip_len(P.lens, clip, P.T);
  if (t0 >= len) return;                                             // the whole workgroup: nothing of this tile is inside the clip
  const int span = (P.k - 1) * P.d, pad = span / 2, rows = HG_TILE + span;
  const int64_t row0 = (int64_t)clip * P.pitch;
  for (int i = threadIdx.x; i < rows * C4; i += HG_THREADS) {
    const int r = i / C4, c = (i - r * C4) << 2, t = t0 - pad + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < len) {
      v = *reinterpret_cast<const f32x4*>(P.x + (row0 + t) * P.ldx + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = leaky(v[e], P.slope);
    }
    *reinterpret_cast<f32x4*>(xs + r * LD + c) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, m16 = lane & 15;
  f32x4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* wp = reinterpret_cast<const f32x4*>(P.wp) + lane;
  for (int j = 0; j < P.k; ++j) {
    f32x4 part[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) part[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xr = xs + (wave * 32 + m16 + j * P.d) * LD + g;     // frame (wave, m16) of the first half tile at tap j, channel g
    const f32x4* wj = wp + (int64_t)j * NT * NT * 64;
#pragma unroll
    for (int kq = 0; kq < NT; ++kq) {
      f32x4 a[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) a[n] = wj[(kq * NT + n) * 64];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float b0 = xr[16 * kq + 4 * e], b1 = xr[16 * LD + 16 * kq + 4 * e];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          part[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[n][e], b0, part[0][n], 0, 0, 0);
          part[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[n][e], b1, part[1][n], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m][n][e] = __fadd_rn(acc[m][n][e], part[m][n][e]);
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int t = t0 + wave * 32 + m * 16 + m16;
    if (t >= len) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int co = 16 * n + 4 * g;                                  // D rows 4 g .. 4 g + 3 of output tile n, column = frame m16
      const f32x4 b = *reinterpret_cast<const f32x4*>(P.bias + co);
      f32x4 v = acc[m][n];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], b[e]);
      if (P.resid) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(P.resid + (row0 + t) * P.ldr + co);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], r[e]);
      }
      *reinterpret_cast<f32x4*>(P.out + (row0 + t) * P.ldo + co) = v;
    }
  }
}

template <int NT>
int launch_conv(const ConvParams& P, int32_t B, size_t lds, hipStream_t stream) {
  static std::atomic<uint64_t> done{0};
  const int rc = v2a_enable_lds((const void*)hifigan_conv_kernel<NT>, HG_LDS_MAX, done, "v2a_hifigan_conv");
  if (rc != V2A_OK) return rc;
  const dim3 grid((unsigned)((P.T + HG_TILE - 1) / HG_TILE), (unsigned)B);
  hipLaunchKernelGGL(hifigan_conv_kernel<NT>, grid, dim3(HG_THREADS), lds, stream, P);
  return v2a_check_launch("v2a_hifigan_conv");
}

}  // namespace

extern "C" int v2a_hifigan_act_pad(const float* s0, const float* s1, const float* s2, int64_t src_rows_per_clip, int64_t ld_src, int32_t B, int32_t T,
                                   int32_t C, const int32_t* lens, float divisor, float slope, float* out, int64_t out_rows_per_clip, int32_t halo,
                                   v2a_stream_t stream) {
  V2A_REQUIRE(s0 && out && (s1 || !s2) && out != s0 && out != s1 && out != s2, "v2a_hifigan_act_pad: null / aliased pointer (sources fill s0, s1, s2 in order)");
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= V2A_HIFIGAN_MAX_ROWS && C >= 4 && C % 4 == 0 && C <= 65536 && halo >= 0 && halo <= (1 << 20),
              "v2a_hifigan_act_pad: B=%d T=%d C=%d halo=%d (1 <= B <= 65535, 1 <= T <= %d, C a multiple of 4 up to 65536, 0 <= halo <= 2^20)", B, T, C, halo,
              V2A_HIFIGAN_MAX_ROWS);
  V2A_REQUIRE(src_rows_per_clip >= T && ld_src >= C && ld_src % 4 == 0 && out_rows_per_clip >= (int64_t)T + 2 * (int64_t)halo &&
                  out_rows_per_clip <= V2A_HIFIGAN_MAX_ROWS,
              "v2a_hifigan_act_pad: src_rows_per_clip=%lld ld_src=%lld out_rows_per_clip=%lld (source clips of T rows of C floats, row stride a multiple "
              "of 4; T + 2 halo <= out_rows_per_clip <= %d)", (long long)src_rows_per_clip, (long long)ld_src, (long long)out_rows_per_clip, V2A_HIFIGAN_MAX_ROWS);
  V2A_REQUIRE(divisor > 0.0f && slope == slope, "v2a_hifigan_act_pad: divisor=%g slope=%g", (double)divisor, (double)slope);
  V2A_REQUIRE((((uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)out) & 15) == 0 && (!lens || ((uintptr_t)lens & 3) == 0),
              "v2a_hifigan_act_pad: alignment (16 bytes)");
  ActPadParams P;
  P.s0 = s0, P.s1 = s1, P.s2 = s2, P.lens = lens, P.out = out;
  P.src_pitch = src_rows_per_clip, P.lds = ld_src, P.out_pitch = out_rows_per_clip;
  P.T = T, P.C4 = C / 4, P.halo = halo, P.div = divisor, P.slope = slope;
  const int64_t blocks = (out_rows_per_clip * P.C4 + HG_THREADS - 1) / HG_THREADS;
  V2A_REQUIRE(blocks < ((int64_t)1 << 31), "v2a_hifigan_act_pad: %lld rows x C=%d is more than one launch takes", (long long)out_rows_per_clip, C);
  hipLaunchKernelGGL(hifigan_act_pad_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(HG_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_hifigan_act_pad");
}

extern "C" int v2a_hifigan_post(const float* a, int64_t rows_per_clip, int32_t B, int32_t T, int32_t C, const int32_t* lens, const float* w,
                                const float* bias, float* wave, int16_t* pcm, float* pre, int64_t out_batch_stride, v2a_stream_t stream) {
  V2A_REQUIRE(a && w && bias && (wave || pcm), "v2a_hifigan_post: null pointer (one of wave and pcm is required)");
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= V2A_HIFIGAN_MAX_ROWS && C >= 1 && C <= V2A_HIFIGAN_POST_MAX_C && rows_per_clip >= T &&
                  out_batch_stride >= T,
              "v2a_hifigan_post: B=%d T=%d C=%d rows_per_clip=%lld out_batch_stride=%lld (1 <= B <= 65535, 1 <= T <= %d, 1 <= C <= %d, both pitches >= T)",
              B, T, C, (long long)rows_per_clip, (long long)out_batch_stride, V2A_HIFIGAN_MAX_ROWS, V2A_HIFIGAN_POST_MAX_C);
  V2A_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)wave | (uintptr_t)pre) & 3) == 0 && ((uintptr_t)pcm & 1) == 0 &&
                  (!lens || ((uintptr_t)lens & 3) == 0), "v2a_hifigan_post: alignment");
  PostParams P;
  P.a = a, P.w = w, P.bias = bias, P.lens = lens, P.wave = wave, P.pre = pre, P.pcm = pcm;
  P.pitch = rows_per_clip, P.obs = out_batch_stride, P.T = T, P.C = C;
  int ts = HG_THREADS;                                               // samples of a block: the largest power of two whose rows fit 64 KB
  while ((size_t)(ts + 2 * HG_POST_HALO) * (C + 1) * sizeof(float) > 64 * 1024) ts >>= 1;
  P.ts = ts;
  const size_t lds = (size_t)(ts + 2 * HG_POST_HALO) * (C + 1) * sizeof(float);
  hipLaunchKernelGGL(hifigan_post_kernel, dim3((unsigned)((T + ts - 1) / ts), (unsigned)B), dim3(HG_THREADS), lds, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_hifigan_post");
}

extern "C" int v2a_hifigan_conv(const float* x, int64_t ldx, int64_t rows_per_clip, int32_t B, int32_t T, int32_t C, const int32_t* lens,
                                const float* wp, const float* bias, int32_t k, int32_t d, float slope, const float* resid, int64_t ldr, float* out,
                                int64_t ldo, v2a_stream_t stream) {
  V2A_REQUIRE(x && wp && bias && out && out != x, "v2a_hifigan_conv: null / aliased pointer (out may be resid, not x)");
  V2A_REQUIRE(C == 32 || C == 64 || C == 128, "v2a_hifigan_conv: C=%d (32, 64 or 128: wider stages run as v2a_gemm)", C);
  V2A_REQUIRE(k >= 1 && k % 2 == 1 && d >= 1 && (int64_t)(k - 1) * d <= 4096, "v2a_hifigan_conv: k=%d d=%d (k odd, (k - 1) d <= 4096)", k, d);
  const size_t lds = (size_t)(HG_TILE + (k - 1) * d) * (C + 4) * sizeof(float);
  V2A_REQUIRE(lds <= HG_LDS_MAX, "v2a_hifigan_conv: C=%d k=%d d=%d needs %zu bytes of LDS for a tile of %d frames, more than %zu", C, k, d, lds, HG_TILE,
              HG_LDS_MAX);
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= V2A_HIFIGAN_MAX_ROWS && rows_per_clip >= T && rows_per_clip <= V2A_HIFIGAN_MAX_ROWS && ldx >= C &&
                  ldo >= C && ldx % 4 == 0 && ldo % 4 == 0 && (!resid || (ldr >= C && ldr % 4 == 0)),
              "v2a_hifigan_conv: B=%d T=%d rows_per_clip=%lld ldx=%lld ldo=%lld ldr=%lld (1 <= B <= 65535, 1 <= T <= rows_per_clip <= %d, row strides >= C "
              "and multiples of 4)", B, T, (long long)rows_per_clip, (long long)ldx, (long long)ldo, (long long)ldr, V2A_HIFIGAN_MAX_ROWS);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)wp | (uintptr_t)bias | (uintptr_t)resid | (uintptr_t)out) & 15) == 0 && (!lens || ((uintptr_t)lens & 3) == 0),
              "v2a_hifigan_conv: alignment (16 bytes)");
  ConvParams P;
  P.x = x, P.wp = wp, P.bias = bias, P.resid = resid, P.lens = lens, P.out = out;
  P.ldx = ldx, P.ldr = ldr, P.ldo = ldo, P.pitch = rows_per_clip;
  P.T = T, P.k = k, P.d = d, P.slope = slope;
  if (C == 32) return launch_conv<2>(P, B, lds, (hipStream_t)stream);
  if (C == 64) return launch_conv<4>(P, B, lds, (hipStream_t)stream);
  return launch_conv<8>(P, B, lds, (hipStream_t)stream);
}
