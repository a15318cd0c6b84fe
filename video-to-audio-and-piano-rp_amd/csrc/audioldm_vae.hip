// The AudioLDM VAE decoder (`AutoencoderKL.decode` behind `decode_first_stage`): latents -> 64-bin mel image, the first half of
// `VaeWrapper.decode` (x3:470-490); the second half is csrc/hifigan.hip.  The network is `Decoder` of
// src/audioldm/variational_autoencoder/modules.py:546-683 behind `post_quant_conv` (autoencoder.py).
//
// Activations are channels-last fp32 maps: time on H, the frequency bins on W, C floats per pixel.  Two row layouts of one geometry
// (Wp = W + 2, rows_per_clip >= (H + 2) Wp), pixel (y, x) of clip b:
//   * bordered: row b * rows_per_clip + (y + 1) Wp + (x + 1); a one-pixel zero border around the clip's own len x W pixels and zero
//               rows behind them -- the operand of a 3x3 convolution (audioldm_vae.py runs it as the exact-fp32 v2a_gemm with one A
//               segment per kernel row over the flat padded grid) and, from its interior on, of a 1x1 one;
//   * flat:     row b * rows_per_clip + y * Wp + x: what such a GEMM writes, one output row per padded position.  Rows with x >= W or
//               y >= len hold values no kernel here reads.
// Every kernel takes the source's row pitch (src_wp), so a dense map (pitch W) is a flat one.  `lens` clamps to 0 .. H as in hifigan.hip.
//   * stage_in:     VaeWrapper's reshape + post_quant_conv (1x1, 1 / scale_factor folded in by the host) -> bordered map, channels padded.
//   * gn_stats:     per (clip, tile of GN_TILE pixels counted from the clip's first pixel, group): sum and sum of squares in double.
//   * gn_act_pad:   the tiles' partials added in ascending order, mean and rstd in double rounded once, the affine map and the swish in
//                   fp32 -> bordered map, or dense rows (border 0) for the attention.
//   * upsample_pad: nearest x2 on both axes, flat -> bordered, bit copies.
//   * softmax:      rows of the attention's score matrix, in place, max-subtracted, columns n .. ld zeroed.
//   * conv_out:     3x3 C -> 1 over an activated bordered map, one fmaf chain per pixel -> mel (b, T, W).
// No atomics anywhere; every sum has one fixed order that does not depend on the batch.
#include "v2a_common.h"

#include <math.h>

namespace {

constexpr int VAE_THREADS = 256;
constexpr int GN_TILE = V2A_VAE_GN_TILE;       // pixels of a workgroup of gn_stats
constexpr int GN_GROUPS = V2A_VAE_GROUPS;      // 32
constexpr int GN_SUB = VAE_THREADS / GN_GROUPS;    // 8 pixel lanes per group
constexpr int ACT_ITERS = 8;                   // float4s per thread of gn_act_pad / upsample_pad

__device__ __forceinline__ int vae_len(const int32_t* lens, int clip, int H) {
  int len = lens ? lens[clip] : H;
  return len < 0 ? 0 : (len > H ? H : len);
}

struct StageInParams {
  const float *src, *w, *bias;
  const int32_t* lens;
  float* out;
  int64_t sb, sc, st, sw, out_pitch;
  int32_t H, W, zc, cpad;
};

__global__ __launch_bounds__(VAE_THREADS) void vae_stage_in_kernel(StageInParams P) {
  const int clip = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x;
  if (r >= P.out_pitch) return;
  const int Wp = P.W + 2;
  const int64_t yy = r / Wp - 1;
  const int xx = (int)(r % Wp) - 1;
  const int len = vae_len(P.lens, clip, P.H);
  float* o = P.out + ((int64_t)clip * P.out_pitch + r) * P.cpad;
  if (yy < 0 || yy >= len || xx < 0 || xx >= P.W) {
    for (int c = 0; c < P.cpad; ++c) o[c] = 0.0f;
    return;
  }
  const float* s = P.src + (int64_t)clip * P.sb + yy * P.st + (int64_t)xx * P.sw;
  for (int co = 0; co < P.zc; ++co) {
    float acc = P.bias[co];
    for (int ci = 0; ci < P.zc; ++ci) acc = __fmaf_rn(P.w[co * P.zc + ci], s[(int64_t)ci * P.sc], acc);
    o[co] = acc;
  }
  for (int c = P.zc; c < P.cpad; ++c) o[c] = 0.0f;
}

struct GnStatsParams {
  const float* x;
  const int32_t* lens;
  double* part;
  int64_t src_pitch;
  int32_t H, W, C, src_wp, tiles;
};

// Thread (sub, group) = (tid / 32, tid % 32): pixels sub, sub + 8, ... of the tile, the group's C / 32 channels in ascending order, one
// double chain each for the sum and the sum of squares; the 8 chains of a group are then added in ascending sub by one thread.
__global__ __launch_bounds__(VAE_THREADS) void vae_gn_stats_kernel(GnStatsParams P) {
  __shared__ double red[GN_SUB][GN_GROUPS][2];
  const int clip = blockIdx.y, tile = blockIdx.x;
  const int g = threadIdx.x & (GN_GROUPS - 1), sub = threadIdx.x / GN_GROUPS;
  const int cpg = P.C / GN_GROUPS;
  const int64_t npix = (int64_t)vae_len(P.lens, clip, P.H) * P.W;
  const int64_t p0 = (int64_t)tile * GN_TILE;
  const int64_t p1 = p0 + GN_TILE < npix ? p0 + GN_TILE : npix;
  double s = 0.0, ss = 0.0;
  const float* base = P.x + (int64_t)clip * P.src_pitch * P.C + g * cpg;
  for (int64_t p = p0 + sub; p < p1; p += GN_SUB) {
    const int64_t y = p / P.W;
    const int x = (int)(p - y * P.W);
    const float* px = base + (y * P.src_wp + x) * P.C;
    for (int c = 0; c < cpg; ++c) {
      const double v = (double)px[c];
      s += v;
      ss = fma(v, v, ss);
    }
  }
  red[sub][g][0] = s;
  red[sub][g][1] = ss;
  __syncthreads();
  if (threadIdx.x < GN_GROUPS) {
    double a = red[0][g][0], b = red[0][g][1];
#pragma unroll
    for (int k = 1; k < GN_SUB; ++k) {
      a += red[k][g][0];
      b += red[k][g][1];
    }
    double* o = P.part + (((int64_t)clip * P.tiles + tile) * GN_GROUPS + g) * 2;
    o[0] = a;
    o[1] = b;
  }
}

struct GnActParams {
  const float *x, *gamma, *beta;
  const double* part;
  const int32_t* lens;
  float* out;
  int64_t src_pitch, out_pitch;
  int32_t H, W, C4, src_wp, tiles, border, swish;
  double eps;
};

__global__ __launch_bounds__(VAE_THREADS) void vae_gn_act_pad_kernel(GnActParams P) {
  __shared__ float stat[GN_GROUPS][2];
  const int clip = blockIdx.y;
  const int len = vae_len(P.lens, clip, P.H);
  const int C = P.C4 << 2, cpg = C / GN_GROUPS;
  if (threadIdx.x < GN_GROUPS) {
    const int64_t npix = (int64_t)len * P.W;
    const int nt = (int)((npix + GN_TILE - 1) / GN_TILE);
    const double* pp = P.part + ((int64_t)clip * P.tiles * GN_GROUPS + threadIdx.x) * 2;
    double s = 0.0, ss = 0.0;
    for (int t = 0; t < nt; ++t) {
      s += pp[(int64_t)t * GN_GROUPS * 2];
      ss += pp[(int64_t)t * GN_GROUPS * 2 + 1];
    }
    float mean = 0.0f, rstd = 0.0f;
    if (npix > 0) {
      const double n = (double)npix * (double)cpg;
      const double m = s / n;
      double var = ss / n - m * m;
      var = var < 0.0 ? 0.0 : var;
      mean = (float)m;
      rstd = (float)(1.0 / sqrt(var + P.eps));
    }
    stat[threadIdx.x][0] = mean;
    stat[threadIdx.x][1] = rstd;
  }
  __syncthreads();
  const int Wd = P.W + 2 * P.border;
  const int64_t total = P.out_pitch * P.C4;
#pragma unroll 1
  for (int it = 0; it < ACT_ITERS; ++it) {
    const int64_t i = ((int64_t)blockIdx.x * ACT_ITERS + it) * VAE_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / P.C4;
    const int c = (int)(i - r * P.C4) << 2;
    const int64_t yy = r / Wd - P.border;
    const int xx = (int)(r % Wd) - P.border;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (yy >= 0 && yy < len && xx >= 0 && xx < P.W) {
      v = *reinterpret_cast<const f32x4*>(P.x + ((int64_t)clip * P.src_pitch + yy * P.src_wp + xx) * C + c);
      const f32x4 ga = *reinterpret_cast<const f32x4*>(P.gamma + c), be = *reinterpret_cast<const f32x4*>(P.beta + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int g = (c + e) / cpg;
        float y = __fmul_rn(__fsub_rn(v[e], stat[g][0]), stat[g][1]);
        y = __fadd_rn(__fmul_rn(y, ga[e]), be[e]);
        v[e] = P.swish ? silu_exact_f(y) : y;
      }
    }
    *reinterpret_cast<f32x4*>(P.out + ((int64_t)clip * P.out_pitch + r) * C + c) = v;
  }
}

struct UpsampleParams {
  const float* x;
  const int32_t* lens;
  float* out;
  int64_t src_pitch, out_pitch;
  int32_t H, W, C4, src_wp;
};

__global__ __launch_bounds__(VAE_THREADS) void vae_upsample_pad_kernel(UpsampleParams P) {
  const int clip = blockIdx.y;
  const int len2 = 2 * vae_len(P.lens, clip, P.H);
  const int C = P.C4 << 2, Wd = 2 * P.W + 2;
  const int64_t total = P.out_pitch * P.C4;
#pragma unroll 1
  for (int it = 0; it < ACT_ITERS; ++it) {
    const int64_t i = ((int64_t)blockIdx.x * ACT_ITERS + it) * VAE_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / P.C4;
    const int c = (int)(i - r * P.C4) << 2;
    const int64_t yy = r / Wd - 1;
    const int xx = (int)(r % Wd) - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (yy >= 0 && yy < len2 && xx >= 0 && xx < 2 * P.W)
      v = *reinterpret_cast<const f32x4*>(P.x + ((int64_t)clip * P.src_pitch + (yy >> 1) * P.src_wp + (xx >> 1)) * C + c);
    *reinterpret_cast<f32x4*>(P.out + ((int64_t)clip * P.out_pitch + r) * C + c) = v;
  }
}

// One workgroup per row.  v = scale * s (one rounded product); the maximum; e = expf(v - max), written in place; a thread adds its
// columns tid, tid + 256, ... in ascending order, a wave adds its 64 lanes by the xor butterfly (32, 16, .. 1), the four waves' sums
// are added as (w0 + w1) + (w2 + w3); p = e / sum (IEEE division).
__global__ __launch_bounds__(VAE_THREADS) void vae_softmax_kernel(float* s, int64_t ld, int32_t n, float scale) {
  __shared__ float red[2][VAE_THREADS / 64];
  float* row = s + (int64_t)blockIdx.x * ld;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < n; j += VAE_THREADS) m = fmaxf(m, __fmul_rn(scale, row[j]));
  m = wave_max(m);
  if (lane == 0) red[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  float sum = 0.0f;
  for (int j = threadIdx.x; j < n; j += VAE_THREADS) {
    const float e = expf(__fsub_rn(__fmul_rn(scale, row[j]), m));
    row[j] = e;
    sum = __fadd_rn(sum, e);
  }
  sum = wave_sum(sum);
  if (lane == 0) red[1][wave] = sum;
  __syncthreads();
  sum = __fadd_rn(__fadd_rn(red[1][0], red[1][1]), __fadd_rn(red[1][2], red[1][3]));
  for (int j = threadIdx.x; j < n; j += VAE_THREADS) row[j] = __fdiv_rn(row[j], sum);
  for (int64_t j = n + threadIdx.x; j < ld; j += VAE_THREADS) row[j] = 0.0f;
}

struct ConvOutParams {
  const float *a, *w, *bias;
  const int32_t* lens;
  float* out;
  int64_t pitch;
  int32_t H, W, C;
};

__global__ __launch_bounds__(VAE_THREADS) void vae_conv_out_kernel(ConvOutParams P) {
  const int clip = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x;
  if (i >= (int64_t)P.H * P.W) return;
  const int64_t y = i / P.W;
  const int x = (int)(i - y * P.W);
  const int Wp = P.W + 2;
  float* o = P.out + (int64_t)clip * P.H * P.W + i;
  if (y >= vae_len(P.lens, clip, P.H)) {
    *o = 0.0f;
    return;
  }
  float acc = P.bias[0];
  for (int ky = 0; ky < 3; ++ky) {
    const float* ar = P.a + ((int64_t)clip * P.pitch + (y + ky) * Wp + x) * P.C;      // bordered (y + ky, x): the window's row ky, kx = 0
    const float* wr = P.w + ky * 3 * P.C;
    for (int k = 0; k < 3 * P.C; k += 4) {                                            // kx-major, then c: 3 C contiguous floats
      const f32x4 av = *reinterpret_cast<const f32x4*>(ar + k);
      acc = __fmaf_rn(wr[k], av[0], acc);
      acc = __fmaf_rn(wr[k + 1], av[1], acc);
      acc = __fmaf_rn(wr[k + 2], av[2], acc);
      acc = __fmaf_rn(wr[k + 3], av[3], acc);
    }
  }
  *o = acc;
}

inline bool geom_ok(int32_t B, int32_t H, int32_t W) { return B >= 1 && B <= 65535 && H >= 1 && H <= V2A_VAE_MAX_H && W >= 1 && W <= V2A_VAE_MAX_W; }

}  // namespace

extern "C" int v2a_vae_stage_in(const float* src, int64_t batch_stride, int64_t chan_stride, int64_t time_stride, int64_t bin_stride, int32_t B,
                                int32_t H, int32_t W, int32_t zc, const int32_t* lens, const float* w, const float* bias, float* out, int32_t c_pad,
                                int64_t out_rows_per_clip, v2a_stream_t stream) {
  V2A_REQUIRE(src && w && bias && out && out != src, "v2a_vae_stage_in: null / aliased pointer");
  V2A_REQUIRE(geom_ok(B, H, W), "v2a_vae_stage_in: B=%d H=%d W=%d (1 <= B <= 65535, 1 <= H <= %d, 1 <= W <= %d)", B, H, W, V2A_VAE_MAX_H, V2A_VAE_MAX_W);
  V2A_REQUIRE(zc >= 1 && zc <= V2A_VAE_MAX_Z && c_pad >= zc && c_pad % 16 == 0 && c_pad <= V2A_VAE_MAX_Z,
              "v2a_vae_stage_in: zc=%d c_pad=%d (1 <= zc <= c_pad <= %d, c_pad a multiple of 16)", zc, c_pad, V2A_VAE_MAX_Z);
  V2A_REQUIRE(batch_stride >= 0 && chan_stride >= 1 && time_stride >= 1 && bin_stride >= 1 && out_rows_per_clip >= (int64_t)(H + 2) * (W + 2) &&
                  out_rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_stage_in: strides %lld %lld %lld %lld out_rows_per_clip=%lld (positive strides; (H + 2)(W + 2) <= out_rows_per_clip <= %d)",
              (long long)batch_stride, (long long)chan_stride, (long long)time_stride, (long long)bin_stride, (long long)out_rows_per_clip, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((((uintptr_t)src | (uintptr_t)w | (uintptr_t)bias) & 3) == 0 && ((uintptr_t)out & 15) == 0 && (!lens || ((uintptr_t)lens & 3) == 0),
              "v2a_vae_stage_in: alignment (out 16 bytes)");
  StageInParams P;
  P.src = src, P.w = w, P.bias = bias, P.lens = lens, P.out = out;
  P.sb = batch_stride, P.sc = chan_stride, P.st = time_stride, P.sw = bin_stride, P.out_pitch = out_rows_per_clip;
  P.H = H, P.W = W, P.zc = zc, P.cpad = c_pad;
  const int64_t blocks = (out_rows_per_clip + VAE_THREADS - 1) / VAE_THREADS;
  hipLaunchKernelGGL(vae_stage_in_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(VAE_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vae_stage_in");
}

extern "C" int v2a_vae_gn_stats(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C,
                                const int32_t* lens, double* partials, int32_t tiles, v2a_stream_t stream) {
  V2A_REQUIRE(x && partials, "v2a_vae_gn_stats: null pointer");
  V2A_REQUIRE(geom_ok(B, H, W), "v2a_vae_gn_stats: B=%d H=%d W=%d (1 <= B <= 65535, 1 <= H <= %d, 1 <= W <= %d)", B, H, W, V2A_VAE_MAX_H, V2A_VAE_MAX_W);
  V2A_REQUIRE(C >= 32 && C % 32 == 0 && C <= V2A_VAE_MAX_C, "v2a_vae_gn_stats: C=%d (a multiple of 32 up to %d: 32 groups)", C, V2A_VAE_MAX_C);
  V2A_REQUIRE(src_wp >= W && src_rows_per_clip >= (int64_t)(H - 1) * src_wp + W && src_rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_gn_stats: src_wp=%d src_rows_per_clip=%lld (src_wp >= W; (H - 1) src_wp + W <= src_rows_per_clip <= %d)", src_wp,
              (long long)src_rows_per_clip, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((int64_t)tiles * V2A_VAE_GN_TILE >= (int64_t)H * W && tiles <= (1 << 24), "v2a_vae_gn_stats: tiles=%d (at least ceil(H W / %d))", tiles,
              V2A_VAE_GN_TILE);
  V2A_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)partials & 7) == 0 && (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vae_gn_stats: alignment");
  GnStatsParams P;
  P.x = x, P.lens = lens, P.part = partials, P.src_pitch = src_rows_per_clip;
  P.H = H, P.W = W, P.C = C, P.src_wp = src_wp, P.tiles = tiles;
  hipLaunchKernelGGL(vae_gn_stats_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(VAE_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vae_gn_stats");
}

extern "C" int v2a_vae_gn_act_pad(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C,
                                  const int32_t* lens, const double* partials, int32_t tiles, const float* gamma, const float* beta, double eps,
                                  int32_t swish, float* out, int64_t out_rows_per_clip, int32_t border, v2a_stream_t stream) {
  V2A_REQUIRE(x && partials && gamma && beta && out && out != x, "v2a_vae_gn_act_pad: null / aliased pointer");
  V2A_REQUIRE(geom_ok(B, H, W), "v2a_vae_gn_act_pad: B=%d H=%d W=%d (1 <= B <= 65535, 1 <= H <= %d, 1 <= W <= %d)", B, H, W, V2A_VAE_MAX_H, V2A_VAE_MAX_W);
  V2A_REQUIRE(C >= 32 && C % 32 == 0 && C <= V2A_VAE_MAX_C, "v2a_vae_gn_act_pad: C=%d (a multiple of 32 up to %d: 32 groups)", C, V2A_VAE_MAX_C);
  V2A_REQUIRE(src_wp >= W && src_rows_per_clip >= (int64_t)(H - 1) * src_wp + W && src_rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_gn_act_pad: src_wp=%d src_rows_per_clip=%lld (src_wp >= W; (H - 1) src_wp + W <= src_rows_per_clip <= %d)", src_wp,
              (long long)src_rows_per_clip, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((border == 0 || border == 1) && (swish == 0 || swish == 1) && eps > 0.0, "v2a_vae_gn_act_pad: border=%d swish=%d eps=%g", border, swish, eps);
  V2A_REQUIRE(out_rows_per_clip >= (int64_t)(H + 2 * border) * (W + 2 * border) && out_rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_gn_act_pad: out_rows_per_clip=%lld ((H + 2 border)(W + 2 border) <= out_rows_per_clip <= %d)", (long long)out_rows_per_clip,
              V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((int64_t)tiles * V2A_VAE_GN_TILE >= (int64_t)H * W && tiles <= (1 << 24), "v2a_vae_gn_act_pad: tiles=%d (at least ceil(H W / %d))", tiles,
              V2A_VAE_GN_TILE);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0 && ((uintptr_t)partials & 7) == 0 &&
                  (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vae_gn_act_pad: alignment (16 bytes)");
  GnActParams P;
  P.x = x, P.gamma = gamma, P.beta = beta, P.part = partials, P.lens = lens, P.out = out;
  P.src_pitch = src_rows_per_clip, P.out_pitch = out_rows_per_clip;
  P.H = H, P.W = W, P.C4 = C / 4, P.src_wp = src_wp, P.tiles = tiles, P.border = border, P.swish = swish, P.eps = eps;
  const int64_t per_block = (int64_t)VAE_THREADS * ACT_ITERS;
  const int64_t blocks = (out_rows_per_clip * P.C4 + per_block - 1) / per_block;
  hipLaunchKernelGGL(vae_gn_act_pad_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(VAE_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vae_gn_act_pad");
}

extern "C" int v2a_vae_upsample_pad(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C,
                                    const int32_t* lens, float* out, int64_t out_rows_per_clip, v2a_stream_t stream) {
  V2A_REQUIRE(x && out && out != x, "v2a_vae_upsample_pad: null / aliased pointer");
  V2A_REQUIRE(geom_ok(B, H, W) && 2 * (int64_t)H <= V2A_VAE_MAX_H && 2 * W <= V2A_VAE_MAX_W,
              "v2a_vae_upsample_pad: B=%d H=%d W=%d (1 <= B <= 65535, 1 <= 2 H <= %d, 1 <= 2 W <= %d)", B, H, W, V2A_VAE_MAX_H, V2A_VAE_MAX_W);
  V2A_REQUIRE(C >= 4 && C % 4 == 0 && C <= V2A_VAE_MAX_C, "v2a_vae_upsample_pad: C=%d (a multiple of 4 up to %d)", C, V2A_VAE_MAX_C);
  V2A_REQUIRE(src_wp >= W && src_rows_per_clip >= (int64_t)(H - 1) * src_wp + W && src_rows_per_clip <= V2A_VAE_MAX_ROWS &&
                  out_rows_per_clip >= (int64_t)(2 * H + 2) * (2 * W + 2) && out_rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_upsample_pad: src_wp=%d src_rows_per_clip=%lld out_rows_per_clip=%lld (src_wp >= W; (H - 1) src_wp + W <= src_rows_per_clip; "
              "(2 H + 2)(2 W + 2) <= out_rows_per_clip; both <= %d)", src_wp, (long long)src_rows_per_clip, (long long)out_rows_per_clip, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0 && (!lens || ((uintptr_t)lens & 3) == 0), "v2a_vae_upsample_pad: alignment (16 bytes)");
  UpsampleParams P;
  P.x = x, P.lens = lens, P.out = out, P.src_pitch = src_rows_per_clip, P.out_pitch = out_rows_per_clip;
  P.H = H, P.W = W, P.C4 = C / 4, P.src_wp = src_wp;
  const int64_t per_block = (int64_t)VAE_THREADS * ACT_ITERS;
  const int64_t blocks = (out_rows_per_clip * P.C4 + per_block - 1) / per_block;
  hipLaunchKernelGGL(vae_upsample_pad_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(VAE_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vae_upsample_pad");
}

extern "C" int v2a_vae_softmax(float* s, int64_t ld, int32_t rows, int32_t n, float scale, v2a_stream_t stream) {
  V2A_REQUIRE(s && ((uintptr_t)s & 3) == 0, "v2a_vae_softmax: null / misaligned pointer");
  V2A_REQUIRE(rows >= 1 && rows <= V2A_VAE_MAX_ROWS && n >= 1 && n <= V2A_VAE_MAX_ROWS && ld >= n && ld <= V2A_VAE_MAX_ROWS,
              "v2a_vae_softmax: rows=%d n=%d ld=%lld (1 <= rows, 1 <= n <= ld, all <= %d)", rows, n, (long long)ld, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE(scale == scale && scale > 0.0f && scale <= 3.0e38f, "v2a_vae_softmax: scale=%g (positive and finite)", (double)scale);
  hipLaunchKernelGGL(vae_softmax_kernel, dim3((unsigned)rows), dim3(VAE_THREADS), 0, (hipStream_t)stream, s, ld, n, scale);
  return v2a_check_launch("v2a_vae_softmax");
}

extern "C" int v2a_vae_conv_out(const float* a, int64_t rows_per_clip, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* lens, const float* w,
                                const float* bias, float* out, v2a_stream_t stream) {
  V2A_REQUIRE(a && w && bias && out && out != a, "v2a_vae_conv_out: null / aliased pointer");
  V2A_REQUIRE(geom_ok(B, H, W), "v2a_vae_conv_out: B=%d H=%d W=%d (1 <= B <= 65535, 1 <= H <= %d, 1 <= W <= %d)", B, H, W, V2A_VAE_MAX_H, V2A_VAE_MAX_W);
  V2A_REQUIRE(C >= 4 && C % 4 == 0 && C <= V2A_VAE_MAX_C, "v2a_vae_conv_out: C=%d (a multiple of 4 up to %d)", C, V2A_VAE_MAX_C);
  V2A_REQUIRE(rows_per_clip >= (int64_t)(H + 2) * (W + 2) && rows_per_clip <= V2A_VAE_MAX_ROWS,
              "v2a_vae_conv_out: rows_per_clip=%lld ((H + 2)(W + 2) <= rows_per_clip <= %d)", (long long)rows_per_clip, V2A_VAE_MAX_ROWS);
  V2A_REQUIRE((((uintptr_t)a) & 15) == 0 && (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 3) == 0 && (!lens || ((uintptr_t)lens & 3) == 0),
              "v2a_vae_conv_out: alignment (a 16 bytes)");
  ConvOutParams P;
  P.a = a, P.w = w, P.bias = bias, P.lens = lens, P.out = out, P.pitch = rows_per_clip, P.H = H, P.W = W, P.C = C;
  const int64_t blocks = ((int64_t)H * W + VAE_THREADS - 1) / VAE_THREADS;
  hipLaunchKernelGGL(vae_conv_out_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(VAE_THREADS), 0, (hipStream_t)stream, P);
  return v2a_check_launch("v2a_vae_conv_out");
}
