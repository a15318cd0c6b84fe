// CLIP ConvNeXt image encoder kernels for gfx950 (open_clip's TimmModel around timm's ConvNeXt, the reference's
// video_encoder = "clip_convnext", x3:1429-1431, 1716-1720, 1739-1741):
//   v2a_convnext_dwconv    7x7 depthwise convolution + bias over fp32 NHWC maps (ConvNeXtBlock.conv_dw)
//   v2a_convnext_pool_ln   mean over a frame's pixels, then LayerNorm (the head's global pool + head.norm)
// The LayerNorms are v2a_clip_layernorm, the stem / downsample convolutions and the MLP are v2a_gemm (fc1 with the GELU epilogue, fc2
// with layer scale folded in and the RESID epilogue), the downsample's patch matrix is v2a_im2col.
#include "v2a_common.h"

#include <math.h>

namespace {

// ---- depthwise 7x7 ------------------------------------------------------------------------------
// A workgroup of 256 threads computes an 8 x 8 pixel tile of 64 channels of one frame.  The 14 x 14 halo tile is staged in LDS,
// [row][column][channel], zero outside the map and past the last channel.  Thread t owns channel t & 63 and the two tile rows
// 2 (t >> 6), 2 (t >> 6) + 1: a wave reads 64 consecutive channels of one pixel (no bank conflict) and every LDS value read serves up to
// seven outputs from registers.  Each output is ONE chain acc = bias; acc = fma(w[ky][kx], x[y + ky - 3][x + kx - 3], acc) over ky, then
// kx, ascending -- a tap outside the map multiplies a zero and leaves the chain's value unchanged, so a pixel's bits depend on nothing
// but the map.
constexpr int DW_K = 7, DW_R = 3;
constexpr int DW_T = 8;                       // tile edge in pixels
constexpr int DW_HT = DW_T + 2 * DW_R;        // halo tile edge
constexpr int DW_C = 64;                      // channels per workgroup

__global__ __launch_bounds__(256) void convnext_dwconv_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ wt,
                                                              const float* __restrict__ bias, int H, int W, int C, int tiles_x) {
  __shared__ __attribute__((aligned(16))) float tile[DW_HT * DW_HT * DW_C];
  const int tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * DW_T, tx0 = (blockIdx.x % tiles_x) * DW_T;
  const int c0 = blockIdx.y * DW_C;
  const int64_t f = blockIdx.z;
  const float* xf = x + f * (int64_t)H * W * C;
  // stage: 16 threads per pixel (one float4 each), 16 pixels per pass
  for (int p = tid >> 4; p < DW_HT * DW_HT; p += 16) {
    const int y = ty0 + p / DW_HT - DW_R, xx = tx0 + p % DW_HT - DW_R;
    const int c = c0 + 4 * (tid & 15);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < H && xx >= 0 && xx < W && c < C) v = *reinterpret_cast<const f32x4*>(xf + ((int64_t)y * W + xx) * C + c);
    *reinterpret_cast<f32x4*>(&tile[p * DW_C + 4 * (tid & 15)]) = v;
  }
  const int cl = tid & 63, c = c0 + cl;
  const bool live = c < C;
  float w[DW_K * DW_K];
#pragma unroll
  for (int i = 0; i < DW_K * DW_K; ++i) w[i] = live ? wt[(int64_t)i * C + c] : 0.f;
  const float b = live ? bias[c] : 0.f;
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < 2; ++r) {
    const int oy = 2 * (tid >> 6) + r;
    float acc[DW_T];
#pragma unroll
    for (int i = 0; i < DW_T; ++i) acc[i] = b;
#pragma unroll
    for (int ky = 0; ky < DW_K; ++ky) {
      float in[DW_HT];
#pragma unroll
      for (int i = 0; i < DW_HT; ++i) in[i] = tile[((oy + ky) * DW_HT + i) * DW_C + cl];
#pragma unroll
      for (int kx = 0; kx < DW_K; ++kx) {
#pragma unroll
        for (int i = 0; i < DW_T; ++i) acc[i] = fmaf(w[ky * DW_K + kx], in[i + kx], acc[i]);
      }
    }
    const int y = ty0 + oy;
    if (live && y < H) {
      float* o = out + ((f * H + y) * (int64_t)W + tx0) * C + c;
#pragma unroll
      for (int i = 0; i < DW_T; ++i)
        if (tx0 + i < W) o[(int64_t)i * C] = acc[i];
    }
  }
}

// ---- global average pool + LayerNorm ----------------------------------------------------------------
// One workgroup per frame; thread t owns channels t, t + 256, ...: the pixel sum of a channel is one chain in ascending pixel order (a wave
// reads 64 consecutive channels of a pixel), the mean is one IEEE division, the LayerNorm over the channels is v2a_clip_layernorm's
// (mean first, then the centred sum of squares).
constexpr int PL_V = 16;                      // channels per thread: C <= 4096

__device__ __forceinline__ float block_sum256(float v, float* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void convnext_pool_ln_kernel(const float* __restrict__ x, int64_t frame_stride, int pixels, int C,
                                                               const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                               float* __restrict__ out, int64_t ldo) {
  __shared__ float part[4];
  const float* xf = x + (int64_t)blockIdx.x * frame_stride;
  float v[PL_V];
#pragma unroll
  for (int i = 0; i < PL_V; ++i) v[i] = 0.f;
  for (int p = 0; p < pixels; ++p) {
    const float* xp = xf + (int64_t)p * C;
#pragma unroll
    for (int i = 0; i < PL_V; ++i) {
      const int c = threadIdx.x + i * 256;
      if (c < C) v[i] += xp[c];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PL_V; ++i) {
    v[i] = v[i] / (float)pixels;
    s += v[i];                                // channels >= C hold 0
  }
  const float mean = block_sum256(s, part) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PL_V; ++i) {
    if (threadIdx.x + i * 256 < C) {
      const float e = v[i] - mean;
      q = fmaf(e, e, q);
    }
  }
  const float r = 1.0f / sqrtf(block_sum256(q, part) / (float)C + eps);
  float* o = out + (int64_t)blockIdx.x * ldo;
#pragma unroll
  for (int i = 0; i < PL_V; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c < C) o[c] = fmaf((v[i] - mean) * r, g[c], b[c]);
  }
}

}  // namespace

extern "C" int v2a_convnext_dwconv(const float* x, float* out, const float* wt, const float* bias, int32_t F, int32_t H, int32_t W, int32_t C,
                                   v2a_stream_t stream) {
  V2A_REQUIRE(x && out && wt && bias, "v2a_convnext_dwconv: null pointer");
  V2A_REQUIRE(x != out, "v2a_convnext_dwconv: in place (x == out) is not possible, a pixel is read by its neighbours");
  V2A_REQUIRE(F > 0 && F <= 65535 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ((uintptr_t)x & 15) == 0,
              "v2a_convnext_dwconv: F=%d (1 .. 65535) H=%d W=%d C=%d (a multiple of 4, 16-byte aligned maps)", F, H, W, C);
  const int64_t tx = (W + DW_T - 1) / DW_T, ty = (H + DW_T - 1) / DW_T;
  const int64_t cb = (C + DW_C - 1) / DW_C;
  V2A_REQUIRE(tx * ty < 0x7fffffffLL && cb <= 65535, "v2a_convnext_dwconv: H=%d W=%d C=%d exceed one launch", H, W, C);
  hipLaunchKernelGGL(convnext_dwconv_kernel, dim3((unsigned)(tx * ty), (unsigned)cb, (unsigned)F), dim3(256), 0, (hipStream_t)stream, x, out, wt,
                     bias, H, W, C, (int)tx);
  return v2a_check_launch("v2a_convnext_dwconv");
}

extern "C" int v2a_convnext_pool_ln(const float* x, int64_t frame_stride, int32_t F, int32_t pixels, int32_t C, const float* gamma,
                                    const float* beta, float eps, float* out, int64_t ldo, v2a_stream_t stream) {
  V2A_REQUIRE(x && gamma && beta && out, "v2a_convnext_pool_ln: null pointer");
  V2A_REQUIRE(F > 0 && pixels > 0 && C > 0 && C <= 256 * PL_V && frame_stride >= (int64_t)pixels * C && ldo >= C,
              "v2a_convnext_pool_ln: F=%d pixels=%d C=%d (<= %d) frame_stride=%lld ldo=%lld", F, pixels, C, 256 * PL_V, (long long)frame_stride,
              (long long)ldo);
  hipLaunchKernelGGL(convnext_pool_ln_kernel, dim3((unsigned)F), dim3(256), 0, (hipStream_t)stream, x, frame_stride, pixels, C, gamma, beta, eps, out,
                     ldo);
  return v2a_check_launch("v2a_convnext_pool_ln");
}
