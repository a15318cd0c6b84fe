// Encodec (24 kHz SEANet) encoder -- `EncodecWrapper.forward` (x3:428-432, predict.py:222): the mirror of vocoder.hip.
// From the first down-sampling convolution on, every layer is a v2a_gemm on a time-major [T][C] buffer: a strided
// Conv1d(k = 2r, stride r) reads overlapping rows with lda = r*C, K = k*C.  Two kernels complete the stack:
//   * elu_pad_lr: out[pl + t] = ELU(x[t]) with pl reflected rows in front and pr reflected rows behind (EncodecConv1d pads
//                 on the right wherever the input length is not a multiple of the stride);
//   * stage0:     the wide, thin end -- waveform -> stem Conv1d(1->32, k7) -> residual block at C = 32 -> [n][32] -- in one
//                 pass: one thread per sample, ~3.3 k FMAs per thread on weights that every lane reads at the same address,
//                 one coalesced write of the [n][32] result.
#include "v2a_common.h"

namespace {

__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }

// one thread per float4 of the padded output
__global__ __launch_bounds__(256) void elu_pad_lr_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t T, int C4,
                                                         int pad_left, int pad_right, int act) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (T + pad_left + pad_right) * C4) return;
  const int64_t row = gid / C4;
  const int c4 = (int)(gid - row * C4);
  int64_t src = row - pad_left;
  if (src < 0) src = -src;                           // front: padded row (pad_left - i) mirrors row i
  if (src >= T) src = 2 * (T - 1) - src;             // back: padded row T - 1 + i mirrors row T - 1 - i; the edge rows are not repeated
  f32x4 v = *reinterpret_cast<const f32x4*>(x + (src * C4 + c4) * 4);
  if (act) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = elu_f(v[e]);
  }
  *reinterpret_cast<f32x4*>(out + gid * 4) = v;
}

// ---- stage 0: stem + residual block at C = 32 ----------------------------------------------------------------------
// Parameter block (floats), see v2a_encodec_stage0 in v2a_cfm.h:
constexpr int S0_C = 32, S0_H = 16, S0_K0 = 7, S0_K1 = 3;
constexpr int S0_W0 = 0;                              // stem weight [32][7]
constexpr int S0_B0 = S0_W0 + S0_C * S0_K0;           // stem bias [32]
constexpr int S0_WS = S0_B0 + S0_C;                   // shortcut weight [32][32]
constexpr int S0_BS = S0_WS + S0_C * S0_C;            // shortcut bias + block.3 bias [32]
constexpr int S0_W1 = S0_BS + S0_C;                   // block.1 weight [16][3][32] (tap-major, as the GEMM path packs it)
constexpr int S0_B1 = S0_W1 + S0_H * S0_K1 * S0_C;    // block.1 bias [16]
constexpr int S0_W3 = S0_B1 + S0_H;                   // block.3 weight [32][16]
constexpr int S0_PARAMS = S0_W3 + S0_C * S0_H;        // 3376
constexpr int S0_LD = S0_C + 4;                       // LDS row stride of the store transpose: 36 floats keeps 16-byte rows off one bank slot

// Thread t computes row t of the output.  The k3 convolution of the block needs ELU(stem) at times t-2, t-1, t (reflected at the
// front: times |t-2|, |t-1|, t), which the thread recomputes from the wave (7 samples each, reflected likewise) instead of
// exchanging: 2 x 224 extra FMAs against 3.3 k.  Every weight address is the same in all lanes, so the loads are uniform and the FMAs
// take the weight as a scalar operand.  The 64 rows of a wave are one contiguous 8 KB of the output: they go through LDS so that
// consecutive lanes store consecutive 16 bytes.
__global__ __launch_bounds__(256) void encodec_stage0_kernel(const float* __restrict__ wave, const float* __restrict__ p,
                                                             float* __restrict__ out, int64_t n) {
  __shared__ float tile[256 * S0_LD];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * 256;
  const int64_t tq = t0 + tid;
  const int64_t t = tq < n ? tq : n - 1;             // tail threads compute the last row again and store nothing

  float e[S0_K1][S0_C];                              // stem output at the three taps, then its ELU
#pragma unroll
  for (int j = 0; j < S0_K1; ++j) {
    int64_t s = t - (S0_K1 - 1) + j;
    if (s < 0) s = -s;
    float x[S0_K0];
#pragma unroll
    for (int i = 0; i < S0_K0; ++i) {
      int64_t q = s - (S0_K0 - 1) + i;
      if (q < 0) q = -q;
      x[i] = wave[q];
    }
#pragma unroll
    for (int c = 0; c < S0_C; ++c) {
      float a = p[S0_B0 + c];
#pragma unroll
      for (int i = 0; i < S0_K0; ++i) a = fmaf(p[S0_W0 + c * S0_K0 + i], x[i], a);
      e[j][c] = a;
    }
  }
  float acc[S0_C];                                   // shortcut(x0[t]) + both biases of the sum
#pragma unroll
  for (int c = 0; c < S0_C; ++c) {
    float a = p[S0_BS + c];
#pragma unroll
    for (int k = 0; k < S0_C; ++k) a = fmaf(p[S0_WS + c * S0_C + k], e[S0_K1 - 1][k], a);
    acc[c] = a;
  }
#pragma unroll
  for (int j = 0; j < S0_K1; ++j) {
#pragma unroll
    for (int c = 0; c < S0_C; ++c) e[j][c] = elu_f(e[j][c]);
  }
  float h[S0_H];
#pragma unroll
  for (int d = 0; d < S0_H; ++d) {
    float a = p[S0_B1 + d];
#pragma unroll
    for (int j = 0; j < S0_K1; ++j) {
#pragma unroll
      for (int c = 0; c < S0_C; ++c) a = fmaf(p[S0_W1 + (d * S0_K1 + j) * S0_C + c], e[j][c], a);
    }
    h[d] = elu_f(a);
  }
#pragma unroll
  for (int c = 0; c < S0_C; ++c) {
    float a = acc[c];
#pragma unroll
    for (int d = 0; d < S0_H; ++d) a = fmaf(p[S0_W3 + c * S0_H + d], h[d], a);
    acc[c] = a;
  }
  // row tid of the block's [256][32] tile; read back below as 2048 consecutive float4
  float* row = tile + tid * S0_LD;
#pragma unroll
  for (int c = 0; c < S0_C; c += 4) {
    f32x4 v = {acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
    *reinterpret_cast<f32x4*>(row + c) = v;
  }
  __syncthreads();
  const int64_t rows = n - t0 < 256 ? n - t0 : 256;   // rows of this block inside the signal
#pragma unroll
  for (int i = 0; i < S0_C / 4; ++i) {
    const int f = i * 256 + tid;                      // float4 index inside the block's [256][32] tile
    const int r = f >> 3, c4 = f & 7;
    if (r < rows) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(tile + r * S0_LD + c4 * 4);
      *reinterpret_cast<f32x4*>(out + (t0 + r) * S0_C + c4 * 4) = v;
    }
  }
}

}  // namespace

extern "C" int v2a_elu_pad_lr(const float* x, float* out, int64_t T, int32_t C, int32_t pad_left, int32_t pad_right, int32_t act,
                              v2a_stream_t stream) {
  V2A_REQUIRE(x && out && x != out, "v2a_elu_pad_lr: null / aliased pointer");
  V2A_REQUIRE(T > 0 && C > 0 && C % 4 == 0 && pad_left >= 0 && pad_right >= 0 && pad_left < T && pad_right < T,
              "v2a_elu_pad_lr: T=%lld C=%d pad_left=%d pad_right=%d (reflected pads must be shorter than the signal)", (long long)T, C,
              pad_left, pad_right);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "v2a_elu_pad_lr: 16-byte alignment");
  const int64_t total = (T + pad_left + pad_right) * (C / 4);
  hipLaunchKernelGGL(elu_pad_lr_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, T, C / 4,
                     pad_left, pad_right, act);
  return v2a_check_launch("v2a_elu_pad_lr");
}

extern "C" int v2a_encodec_stage0(const float* wave, const float* params, float* out, int64_t n, v2a_stream_t stream) {
  V2A_REQUIRE(wave && params && out && wave != out, "v2a_encodec_stage0: null / aliased pointer");
  V2A_REQUIRE(n >= S0_K0 + S0_K1 - 2 && n < ((int64_t)1 << 31) * 256, "v2a_encodec_stage0: n=%lld (at least %d samples: the reflected pads)",
              (long long)n, S0_K0 + S0_K1 - 2);
  V2A_REQUIRE((((uintptr_t)params | (uintptr_t)out) & 15) == 0 && ((uintptr_t)wave & 3) == 0, "v2a_encodec_stage0: alignment (16 bytes for params / out)");
  hipLaunchKernelGGL(encodec_stage0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wave, params, out, n);
  return v2a_check_launch("v2a_encodec_stage0");
}
