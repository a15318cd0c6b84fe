// The arithmetic around the DiT in the validation pass of `E2TTS.forward(val=True)` (e2_tts_crossatt3.py:2307-2588): the
// flow-matching interpolation in front of the transformer and the two losses behind it.
//
//   * cfm_interp: w = (1 - t) x0 + t x1, flow = x1 - x0 and cond = span ? 0 : x1 in one pass over the latents.  w is two rounded
//     products and a rounded sum, the bits of torch's fp32 `(1. - t) * x0 + t * x1`.  The library is compiled with
//     -ffp-contract=fast, under which __fmul_rn / __fadd_rn (plain operators in the HIP headers) still came out as v_pk_fma_f32, so
//     each product also passes through an empty asm statement: the compiler cannot fuse what it cannot see through.
//   * masked_sqerr / roll_metrics: sums over the masked frames, in double.  Every thread sums its grid-stride share, a wave
//     reduces by shuffles, the four waves of a workgroup through LDS, and the workgroup stores its partial in `scratch`; a second
//     launch of one workgroup sums the partials the same way.  The shape alone fixes the grid, so every addition happens in the
//     same order on every run: no atomics, identical bits.
#include "v2a_common.h"

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / V2A_WAVE;

// the value as it is, behind a wall for the optimiser: a product that went through here is rounded, never the inside of an FMA
__device__ __forceinline__ float rounded(float v) {
  asm("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(256) void cfm_interp_kernel(const f32x4* __restrict__ x0, const f32x4* __restrict__ x1, const float* __restrict__ t,
                                                         const uint8_t* __restrict__ span, f32x4* __restrict__ w, f32x4* __restrict__ flow,
                                                         f32x4* __restrict__ cond, int64_t n4, int32_t row4, int64_t clip4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float tb = t[i / clip4];
  const float omt = __fsub_rn(1.0f, tb);
  const f32x4 a = x0[i], b = x1[i];
  f32x4 wv, fv;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    wv[c] = __fadd_rn(rounded(__fmul_rn(omt, a[c])), rounded(__fmul_rn(tb, b[c])));
    fv[c] = __fsub_rn(b[c], a[c]);
  }
  w[i] = wv;
  flow[i] = fv;
  if (cond) cond[i] = (span && span[i / row4]) ? f32x4{0.f, 0.f, 0.f, 0.f} : b;
}

// Sum of K doubles per thread over the workgroup, in a fixed order; thread 0 stores the K sums at dst.
template <int K>
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* __restrict__ dst) {
  __shared__ double part[LOSS_WAVES][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0) part[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = part[0][k];
#pragma unroll
      for (int q = 1; q < LOSS_WAVES; ++q) s += part[q][k];
      dst[k] = s;
    }
  }
}

// one workgroup: out[k] = sum over the `parts` partials of scratch[part][k]
template <int K>
__global__ __launch_bounds__(LOSS_THREADS) void loss_final_kernel(const double* __restrict__ scratch, int32_t parts, double* __restrict__ out) {
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int p = threadIdx.x; p < parts; p += LOSS_THREADS) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += scratch[(int64_t)p * K + k];
  }
  block_sum_store<K>(v, out);
}

// partial[block] = (sum of (pred - target)^2, number of elements) over the frames with mask != 0
__global__ __launch_bounds__(LOSS_THREADS) void masked_sqerr_kernel(const f32x4* __restrict__ pred, const f32x4* __restrict__ target,
                                                                    const uint8_t* __restrict__ mask, int64_t n4, int32_t row4,
                                                                    double* __restrict__ scratch) {
  double v[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * LOSS_THREADS) {
    if (!mask[i / row4]) continue;
    const f32x4 p = pred[i], q = target[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double d = (double)p[c] - (double)q[c];
      v[0] += d * d;
    }
    v[1] += 4.0;
  }
  block_sum_store<2>(v, scratch + (int64_t)blockIdx.x * 2);
}

__device__ __forceinline__ float mean3(float a, float b, float c) { return __fdiv_rn(__fadd_rn(__fadd_rn(a, b), c), 3.0f); }

// partial[block] = (sum of (roll - midi)^2 |midi - 0.10|, number of elements) over the masked frames, then tp, fp, fn, tn over the
// (clip, frame triple, note) cells whose three frames are all masked in: roll >= 0.4 against midi >= 0.5 on the 3-frame means
__global__ __launch_bounds__(LOSS_THREADS) void roll_metrics_kernel(const float* __restrict__ roll, const float* __restrict__ midis,
                                                                    const uint8_t* __restrict__ mask, int32_t T, int32_t notes, int64_t n,
                                                                    int64_t cells, double* __restrict__ scratch) {
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t first = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * LOSS_THREADS;
  for (int64_t i = first; i < n; i += stride) {
    if (!mask[i / notes]) continue;
    const double m = (double)midis[i], d = (double)roll[i] - m;
    v[0] += d * d * fabs(m - 0.10);
    v[1] += 1.0;
  }
  const int32_t T3 = T / 3;
  const int64_t clip_cells = (int64_t)T3 * notes;
  for (int64_t i = first; i < cells; i += stride) {
    const int64_t b = i / clip_cells, r = i % clip_cells;
    const int64_t g = r / notes, f = r % notes;
    const int64_t row = b * T + 3 * g;
    if (!(mask[row] && mask[row + 1] && mask[row + 2])) continue;
    const int64_t e = row * notes + f;
    const bool on = mean3(roll[e], roll[e + notes], roll[e + 2 * notes]) >= 0.4f;
    const bool gt = mean3(midis[e], midis[e + notes], midis[e + 2 * notes]) >= 0.5f;
    v[2] += (on && gt) ? 1.0 : 0.0;                  // tp
    v[3] += (on && !gt) ? 1.0 : 0.0;                 // fp
    v[4] += (!on && gt) ? 1.0 : 0.0;                 // fn
    v[5] += (!on && !gt) ? 1.0 : 0.0;                // tn
  }
  block_sum_store<6>(v, scratch + (int64_t)blockIdx.x * 6);
}

// workgroups of a partial launch over `items` work items: about four items a thread, at most V2A_LOSS_MAX_PARTS
inline int loss_parts(int64_t items) {
  const int64_t want = (items + 4 * LOSS_THREADS - 1) / (4 * LOSS_THREADS);
  return (int)(want < 1 ? 1 : (want > V2A_LOSS_MAX_PARTS ? V2A_LOSS_MAX_PARTS : want));
}

}  // namespace

extern "C" int v2a_cfm_interp(const float* x0, const float* x1, const float* t, const uint8_t* span, float* w, float* flow, float* cond,
                              int32_t B, int32_t T, int32_t C, v2a_stream_t stream) {
  V2A_REQUIRE(x0 && x1 && t && w && flow, "v2a_cfm_interp: null pointer");
  V2A_REQUIRE(B >= 1 && T >= 1 && C >= 4 && C % 4 == 0 && (int64_t)B * T * C <= ((int64_t)1 << 40), "v2a_cfm_interp: B=%d T=%d C=%d (C a multiple of 4)", B, T, C);
  V2A_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)w | (uintptr_t)flow | (uintptr_t)cond) & 15) == 0 && ((uintptr_t)t & 3) == 0,
              "v2a_cfm_interp: alignment (16 bytes for the latents)");
  const int64_t n4 = (int64_t)B * T * C / 4;
  V2A_REQUIRE((n4 + 255) / 256 <= 0x7fffffff, "v2a_cfm_interp: B=%d T=%d C=%d", B, T, C);
  hipLaunchKernelGGL(cfm_interp_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)x0, (const f32x4*)x1, t,
                     span, (f32x4*)w, (f32x4*)flow, (f32x4*)cond, n4, C / 4, (int64_t)T * C / 4);
  return v2a_check_launch("v2a_cfm_interp");
}

extern "C" int v2a_masked_sqerr(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t T, int32_t C, double* scratch,
                                double* out, v2a_stream_t stream) {
  V2A_REQUIRE(pred && target && mask && scratch && out, "v2a_masked_sqerr: null pointer");
  V2A_REQUIRE(B >= 1 && T >= 1 && C >= 4 && C % 4 == 0 && (int64_t)B * T * C <= ((int64_t)1 << 40), "v2a_masked_sqerr: B=%d T=%d C=%d (C a multiple of 4)", B, T, C);
  V2A_REQUIRE((((uintptr_t)pred | (uintptr_t)target) & 15) == 0 && (((uintptr_t)scratch | (uintptr_t)out) & 7) == 0,
              "v2a_masked_sqerr: alignment (16 bytes for pred and target, 8 for scratch and out)");
  const int64_t n4 = (int64_t)B * T * C / 4;
  const int parts = loss_parts(n4);
  hipLaunchKernelGGL(masked_sqerr_kernel, dim3(parts), dim3(LOSS_THREADS), 0, (hipStream_t)stream, (const f32x4*)pred, (const f32x4*)target, mask, n4,
                     C / 4, scratch);
  hipLaunchKernelGGL(loss_final_kernel<2>, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, scratch, parts, out);
  return v2a_check_launch("v2a_masked_sqerr");
}

extern "C" int v2a_roll_metrics(const float* roll, const float* midis, const uint8_t* mask, int32_t B, int32_t T, int32_t notes, double* scratch,
                                double* out, v2a_stream_t stream) {
  V2A_REQUIRE(roll && midis && mask && scratch && out, "v2a_roll_metrics: null pointer");
  V2A_REQUIRE(B >= 1 && T >= 1 && notes >= 1 && (int64_t)B * T * notes <= ((int64_t)1 << 40), "v2a_roll_metrics: B=%d T=%d notes=%d", B, T, notes);
  V2A_REQUIRE((((uintptr_t)roll | (uintptr_t)midis) & 3) == 0 && (((uintptr_t)scratch | (uintptr_t)out) & 7) == 0, "v2a_roll_metrics: alignment");
  const int64_t n = (int64_t)B * T * notes;
  const int parts = loss_parts(n);
  hipLaunchKernelGGL(roll_metrics_kernel, dim3(parts), dim3(LOSS_THREADS), 0, (hipStream_t)stream, roll, midis, mask, T, notes, n,
                     (int64_t)B * (T / 3) * notes, scratch);
  hipLaunchKernelGGL(loss_final_kernel<6>, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, scratch, parts, out);
  return v2a_check_launch("v2a_roll_metrics");
}
