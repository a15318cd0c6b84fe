// The wave front end of the reference's data path (trainer_multigpus_alldatas3.py:1047-1050, 1427-1431; torch_tools.py:53-56): what
// turns the first channel of an audio file at any rate into the 24 kHz wave the Encodec encoder reads.
//
//   * wave_resample: torchaudio's `functional.resample` as a polyphase FIR.  With o / n the reduced input / output rates and
//     table (n phases, K = 2 * width + o taps) built on the host (wave.py), output j = q * n + p is
//         y[j] = sum_k xpad[q * o + k] * table[p][k],    xpad = the wave with `width` zeros in front and zeros behind.
//     One thread owns one output and runs the K taps as one chain of fmaf from k = 0 up, the zero padding included, so a sample's
//     bits depend on its window and its table row alone: not on the tile it fell in, not on the path the table took.  A workgroup
//     takes `Q` consecutive q (all n phases of each), stages their input window in LDS, and stages the whole table beside it when
//     both fit V2A_WAVE_LDS_BYTES; a larger table is read from global memory by the same loop.  Table rows are K floats apart and
//     K is odd for every rate whose o is odd (44.1 / 22.05 / 11.025 kHz), so the n phases of a wave fall on distinct LDS banks.
//   * wave_stats: the partials of a wave that is already at the target rate.
//   * Both store one partial per workgroup: the sum of its samples in double and their fp32 minimum and maximum.  Every thread sums
//     its samples in index order, a wave reduces by shuffles, the four waves through LDS: an order the shape alone fixes.
//   * wave_normalize: every workgroup reads the partials into LDS and its first thread adds them in index order (at most
//     V2A_WAVE_MAX_PARTS doubles), so every workgroup holds the same m and peak without a launch in between; then
//     (x - m) / (peak + 1e-8f) * 0.5f, three rounded fp32 operations, written into a destination that cuts or zero-pads the wave.
// No atomics anywhere: two runs give the same bits (as in cfm_loss.hip).
#include "v2a_common.h"

#include <math.h>

namespace {

constexpr int WAVE_THREADS = 256;
constexpr int WAVE_WAVES = WAVE_THREADS / V2A_WAVE;
constexpr int WAVE_TILE_OUT = 1024;                 // outputs a workgroup aims at per tile (Q = WAVE_TILE_OUT / n, at least 1)
constexpr int WAVE_WINDOW_MAX = 8192;               // floats of the staged input window: (Q - 1) * o + K

struct WavePart {                                   // 16 bytes: the layout of `parts` in include/v2a_cfm.h
  double sum;
  float mn, mx;
};

// (sum, min, max) over the workgroup in a fixed order; thread 0 stores them
__device__ __forceinline__ void block_part_store(double s, float mn, float mx, WavePart* __restrict__ dst) {
  __shared__ WavePart part[WAVE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) part[wave] = WavePart{s, mn, mx};
  __syncthreads();
  if (threadIdx.x == 0) {
    WavePart r = part[0];
#pragma unroll
    for (int q = 1; q < WAVE_WAVES; ++q) {
      r.sum += part[q].sum;
      r.mn = fminf(r.mn, part[q].mn);
      r.mx = fmaxf(r.mx, part[q].mx);
    }
    *dst = r;
  }
}

struct ResampleParams {
  const float* x;
  const float* table;
  float* y;
  WavePart* parts;
  int64_t L, out_len, tiles;
  int32_t o, n, K, width, Q, win_len;
};

template <bool LDS_TABLE>
__global__ __launch_bounds__(WAVE_THREADS) void wave_resample_kernel(ResampleParams P) {
  extern __shared__ float smem[];
  float* win = smem;                                  // win_len floats
  const float* tab = P.table;
  if constexpr (LDS_TABLE) {
    float* t = smem + P.win_len;
    for (int i = threadIdx.x; i < P.n * P.K; i += WAVE_THREADS) t[i] = P.table[i];
    tab = t;
  }
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  const int tile_out = P.Q * P.n;
  for (int64_t tile = blockIdx.x; tile < P.tiles; tile += gridDim.x) {
    const int64_t q0 = tile * P.Q;
    __syncthreads();                                  // the window of the tile before has been read
    const int64_t g0 = q0 * P.o - P.width;            // wave index of win[0]
    for (int i = threadIdx.x; i < P.win_len; i += WAVE_THREADS) {
      const int64_t g = g0 + i;
      win[i] = (g >= 0 && g < P.L) ? P.x[g] : 0.0f;
    }
    __syncthreads();
    for (int jj = threadIdx.x; jj < tile_out; jj += WAVE_THREADS) {
      const int64_t j = q0 * P.n + jj;
      if (j >= P.out_len) break;
      const int ql = jj / P.n, p = jj - ql * P.n;
      const float* xw = win + ql * P.o;               // ql < Q: xw[K - 1] is win[(Q - 1) * o + K - 1] at most
      const float* tr = tab + (int64_t)p * P.K;
      float acc = 0.0f;
#pragma unroll 4
      for (int k = 0; k < P.K; ++k) acc = fmaf(xw[k], tr[k], acc);
      P.y[j] = acc;
      s += (double)acc;
      mn = fminf(mn, acc);
      mx = fmaxf(mx, acc);
    }
  }
  block_part_store(s, mn, mx, P.parts + blockIdx.x);
}

__global__ __launch_bounds__(WAVE_THREADS) void wave_stats_kernel(const float* __restrict__ x, int64_t n, WavePart* __restrict__ parts) {
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * WAVE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WAVE_THREADS) {
    const float v = x[i];
    s += (double)v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_part_store(s, mn, mx, parts + blockIdx.x);
}

__global__ __launch_bounds__(WAVE_THREADS) void wave_normalize_kernel(const float* __restrict__ x, int64_t n, const WavePart* __restrict__ parts,
                                                                     int32_t n_parts, float* __restrict__ out, int64_t n_out,
                                                                     float* __restrict__ stats) {
  __shared__ WavePart sp[V2A_WAVE_MAX_PARTS];
  __shared__ float mp[2];
  for (int i = threadIdx.x; i < n_parts; i += WAVE_THREADS) sp[i] = parts[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    WavePart r = sp[0];
    for (int i = 1; i < n_parts; ++i) {
      r.sum += sp[i].sum;
      r.mn = fminf(r.mn, sp[i].mn);
      r.mx = fmaxf(r.mx, sp[i].mx);
    }
    const float m = (float)(r.sum / (double)n);
    const float peak = fmaxf(__fsub_rn(r.mx, m), __fsub_rn(m, r.mn));
    mp[0] = m;
    mp[1] = peak;
    if (blockIdx.x == 0) {
      stats[0] = m;
      stats[1] = peak;
    }
  }
  __syncthreads();
  const float m = mp[0], den = __fadd_rn(mp[1], 1e-8f);
  for (int64_t i = (int64_t)blockIdx.x * WAVE_THREADS + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * WAVE_THREADS)
    out[i] = i < n ? __fmul_rn(__fdiv_rn(__fsub_rn(x[i], m), den), 0.5f) : 0.0f;
}

inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int v2a_wave_resample(const float* x, int64_t L, const float* table, int32_t o, int32_t n, int32_t K, int32_t width, float* y,
                                 int64_t out_len, void* parts, int32_t* n_parts, v2a_stream_t stream) {
  V2A_REQUIRE(x && table && y && parts && n_parts, "v2a_wave_resample: null pointer");
  V2A_REQUIRE(o >= 1 && n >= 1 && width >= 1 && K == 2 * width + o && K <= WAVE_WINDOW_MAX && (int64_t)n * K <= V2A_WAVE_TABLE_MAX,
              "v2a_wave_resample: o=%d n=%d width=%d K=%d (K = 2 width + o <= %d, n K <= %d)", o, n, width, K, WAVE_WINDOW_MAX, V2A_WAVE_TABLE_MAX);
  V2A_REQUIRE(L >= 1 && L <= ((int64_t)1 << 40) && out_len == ceil_div64((int64_t)n * L, o), "v2a_wave_resample: L=%lld out_len=%lld (ceil(n L / o))",
              (long long)L, (long long)out_len);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)table | (uintptr_t)y) & 3) == 0 && ((uintptr_t)parts & 7) == 0, "v2a_wave_resample: alignment");
  ResampleParams P;
  P.x = x, P.table = table, P.y = y, P.parts = (WavePart*)parts;
  P.L = L, P.out_len = out_len;
  P.o = o, P.n = n, P.K = K, P.width = width;
  int64_t Q = WAVE_TILE_OUT / n < 1 ? 1 : WAVE_TILE_OUT / n;
  const int64_t q_fit = (WAVE_WINDOW_MAX - K) / o + 1;                 // (Q - 1) * o + K <= WAVE_WINDOW_MAX
  if (Q > q_fit) Q = q_fit;
  P.Q = (int32_t)Q;
  P.win_len = (int32_t)((Q - 1) * o + K);
  P.tiles = ceil_div64(ceil_div64(out_len, n), Q);
  const int grid = (int)(P.tiles < V2A_WAVE_MAX_PARTS ? P.tiles : V2A_WAVE_MAX_PARTS);
  *n_parts = grid;
  const size_t win_bytes = (size_t)P.win_len * sizeof(float), tab_bytes = (size_t)n * K * sizeof(float);
  if (win_bytes + tab_bytes <= V2A_WAVE_LDS_BYTES) {
    static std::atomic<uint64_t> lds_set{0};
    if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(wave_resample_kernel<true>), V2A_WAVE_LDS_BYTES, lds_set, "v2a_wave_resample")) return rc;
    hipLaunchKernelGGL(wave_resample_kernel<true>, dim3(grid), dim3(WAVE_THREADS), win_bytes + tab_bytes, (hipStream_t)stream, P);
  } else {
    hipLaunchKernelGGL(wave_resample_kernel<false>, dim3(grid), dim3(WAVE_THREADS), win_bytes, (hipStream_t)stream, P);
  }
  return v2a_check_launch("v2a_wave_resample");
}

extern "C" int v2a_wave_stats(const float* x, int64_t n, void* parts, int32_t* n_parts, v2a_stream_t stream) {
  V2A_REQUIRE(x && parts && n_parts, "v2a_wave_stats: null pointer");
  V2A_REQUIRE(n >= 1 && n <= ((int64_t)1 << 40), "v2a_wave_stats: n=%lld", (long long)n);
  V2A_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)parts & 7) == 0, "v2a_wave_stats: alignment");
  const int64_t want = ceil_div64(n, 8 * WAVE_THREADS);                // about eight samples a thread
  const int grid = (int)(want < V2A_WAVE_MAX_PARTS ? want : V2A_WAVE_MAX_PARTS);
  *n_parts = grid;
  hipLaunchKernelGGL(wave_stats_kernel, dim3(grid), dim3(WAVE_THREADS), 0, (hipStream_t)stream, x, n, (WavePart*)parts);
  return v2a_check_launch("v2a_wave_stats");
}

extern "C" int v2a_wave_normalize(const float* x, int64_t n, const void* parts, int32_t n_parts, float* out, int64_t n_out, float* stats,
                                  v2a_stream_t stream) {
  V2A_REQUIRE(x && parts && out && stats, "v2a_wave_normalize: null pointer");
  V2A_REQUIRE(n >= 1 && n <= ((int64_t)1 << 40) && n_out >= 1 && n_out <= ((int64_t)1 << 40) && n_parts >= 1 && n_parts <= V2A_WAVE_MAX_PARTS,
              "v2a_wave_normalize: n=%lld n_out=%lld n_parts=%d (1 .. %d)", (long long)n, (long long)n_out, n_parts, V2A_WAVE_MAX_PARTS);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)stats) & 3) == 0 && ((uintptr_t)parts & 7) == 0, "v2a_wave_normalize: alignment");
  const int64_t want = ceil_div64(n_out, 4 * WAVE_THREADS);
  const int grid = (int)(want < 1024 ? want : 1024);
  hipLaunchKernelGGL(wave_normalize_kernel, dim3(grid), dim3(WAVE_THREADS), 0, (hipStream_t)stream, x, n, (const WavePart*)parts, n_parts, out,
                     n_out, stats);
  return v2a_check_launch("v2a_wave_normalize");
}
