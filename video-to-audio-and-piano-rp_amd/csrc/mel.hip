// The log-mel front end: the reference's `MelSpec` (x3:375-417), a torchaudio MelSpectrogram followed by log(clamp(mel, 1e-5)).
//
// The short-time Fourier transform is a GEMM over overlapping rows, the Encodec encoder's lda = stride * C trick with C = 1: frame t of
// a padded wave starts hop samples after frame t - 1, so v2a_gemm (exact fp32, lda = hop, K = n_fft) on the windowed real DFT basis
// (mel.py: stft_basis) gives re | im of every frame of every clip in one launch.  The exact-fp32 GEMM adds its K products in one chain,
// whose rounding error grows with K; mel.py therefore cuts K into chunks of 256 samples, one launch and one partial DFT each (the A and
// W pointers moved by the chunk, lda and ldw unchanged), and mel_from_dft adds the partials in chunk order.  Two kernels stand around it:
//   * mel_pad:      (B, nw) waves -> one buffer of B padded waves `pitch` samples apart (pitch a multiple of hop, so frame t of clip b is
//                   GEMM row b * pitch / hop + t): `pad` reflected samples on both sides (torch.stft's center = True), or a plain copy.
//   * mel_from_dft: per frame re^2 + im^2 (power 2) or its square root (power 1) of every bin, the mel projection and the log, stored
//                   transposed as (B, n_mels, T).  A workgroup takes MEL_TF consecutive frames of one clip: it reads their DFT rows
//                   row-major (lanes along the bins: 8-byte loads, coalesced), leaves the powers in LDS bin-major, and then runs one
//                   thread per (mel channel, frame) with the frame in the low lane bits, so the stores run along time.  The filterbank
//                   comes in band form -- per channel the first bin, the bin count and that many weights -- and a mel value is ONE
//                   chain of fmaf over its bins from the first up: its bits depend on the frame's DFT row and the channel's weights
//                   alone, not on the tile, the batch or the clip length.  No atomics.
// The log is taken in double and rounded once, log(1e-5f) included: a mel value's log does not depend on a fp32 libm.
#include "v2a_common.h"

#include <math.h>

namespace {

constexpr int MEL_THREADS = 256;
constexpr int MEL_TF = 16;                          // frames of a workgroup's tile
constexpr int MEL_LD = MEL_TF + 1;                  // floats between two bins in LDS: lanes along the bins fall on distinct banks
constexpr int MEL_LDS_MAX = (V2A_MEL_MAX_FFT / 2 + 1) * MEL_LD * (int)sizeof(float);

__global__ __launch_bounds__(MEL_THREADS) void mel_pad_kernel(const float* __restrict__ x, int64_t ldx, int64_t nw, int32_t pad,
                                                              float* __restrict__ out, int64_t pitch) {
  const int64_t i = (int64_t)blockIdx.x * MEL_THREADS + threadIdx.x;
  if (i >= nw + 2 * (int64_t)pad) return;
  int64_t src = i - pad;
  if (src < 0) src = -src;                          // pad < nw: one reflection lands inside the wave
  if (src >= nw) src = 2 * (nw - 1) - src;
  out[blockIdx.y * pitch + i] = x[blockIdx.y * ldx + src];
}

struct MelParams {
  const float* dft;
  const int32_t* bands;
  const float* weights;
  float* out;
  int64_t ld_dft, rows_per_clip, chunk_stride, out_batch_stride, out_row_stride;
  int32_t T, n_bins, n_mels, wpitch, n_chunks;
  float eps;
};

template <int POWER>
__global__ __launch_bounds__(MEL_THREADS) void mel_from_dft_kernel(MelParams P) {
  extern __shared__ float pw[];                     // [n_bins][MEL_LD]: the power (or magnitude) of bin k in frame f at pw[k * MEL_LD + f]
  const int clip = blockIdx.y;
  const int t0 = blockIdx.x * MEL_TF;
  const int nf = P.T - t0 < MEL_TF ? P.T - t0 : MEL_TF;          // frames of this tile inside the clip; the rows behind them are not read
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int f = wave; f < MEL_TF; f += MEL_THREADS / V2A_WAVE) {
    const float* row = P.dft + ((int64_t)clip * P.rows_per_clip + t0 + f) * P.ld_dft;
    for (int k = lane; k < P.n_bins; k += V2A_WAVE) {
      float p = 0.0f;
      if (f < nf) {
        f32x2 v = *reinterpret_cast<const f32x2*>(row + 2 * k);
        for (int c = 1; c < P.n_chunks; ++c) {        // the partial DFTs of the K chunks, added in chunk order
          const f32x2 q = *reinterpret_cast<const f32x2*>(row + c * P.chunk_stride + 2 * k);
          v[0] = __fadd_rn(v[0], q[0]);
          v[1] = __fadd_rn(v[1], q[1]);
        }
        p = __fmaf_rn(v[1], v[1], __fmul_rn(v[0], v[0]));
        if (POWER == 1) p = __fsqrt_rn(p);
      }
      pw[k * MEL_LD + f] = p;
    }
  }
  __syncthreads();
  const int f = threadIdx.x & (MEL_TF - 1);
  for (int m = threadIdx.x / MEL_TF; m < P.n_mels; m += MEL_THREADS / MEL_TF) {
    // the entry point has checked the host's copy of the table; the clamps keep any table inside LDS and inside the channel's weight row
    int first = P.bands[2 * m], count = P.bands[2 * m + 1];
    first = first < 0 ? 0 : (first > P.n_bins ? P.n_bins : first);
    count = count < 0 ? 0 : count;
    count = count > P.n_bins - first ? P.n_bins - first : count;
    count = count > P.wpitch ? P.wpitch : count;
    const float* w = P.weights + (int64_t)m * P.wpitch;
    const float* s = pw + first * MEL_LD + f;
    float acc = 0.0f;
    for (int i = 0; i < count; ++i) acc = __fmaf_rn(w[i], s[i * MEL_LD], acc);
    if (f < nf)
      P.out[clip * P.out_batch_stride + m * P.out_row_stride + t0 + f] = P.eps < 0.0f ? acc : (float)log((double)fmaxf(acc, P.eps));
  }
}

}  // namespace

extern "C" int v2a_mel_pad(const float* x, int64_t ldx, int32_t B, int64_t nw, int32_t pad, float* out, int64_t pitch, v2a_stream_t stream) {
  V2A_REQUIRE(x && out && x != out, "v2a_mel_pad: null / aliased pointer");
  V2A_REQUIRE(B >= 1 && B <= 65535 && nw >= 1 && nw <= ((int64_t)1 << 30) && pad >= 0 && pad < nw && ldx >= nw && pitch >= nw + 2 * (int64_t)pad,
              "v2a_mel_pad: B=%d nw=%lld pad=%d ldx=%lld pitch=%lld (1 <= B <= 65535, a reflected pad is shorter than the wave, ldx >= nw, "
              "pitch >= nw + 2 pad)", B, (long long)nw, pad, (long long)ldx, (long long)pitch);
  V2A_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "v2a_mel_pad: alignment");
  const int64_t blocks = (nw + 2 * (int64_t)pad + MEL_THREADS - 1) / MEL_THREADS;
  hipLaunchKernelGGL(mel_pad_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(MEL_THREADS), 0, (hipStream_t)stream, x, ldx, nw, pad, out, pitch);
  return v2a_check_launch("v2a_mel_pad");
}

extern "C" int v2a_mel_from_dft(const float* dft, int64_t ld_dft, int64_t rows_per_clip, int32_t n_chunks, int64_t chunk_stride, int32_t B,
                                int32_t T, int32_t n_fft, int32_t hop,
                                int32_t n_mels, const int32_t* bands_host, const int32_t* bands, const float* weights, int32_t wpitch,
                                int32_t power, float eps, float* out, int64_t out_batch_stride, int64_t out_row_stride, v2a_stream_t stream) {
  V2A_REQUIRE(dft && bands_host && bands && weights && out, "v2a_mel_from_dft: null pointer");
  V2A_REQUIRE(n_fft >= 4 && n_fft % 2 == 0 && n_fft <= V2A_MEL_MAX_FFT, "v2a_mel_from_dft: n_fft=%d (even, 4 .. %d)", n_fft, V2A_MEL_MAX_FFT);
  V2A_REQUIRE(hop >= 1 && hop % 4 == 0, "v2a_mel_from_dft: hop=%d (a positive multiple of 4: the lda of the exact-fp32 GEMM in front)", hop);
  V2A_REQUIRE(n_mels >= 1 && n_mels <= (1 << 16), "v2a_mel_from_dft: n_mels=%d", n_mels);
  V2A_REQUIRE(power == 1 || power == 2, "v2a_mel_from_dft: power=%d (1 or 2)", power);
  const int n_bins = n_fft / 2 + 1;
  V2A_REQUIRE(wpitch >= 1 && wpitch <= n_bins, "v2a_mel_from_dft: wpitch=%d (1 .. n_fft / 2 + 1 = %d)", wpitch, n_bins);
  for (int m = 0; m < n_mels; ++m) {
    const int first = bands_host[2 * m], count = bands_host[2 * m + 1];
    V2A_REQUIRE(first >= 0 && count >= 0 && count <= wpitch && (int64_t)first + count <= n_bins,
                "v2a_mel_from_dft: band %d = bins [%d, %d + %d) outside the %d bins or wider than wpitch=%d", m, first, first, count, n_bins, wpitch);
  }
  V2A_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && rows_per_clip >= T && ld_dft >= 2 * (int64_t)n_bins && ld_dft % 2 == 0,
              "v2a_mel_from_dft: B=%d T=%d rows_per_clip=%lld ld_dft=%lld (1 <= B <= 65535, rows_per_clip >= T >= 1, ld_dft even and >= 2 bins)", B, T,
              (long long)rows_per_clip, (long long)ld_dft);
  V2A_REQUIRE(n_chunks >= 1 && n_chunks <= V2A_MEL_MAX_CHUNKS && chunk_stride % 2 == 0 &&
                  (n_chunks == 1 || chunk_stride >= ((int64_t)(B - 1) * rows_per_clip + T) * ld_dft),
              "v2a_mel_from_dft: n_chunks=%d chunk_stride=%lld (1 .. %d partial DFTs, an even number of floats apart and no closer than the "
              "(B - 1) rows_per_clip + T rows of one)", n_chunks, (long long)chunk_stride, V2A_MEL_MAX_CHUNKS);
  V2A_REQUIRE(out_row_stride >= T && out_batch_stride >= (int64_t)(n_mels - 1) * out_row_stride + T,
              "v2a_mel_from_dft: out_row_stride=%lld out_batch_stride=%lld (rows of T=%d frames, clips of n_mels=%d rows)", (long long)out_row_stride,
              (long long)out_batch_stride, T, n_mels);
  V2A_REQUIRE(((uintptr_t)dft & 7) == 0 && (((uintptr_t)bands | (uintptr_t)weights | (uintptr_t)out) & 3) == 0, "v2a_mel_from_dft: alignment (8 bytes for dft)");
  MelParams P;
  P.dft = dft, P.bands = bands, P.weights = weights, P.out = out;
  P.ld_dft = ld_dft, P.rows_per_clip = rows_per_clip, P.chunk_stride = chunk_stride, P.out_batch_stride = out_batch_stride, P.out_row_stride = out_row_stride;
  P.T = T, P.n_bins = n_bins, P.n_mels = n_mels, P.wpitch = wpitch, P.n_chunks = n_chunks;
  P.eps = eps;
  const size_t lds = (size_t)n_bins * MEL_LD * sizeof(float);
  const dim3 grid((unsigned)((T + MEL_TF - 1) / MEL_TF), (unsigned)B);
  if (power == 1) {
    static std::atomic<uint64_t> lds_set{0};
    if (lds > 64 * 1024)
      if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(mel_from_dft_kernel<1>), MEL_LDS_MAX, lds_set, "v2a_mel_from_dft")) return rc;
    hipLaunchKernelGGL(mel_from_dft_kernel<1>, grid, dim3(MEL_THREADS), lds, (hipStream_t)stream, P);
  } else {
    static std::atomic<uint64_t> lds_set{0};
    if (lds > 64 * 1024)
      if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(mel_from_dft_kernel<2>), MEL_LDS_MAX, lds_set, "v2a_mel_from_dft")) return rc;
    hipLaunchKernelGGL(mel_from_dft_kernel<2>, grid, dim3(MEL_THREADS), lds, (hipStream_t)stream, P);
  }
  return v2a_check_launch("v2a_mel_from_dft");
}
