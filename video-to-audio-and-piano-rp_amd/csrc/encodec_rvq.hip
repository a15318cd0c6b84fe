// Encodec residual vector quantizer -- `EncodecResidualVectorQuantizer.encode` / `.decode` with `EncodecEuclideanCodebook.quantize`
// (transformers/models/encodec/modeling_encodec.py): the part of `EncodecModel.encode` / `.decode` between encodec_enc.hip and
// vocoder.hip.  Per stage the library takes arg-max_j -(|r|^2 - 2 r.e_j + |e_j|^2) over the stage's codebook, subtracts the chosen
// codeword from the residual and goes on; `decode` sums the chosen codewords in stage order.
//
//   * rvq_encode: every requested stage in ONE launch.  A workgroup of 8 waves owns 16 frames.  The result is an index, not a value,
//     so the products are exact fp32: v_mfma_f32_16x16x4_f32 with the 16 frames as the A rows and 16 codewords as the B columns.
//     The residual never leaves registers: lane (m = lane & 15, g = lane >> 4) holds channels 16 i + 4 g + c (i < 8, c < 4) of
//     frame m, which is exactly its A operand of k-step (i, c) -- the k order of a dot product is free as long as A and B agree, and
//     this order makes the B operand of codeword j one 16-byte load per i (e_j[16 i + 4 g .. + 3]).  Every wave keeps its own copy
//     of the residual (the same bits in all eight) and scores its eighth of the codebook, 64 codewords (4 independent accumulator
//     tiles) at a time; the codebooks (512 KB per stage) stream from L2 through a one-step register prefetch.  The arg-max runs per
//     lane over the wave's tiles, then over the 16 lanes of a row (ds_bpermute), then over the 8 waves through 2 KB of LDS, double
//     buffered by stage parity so that one barrier per stage is enough.  Ties go to the lowest index at every level.
//     A frame's scores are rows of MFMA tiles, which never mix, so its codes do not depend on its neighbours in the tile or launch.
//   * rvq_decode: out = ((0 + e0[c0]) + e1[c1]) + ... in fp32, one thread per output element.
#include "v2a_common.h"

namespace {

constexpr int RVQ_D = 128;            // codebook dimension (EncodecConfig.codebook_dim = hidden_size)
constexpr int RVQ_FRAMES = 16;        // frames per workgroup = rows of one MFMA tile: a 750-frame clip is 47 workgroups
constexpr int RVQ_WAVES = 8;
constexpr int RVQ_NT = 4;             // 16-codeword tiles in flight per wave: independent accumulators hide the MFMA's 40-cycle latency
constexpr int RVQ_GROUP = 16 * RVQ_NT;

struct best_t {
  float v;
  int32_t j;
};

// (ov, oj) replaces (v, j) when it scores higher, or the same at a lower index
__device__ __forceinline__ void take_better(float& v, int32_t& j, float ov, int32_t oj) {
  if (ov > v || (ov == v && oj < j)) {
    v = ov;
    j = oj;
  }
}

__global__ __launch_bounds__(64 * RVQ_WAVES) void rvq_encode_kernel(const float* __restrict__ x, int64_t sb, int64_t st, int64_t sc, int32_t T,
                                                                    int64_t F, const float* __restrict__ cb, const float* __restrict__ nrm,
                                                                    int32_t Kc, int32_t n_q, int64_t* __restrict__ codes) {
  __shared__ best_t red[2][RVQ_WAVES][RVQ_FRAMES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int64_t f = (int64_t)blockIdx.x * RVQ_FRAMES + m;
  const bool live = f < F;

  f32x4 r[8];                                      // r[i][c] = residual[frame m][16 i + 4 g + c]; frames past the end stay zero
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* xf = x + (f / T) * sb + (f % T) * st;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int c = 0; c < 4; ++c) r[i][c] = xf[(int64_t)(16 * i + 4 * g + c) * sc];
    }
  }

  const int per_wave = Kc / RVQ_WAVES;             // codewords [wave * per_wave, (wave + 1) * per_wave) are this wave's
  const int groups = per_wave / RVQ_GROUP;
  const int steps = groups * 8;                    // (group, i) pairs: one B load per tile and four MFMAs per tile each

  for (int s = 0; s < n_q; ++s) {
    const float* e = cb + (int64_t)s * Kc * RVQ_D;
    const float* en = nrm + (int64_t)s * Kc;
    // this lane's B operand of tile t at step q = (group, i): codeword wave * per_wave + group * 64 + 16 t + m, floats 16 i + 4 g ..
    const float* eb = e + (int64_t)(wave * per_wave + m) * RVQ_D + 4 * g;
    auto load = [&](f32x4 (&b)[RVQ_NT], int q) {
      const float* p = eb + (int64_t)(q >> 3) * RVQ_GROUP * RVQ_D + (q & 7) * 16;
#pragma unroll
      for (int t = 0; t < RVQ_NT; ++t) b[t] = *reinterpret_cast<const f32x4*>(p + t * 16 * RVQ_D);
    };

    float bv[4];                                   // best score / index so far of frames 4 g + 0 .. 3 among this lane's codewords
    int32_t bj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      bv[a] = -INFINITY;
      bj[a] = wave * per_wave + m;
    }
    f32x4 bcur[RVQ_NT], bnxt[RVQ_NT];
    load(bcur, 0);
    for (int grp = 0; grp < groups; ++grp) {
      f32x4 acc[RVQ_NT];
#pragma unroll
      for (int t = 0; t < RVQ_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int q = grp * 8 + i;
        load(bnxt, q + 1 < steps ? q + 1 : q);     // the last step loads itself again: in bounds, never used
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int t = 0; t < RVQ_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(r[i][c], bcur[t][c], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < RVQ_NT; ++t) bcur[t] = bnxt[t];
      }
      // acc[t][a] = r[frame 4 g + a] . e[codeword j]; score 2 r.e - |e|^2, tiles in ascending j so `>` keeps the lowest index
#pragma unroll
      for (int t = 0; t < RVQ_NT; ++t) {
        const int32_t j = wave * per_wave + grp * RVQ_GROUP + 16 * t + m;
        const float n2 = en[j];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float sv = fmaf(2.f, acc[t][a], -n2);
          if (sv > bv[a]) {
            bv[a] = sv;
            bj[a] = j;
          }
        }
      }
    }
    // over the 16 lanes of the row (they hold the 16 columns of every tile)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv[a], o, 64);
        const int32_t oj = __shfl_xor(bj[a], o, 64);
        take_better(bv[a], bj[a], ov, oj);
      }
    }
    best_t(*buf)[RVQ_FRAMES] = red[s & 1];
    if (m == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a) buf[wave][4 * g + a] = best_t{bv[a], bj[a]};
    }
    __syncthreads();
    // over the waves, for the frame whose residual this lane holds
    best_t w = buf[0][m];
#pragma unroll
    for (int k = 1; k < RVQ_WAVES; ++k) take_better(w.v, w.j, buf[k][m].v, buf[k][m].j);
    if (wave == 0 && g == 0 && live) codes[(int64_t)s * F + f] = w.j;
    // residual - quantized: one fp32 subtraction per element, as the library's `residual = residual - quantized`
    const float* ej = e + (int64_t)w.j * RVQ_D + 4 * g;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(ej + 16 * i);
      r[i] = live ? r[i] - q : r[i];
    }
  }
}

// thread -> (frame, channel): channel fastest when the output's channel stride is 1, frame fastest otherwise
__global__ __launch_bounds__(256) void rvq_decode_kernel(const int64_t* __restrict__ codes, int32_t n_q, int32_t T, int64_t F,
                                                         const float* __restrict__ cb, int32_t Kc, float* __restrict__ out, int64_t sb,
                                                         int64_t st, int64_t sc, int32_t frame_fast) {
  int64_t f;
  int c;
  if (frame_fast) {                                // 256 consecutive frames of one channel per block
    const int64_t blocks_per_c = (F + 255) / 256;
    c = (int)(blockIdx.x / blocks_per_c);
    f = (blockIdx.x % blocks_per_c) * 256 + threadIdx.x;
  } else {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    f = gid / RVQ_D;
    c = (int)(gid % RVQ_D);
  }
  if (f >= F) return;
  float a = 0.f;
  for (int s = 0; s < n_q; ++s) {
    int64_t j = codes[(int64_t)s * F + f];
    j = j < 0 ? 0 : (j >= Kc ? Kc - 1 : j);        // the caller has checked the range; no index leaves the codebook here either way
    a += cb[((int64_t)s * Kc + j) * RVQ_D + c];
  }
  out[(f / T) * sb + (f % T) * st + c * sc] = a;
}

}  // namespace

extern "C" int v2a_encodec_rvq_encode(const float* x, int64_t batch_stride, int64_t frame_stride, int64_t chan_stride, int32_t B, int32_t T,
                                      const float* codebooks, const float* norms, int32_t S, int32_t Kc, int32_t D, int32_t n_q,
                                      int64_t* codes, v2a_stream_t stream) {
  V2A_REQUIRE(x && codebooks && norms && codes, "v2a_encodec_rvq_encode: null pointer");
  V2A_REQUIRE(D == RVQ_D && Kc >= RVQ_WAVES * RVQ_GROUP && Kc % (RVQ_WAVES * RVQ_GROUP) == 0 && Kc <= (1 << 20),
              "v2a_encodec_rvq_encode: D=%d Kc=%d (D = %d, Kc a multiple of %d)", D, Kc, RVQ_D, RVQ_WAVES * RVQ_GROUP);
  V2A_REQUIRE(S >= 1 && n_q >= 1 && n_q <= S, "v2a_encodec_rvq_encode: n_q=%d of S=%d stages", n_q, S);
  V2A_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= ((int64_t)1 << 30), "v2a_encodec_rvq_encode: B=%d T=%d", B, T);
  V2A_REQUIRE(batch_stride >= 0 && frame_stride >= 0 && chan_stride >= 0, "v2a_encodec_rvq_encode: negative stride");
  V2A_REQUIRE(((uintptr_t)codebooks & 15) == 0 && (((uintptr_t)x | (uintptr_t)norms) & 3) == 0 && ((uintptr_t)codes & 7) == 0,
              "v2a_encodec_rvq_encode: alignment (16 bytes for codebooks)");
  const int64_t F = (int64_t)B * T;
  hipLaunchKernelGGL(rvq_encode_kernel, dim3((unsigned)((F + RVQ_FRAMES - 1) / RVQ_FRAMES)), dim3(64 * RVQ_WAVES), 0, (hipStream_t)stream, x,
                     batch_stride, frame_stride, chan_stride, T, F, codebooks, norms, Kc, n_q, codes);
  return v2a_check_launch("v2a_encodec_rvq_encode");
}

extern "C" int v2a_encodec_rvq_decode(const int64_t* codes, int32_t n_q, int32_t B, int32_t T, const float* codebooks, int32_t S, int32_t Kc,
                                      int32_t D, float* out, int64_t batch_stride, int64_t frame_stride, int64_t chan_stride,
                                      v2a_stream_t stream) {
  V2A_REQUIRE(codes && codebooks && out, "v2a_encodec_rvq_decode: null pointer");
  V2A_REQUIRE(D == RVQ_D && Kc >= 1 && Kc <= (1 << 20), "v2a_encodec_rvq_decode: D=%d Kc=%d (D = %d)", D, Kc, RVQ_D);
  V2A_REQUIRE(S >= 1 && n_q >= 1 && n_q <= S, "v2a_encodec_rvq_decode: n_q=%d of S=%d stages", n_q, S);
  V2A_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T <= ((int64_t)1 << 30), "v2a_encodec_rvq_decode: B=%d T=%d", B, T);
  V2A_REQUIRE(batch_stride >= 0 && frame_stride >= 0 && chan_stride >= 0, "v2a_encodec_rvq_decode: negative stride");
  V2A_REQUIRE((((uintptr_t)codebooks | (uintptr_t)out) & 3) == 0 && ((uintptr_t)codes & 7) == 0, "v2a_encodec_rvq_decode: alignment");
  const int64_t F = (int64_t)B * T;
  const int frame_fast = chan_stride != 1;
  const int64_t blocks = frame_fast ? ((F + 255) / 256) * RVQ_D : (F * RVQ_D + 255) / 256;
  hipLaunchKernelGGL(rvq_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, codes, n_q, T, F, codebooks, Kc, out,
                     batch_stride, frame_stride, chan_stride, frame_fast);
  return v2a_check_launch("v2a_encodec_rvq_decode");
}
