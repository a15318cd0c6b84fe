// FLAN-T5 encoder kernels for gfx950 (transformers T5EncoderModel arithmetic, fp32 throughout):
//   v2a_t5_rmsnorm       T5LayerNorm  y = w * x * rsqrt(mean(x^2) + eps), optionally gathering x from the embedding table
//   v2a_t5_attention     unscaled q.k^T + relative-position bias, key mask, fp32 online softmax, p.v (VALU FMA)
//   v2a_gemm_skinny_f32  exact-fp32 MFMA GEMM for few rows: the weight stream spread over N-column workgroups whose waves split K,
//                        partial sums reduced through LDS in a fixed order (same bits on every run, for every M)
#include "v2a_common.h"

#include <math.h>

namespace {

// ---- T5LayerNorm -------------------------------------------------------------------------
// One workgroup of 256 threads per row, float4 lanes.  With ids the row is gathered from the embedding table (ids clamped to
// [0, vocab): the host validates them, the clamp only keeps a bad id from reading outside the table) and written to resid.
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ ids,
                                                         int32_t vocab, float* __restrict__ resid, int64_t ldr, float* __restrict__ y,
                                                         int64_t ldy, int32_t d, const float* __restrict__ w, float eps) {
  const int64_t row = blockIdx.x;
  const float* xr;
  if (ids) {
    int32_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    xr = x + (int64_t)id * ldx;
  } else {
    xr = x + row * ldx;
  }
  const int d4 = d >> 2;
  float ss = 0.f;
  for (int c = threadIdx.x; c < d4; c += 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(xr)[c];
    if (ids) reinterpret_cast<f32x4*>(resid + row * ldr)[c] = v;
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  __shared__ float part[4];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float tot = (part[0] + part[1]) + (part[2] + part[3]);
  const float r = 1.0f / sqrtf(tot / (float)d + eps);
  for (int c = threadIdx.x; c < d4; c += 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(xr)[c];
    const f32x4 g = reinterpret_cast<const f32x4*>(w)[c];
    f32x4 o;
    o.x = g.x * (v.x * r);
    o.y = g.y * (v.y * r);
    o.z = g.z * (v.z * r);
    o.w = g.w * (v.w * r);
    reinterpret_cast<f32x4*>(y + row * ldy)[c] = o;
  }
}

// ---- T5Attention core ---------------------------------------------------------------------
// Workgroup = 4 waves = 64 queries of one (batch, head); a query is owned by 4 adjacent lanes, lane s of the group holding
// dims [16 s, 16 s + 16) of q and of the output.  Keys / values stream through LDS in blocks of 64 rows; per block the scores
// are formed, the running max and sum are rescaled once, and the probabilities are applied to V.
constexpr int T5_KB = 64;

__device__ __forceinline__ float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // [2,3,0,1]
  return v;
}

__global__ __launch_bounds__(256) void t5_attention_kernel(v2a_t5_attn_args a) {
  __shared__ __attribute__((aligned(16))) float ks[T5_KB][64];
  __shared__ __attribute__((aligned(16))) float vs[T5_KB][64];
  __shared__ int32_t km[T5_KB];
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x;
  const int s = tid & 3;
  const int qi = blockIdx.x * 64 + (tid >> 2);
  const int N = a.N;
  const int qrow = qi < N ? qi : N - 1;
  const float* qp = a.q + (int64_t)b * a.q_batch_stride + (int64_t)qrow * a.q_row_stride + h * 64 + s * 16;
  f32x4 q[4], o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    q[t] = reinterpret_cast<const f32x4*>(qp)[t];
    o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float* brow = a.bias + (int64_t)h * (2 * N - 1) + (N - 1) - qrow;      // brow[j] = bias[h][j - i + N - 1]
  const int32_t* mrow = a.key_mask + (int64_t)b * N;
  const float* kb = a.k + (int64_t)b * a.k_batch_stride + h * 64;
  const float* vb = a.v + (int64_t)b * a.v_batch_stride + h * 64;
  float mx = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < N; j0 += T5_KB) {
    __syncthreads();
    // stage: 64 rows x 16 float4 of K and of V, 4 + 4 per thread
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = tid + r * 256, kr = e >> 4, c4 = e & 15;
      const int j = j0 + kr;
      f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (j < N) {
        kv = reinterpret_cast<const f32x4*>(kb + (int64_t)j * a.k_row_stride)[c4];
        vv = reinterpret_cast<const f32x4*>(vb + (int64_t)j * a.v_row_stride)[c4];
      }
      reinterpret_cast<f32x4*>(&ks[kr][0])[c4] = kv;
      reinterpret_cast<f32x4*>(&vs[kr][0])[c4] = vv;
    }
    if (tid < T5_KB) km[tid] = (j0 + tid < N) ? mrow[j0 + tid] : 0;
    __syncthreads();
    const int nk = min(T5_KB, N - j0);
    float sc[T5_KB];
    float bm = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < T5_KB; ++jj) {
      float v = -INFINITY;
      if (jj < nk) {
        const f32x4* kr = reinterpret_cast<const f32x4*>(&ks[jj][s * 16]);
        float p = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 kk = kr[t];
          p = fmaf(q[t].x, kk.x, p);
          p = fmaf(q[t].y, kk.y, p);
          p = fmaf(q[t].z, kk.z, p);
          p = fmaf(q[t].w, kk.w, p);
        }
        p = quad_sum(p);
        if (km[jj]) v = p + brow[j0 + jj];
      }
      sc[jj] = v;
      bm = fmaxf(bm, v);
    }
    if (bm == -INFINITY) continue;                     // every key of this block masked
    const float mn = fmaxf(mx, bm);
    const float corr = expf(mx - mn);                  // mx = -inf on the first live block: corr = 0
    mx = mn;
    l *= corr;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] *= corr;
#pragma unroll
    for (int jj = 0; jj < T5_KB; ++jj) {
      if (sc[jj] == -INFINITY) continue;
      const float p = expf(sc[jj] - mn);
      l += p;
      const f32x4* vr = reinterpret_cast<const f32x4*>(&vs[jj][s * 16]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 vv = vr[t];
        o[t].x = fmaf(p, vv.x, o[t].x);
        o[t].y = fmaf(p, vv.y, o[t].y);
        o[t].z = fmaf(p, vv.z, o[t].z);
        o[t].w = fmaf(p, vv.w, o[t].w);
      }
    }
  }
  if (qi >= N) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  float* op = a.out + (int64_t)b * a.out_batch_stride + (int64_t)qi * a.out_row_stride + h * 64 + s * 16;
#pragma unroll
  for (int t = 0; t < 4; ++t) reinterpret_cast<f32x4*>(op)[t] = o[t] * inv;
}

// ---- skinny exact-fp32 GEMM -------------------------------------------------------------------
// Workgroup = NW waves over a BM x (16 * NT) output tile (NT = 2 for GEGLU_TANH: the value and gate rows of 16 outputs).  Wave w
// walks K steps [w * S / NW, (w + 1) * S / NW) of 32; a lane reads 8 consecutive K of its A / W rows (two float4, whole 128-B lines
// per row across the lane quad) and feeds them to 8 v_mfma_f32_16x16x4_f32 with the K index permuted identically in both operands.
// The NW partial tiles meet in LDS and are summed in wave order: the result depends on K and NW only, never on M or on timing.
constexpr int SK_NW = 8;
constexpr int SK_KS = 32;

__device__ __forceinline__ float gelu_new_f(float x) {
  return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}

template <int MT, int NT, int EPI>
__global__ __launch_bounds__(SK_NW * 64) void gemm_skinny_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ W,
                                                                 int64_t ldw, const float* __restrict__ bias, float* out, int64_t ldo,
                                                                 const float* resid, int64_t ldr, int M, int N, int K) {
  constexpr int R = MT * NT * 4;                      // accumulator floats per lane
  __shared__ float red[SK_NW][R][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.y * (MT * 16);
  const int n0 = blockIdx.x * (NT * 16);              // packed W row / output column base
  const float* ap[MT];
  const float* wp[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = min(m0 + i * 16 + lr, M - 1);
    ap[i] = A + (int64_t)m * lda + lq * 8;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) wp[j] = W + (int64_t)(n0 + j * 16 + lr) * ldw + lq * 8;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int S = K / SK_KS;
  const int s0 = (int)((int64_t)wave * S / SK_NW), s1 = (int)((int64_t)(wave + 1) * S / SK_NW);
  f32x4 af[MT][2], wf[NT][2];
  auto load = [&](int st) {
    const int k = st * SK_KS;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      af[i][0] = *reinterpret_cast<const f32x4*>(ap[i] + k);
      af[i][1] = *reinterpret_cast<const f32x4*>(ap[i] + k + 4);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      wf[j][0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wp[j] + k));
      wf[j][1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wp[j] + k + 4));
    }
  };
  if (s0 < s1) load(s0);
  for (int st = s0; st < s1; ++st) {
    f32x4 ac[MT][2], wc[NT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i) { ac[i][0] = af[i][0]; ac[i][1] = af[i][1]; }
#pragma unroll
    for (int j = 0; j < NT; ++j) { wc[j][0] = wf[j][0]; wc[j][1] = wf[j][1]; }
    if (st + 1 < s1) load(st + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i][h][e], wc[j][h][e], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][(i * NT + j) * 4 + r][lane] = acc[i][j][r];
  __syncthreads();
  // epilogue: one output (row, column) per iteration; D layout col = lane & 15, row = (lane >> 4) * 4 + r
  constexpr int OUTS = MT * 4 * 64;                   // outputs of the 16 columns of the tile
  for (int e = tid; e < OUTS; e += SK_NW * 64) {
    const int ln = e & 63, ir = e >> 6, i = ir >> 2, r = ir & 3;
    const int m = m0 + i * 16 + (ln >> 4) * 4 + r;
    if (m >= M) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < SK_NW; ++w) v += red[w][(i * NT) * 4 + r][ln];
    if constexpr (EPI == V2A_EPI_GEGLU_TANH) {
      float g = 0.f;
#pragma unroll
      for (int w = 0; w < SK_NW; ++w) g += red[w][(i * NT + 1) * 4 + r][ln];
      const int n = n0 + (ln & 15);
      if (bias) { v += bias[n]; g += bias[n + 16]; }
      out[(int64_t)m * ldo + (n0 >> 1) + (ln & 15)] = v * gelu_new_f(g);
    } else {
      const int n = n0 + (ln & 15);
      if (bias) v += bias[n];
      if constexpr (EPI == V2A_EPI_RESID) v += resid[(int64_t)m * ldr + n];
      out[(int64_t)m * ldo + n] = v;
    }
  }
}

template <int MT, int NT, int EPI>
int launch_skinny(const v2a_gemm_args* a, hipStream_t s) {
  const int ncols = NT * 16;
  dim3 grid(a->N / ncols, (a->M + MT * 16 - 1) / (MT * 16));
  hipLaunchKernelGGL((gemm_skinny_kernel<MT, NT, EPI>), grid, dim3(SK_NW * 64), 0, s, (const float*)a->a[0], a->lda[0],
                     (const float*)a->w, a->ldw, a->bias, (float*)a->out, a->ldo, a->resid, a->ldr, a->M, a->N, a->ka[0]);
  return v2a_check_launch("v2a_gemm_skinny_f32");
}

template <int EPI, int NT>
int skinny_by_rows(const v2a_gemm_args* a, hipStream_t s) {
  if (a->M <= 16) return launch_skinny<1, NT, EPI>(a, s);
  if (a->M <= 32) return launch_skinny<2, NT, EPI>(a, s);
  return launch_skinny<4, NT, EPI>(a, s);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int v2a_t5_rmsnorm(const float* x, int64_t ldx, const int32_t* ids, int32_t vocab, float* resid, int64_t ldr, float* y,
                              int64_t ldy, int64_t rows, int32_t d, const float* w, float eps, v2a_stream_t stream) {
  V2A_REQUIRE(x && y && w, "v2a_t5_rmsnorm: null pointer");
  V2A_REQUIRE(rows > 0 && rows <= (1 << 30) && d > 0 && d % 4 == 0, "v2a_t5_rmsnorm: rows %lld, d %d (d %% 4 == 0)", (long long)rows, d);
  V2A_REQUIRE(ldx >= d && ldy >= d && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && al16(w),
              "v2a_t5_rmsnorm: 16-byte aligned rows needed (ldx %lld, ldy %lld)", (long long)ldx, (long long)ldy);
  V2A_REQUIRE(eps >= 0.f, "v2a_t5_rmsnorm: eps %g", (double)eps);
  if (ids) {
    V2A_REQUIRE(resid && vocab > 0 && ldr >= d && ldr % 4 == 0 && al16(resid),
                "v2a_t5_rmsnorm: the gather needs vocab > 0 (%d) and a 16-byte aligned resid buffer", vocab);
  }
  hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, ldx, ids, vocab, resid, ldr, y, ldy, d,
                     w, eps);
  return v2a_check_launch("v2a_t5_rmsnorm");
}

extern "C" int v2a_t5_attention(const v2a_t5_attn_args* a, v2a_stream_t stream) {
  V2A_REQUIRE(a && a->q && a->k && a->v && a->out && a->bias && a->key_mask, "v2a_t5_attention: null pointer");
  V2A_REQUIRE(a->d_kv == 64, "v2a_t5_attention: d_kv %d (64 only)", a->d_kv);
  V2A_REQUIRE(a->B > 0 && a->H > 0 && a->B <= 65535 && a->H <= 65535 && a->N > 0 && a->N <= 512,
              "v2a_t5_attention: B %d, H %d, N %d (N <= 512)", a->B, a->H, a->N);
  V2A_REQUIRE(al16(a->q) && al16(a->k) && al16(a->v) && al16(a->out) && a->q_row_stride % 4 == 0 && a->k_row_stride % 4 == 0 &&
                  a->v_row_stride % 4 == 0 && a->out_row_stride % 4 == 0 && a->q_batch_stride % 4 == 0 && a->k_batch_stride % 4 == 0 &&
                  a->v_batch_stride % 4 == 0 && a->out_batch_stride % 4 == 0,
              "v2a_t5_attention: q / k / v / out need 16-byte aligned rows");
  dim3 grid((a->N + 63) / 64, a->H, a->B);
  hipLaunchKernelGGL(t5_attention_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a);
  return v2a_check_launch("v2a_t5_attention");
}

extern "C" int v2a_gemm_skinny_f32(const v2a_gemm_args* a, v2a_stream_t stream) {
  V2A_REQUIRE(a, "v2a_gemm_skinny_f32: null args");
  V2A_REQUIRE(a->nseg == 1 && a->a_dtype == V2A_F32 && a->compute_dtype == V2A_F32 && a->out_dtype == V2A_F32,
              "v2a_gemm_skinny_f32: one fp32 A segment, fp32 compute and output only (nseg %d, a_dtype %d, compute %d, out %d)", a->nseg,
              a->a_dtype, a->compute_dtype, a->out_dtype);
  V2A_REQUIRE(a->a[0] && a->w && a->out, "v2a_gemm_skinny_f32: null pointer");
  V2A_REQUIRE(!a->out_bf16 && !a->rope_table && !a->relu && !a->a_row_offset && !a->a_ktile_offset && !a->out_row_offset && !a->norm_gamma &&
                  !a->norm_ssq && !a->row_ssq && !a->out_bf16_split && !a->tile_hint,
              "v2a_gemm_skinny_f32: shadows, RoPE, ReLU, offset tables, folded norms and tile hints are not supported");
  const int K = a->ka[0];
  V2A_REQUIRE(a->M > 0 && a->M <= 16 * 512 && a->N > 0 && K > 0 && K % SK_KS == 0,
              "v2a_gemm_skinny_f32: M %d (1..8192), N %d, K %d (K %% 32 == 0)", a->M, a->N, K);
  V2A_REQUIRE(al16(a->a[0]) && al16(a->w) && a->lda[0] >= K && a->ldw >= K && a->lda[0] % 4 == 0 && a->ldw % 4 == 0,
              "v2a_gemm_skinny_f32: A and W need 16-byte aligned rows of at least K elements");
  hipStream_t s = (hipStream_t)stream;
  switch (a->epilogue) {
    case V2A_EPI_STORE:
      V2A_REQUIRE(a->N % 16 == 0 && a->ldo >= a->N, "v2a_gemm_skinny_f32: STORE needs N %% 16 == 0 (N=%d), ldo >= N", a->N);
      return skinny_by_rows<V2A_EPI_STORE, 1>(a, s);
    case V2A_EPI_RESID:
      V2A_REQUIRE(a->resid && a->N % 16 == 0 && a->ldo >= a->N && a->ldr >= a->N,
                  "v2a_gemm_skinny_f32: RESID needs resid, N %% 16 == 0 (N=%d), ldo / ldr >= N", a->N);
      return skinny_by_rows<V2A_EPI_RESID, 1>(a, s);
    case V2A_EPI_GEGLU_TANH:
      V2A_REQUIRE(a->N % 32 == 0 && a->ldo >= a->N / 2, "v2a_gemm_skinny_f32: GEGLU_TANH needs N %% 32 == 0 (N=%d), ldo >= N / 2", a->N);
      return skinny_by_rows<V2A_EPI_GEGLU_TANH, 2>(a, s);
  }
  return v2a_fail(V2A_ERR_ARG, "v2a_gemm_skinny_f32: unsupported epilogue %d (STORE, RESID, GEGLU_TANH)", a->epilogue);
}
