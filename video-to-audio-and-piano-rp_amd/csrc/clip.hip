// CLIP ViT image encoder kernels for gfx950 (transformers CLIPVisionModelWithProjection behind CLIPImageProcessor, the reference's
// video_encoder = "clip_vit", x3:1423-1425, 1714, 1733-1735):
//   v2a_clip_resize_h     Pillow BICUBIC resize, horizontal pass: 22-bit fixed-point integer sums, uint8 clipped intermediate
//   v2a_clip_resize_v     vertical pass + centre crop + rescale / normalise (host table) -> the patch matrix of the patch convolution
//   v2a_clip_embed_init   class / position embedding rows of the residual stream (the patch GEMM adds onto them)
//   v2a_clip_layernorm    nn.LayerNorm (pre_layrnorm, layer_norm1/2, post_layernorm), fp32 or split-plane output, any row stride
//   v2a_clip_attention    bidirectional unmasked softmax attention, head dim <= 112, fp32 VALU with an online softmax
// The Linears run on v2a_gemm (fp32 MFMA or split-bf16 operands; fc1 with the GELU epilogue).
#include "v2a_common.h"

#include <math.h>

namespace {

// ---- Pillow resample, horizontal pass ---------------------------------------------------------
// tmp[f][y - y0][x][c] = clip8((2^21 + sum_i in[f][y][xmin(x) + i][c] * k[x][i]) >> 22) for the crop columns x < S and the input
// rows y0 <= y < y1 the vertical pass reads.  One thread per (row, column, channel).
__global__ __launch_bounds__(256) void clip_resize_h_kernel(const uint8_t* __restrict__ in, int64_t frames, int H, int W, uint8_t* __restrict__ tmp,
                                                            int y0, int rows, int S, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ coef, int ksize) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = frames * rows * S * 3;
  if (idx >= total) return;
  const int c = (int)(idx % 3);
  const int x = (int)((idx / 3) % S);
  const int64_t fy = idx / (3 * S);
  const int y = (int)(fy % rows) + y0;
  const int64_t f = fy / rows;
  const int xmin = bounds[2 * x], xs = bounds[2 * x + 1];
  const uint8_t* src = in + ((f * H + y) * (int64_t)W + xmin) * 3 + c;
  const int32_t* k = coef + (int64_t)x * ksize;
  int32_t ss = 1 << 21;
  for (int i = 0; i < xs; ++i) ss += (int32_t)src[3 * i] * k[i];
  ss >>= 22;
  tmp[idx] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
}

// ---- vertical pass + crop + normalise + patch matrix ----------------------------------------------
// Crop pixel (y, x) of frame f: u = clip8 of the vertical sum over tmp rows, v = lut[c][u] ((u / 255 - mean_c) / std_c, exactly as the
// processor rounds it, computed on the host).  It lands in row f * T + 1 + (y / P) * (S / P) + x / P of the patch matrix, column
// c * P * P + (y % P) * P + x % P (the Conv2d weight's own order); rows f * T (the class slot) and columns >= 3 P^2 are never written.
__global__ __launch_bounds__(256) void clip_resize_v_kernel(const uint8_t* __restrict__ tmp, int64_t frames, int rows, int S, int P,
                                                            const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef, int ksize,
                                                            const float* __restrict__ lut, void* __restrict__ patches, int64_t ldp,
                                                            int split, int64_t lo_offset, uint8_t* __restrict__ crop) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = frames * S * S * 3;
  if (idx >= total) return;
  const int c = (int)(idx % 3);
  const int x = (int)((idx / 3) % S);
  const int y = (int)((idx / (3 * S)) % S);
  const int64_t f = idx / (3 * S * S);
  const int ymin = bounds[2 * y], ys = bounds[2 * y + 1];
  const uint8_t* src = tmp + ((f * rows + ymin) * (int64_t)S + x) * 3 + c;
  const int32_t* k = coef + (int64_t)y * ksize;
  int32_t ss = 1 << 21;
  for (int i = 0; i < ys; ++i) ss += (int32_t)src[(int64_t)i * S * 3] * k[i];
  ss >>= 22;
  const int u = ss < 0 ? 0 : (ss > 255 ? 255 : ss);
  if (crop) crop[idx] = (uint8_t)u;
  const float v = lut[c * 256 + u];
  const int g = S / P;
  const int64_t row = f * (1 + g * g) + 1 + (y / P) * g + x / P;
  const int64_t col = c * P * P + (y % P) * P + x % P;
  if (split) {
    bf16_t* o = reinterpret_cast<bf16_t*>(patches) + row * ldp + col;
    const bf16_t hi = (bf16_t)v;
    o[0] = hi;
    o[lo_offset] = (bf16_t)(v - (float)hi);
  } else {
    reinterpret_cast<float*>(patches)[row * ldp + col] = v;
  }
}

// ---- embeddings ------------------------------------------------------------------------------------
// h[f * T + t][c] = pos[t][c] + (t == 0 ? cls[c] : 0); the patch GEMM (RESID epilogue, zero A row for t = 0) then adds the patches
__global__ __launch_bounds__(256) void clip_embed_init_kernel(float* __restrict__ h, int64_t ldh, int64_t rows, int T, int d,
                                                              const float* __restrict__ cls, const float* __restrict__ pos) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d4 = d >> 2;
  if (idx >= rows * d4) return;
  const int c4 = (int)(idx % d4);
  const int64_t r = idx / d4;
  const int t = (int)(r % T);
  f32x4 v = reinterpret_cast<const f32x4*>(pos + (int64_t)t * d)[c4];
  if (t == 0) v += reinterpret_cast<const f32x4*>(cls)[c4];
  reinterpret_cast<f32x4*>(h + r * ldh)[c4] = v;
}

// ---- LayerNorm -----------------------------------------------------------------------------------------
// One workgroup of 256 threads per row; the row stays in registers (d <= 4096: four float4 per thread), mean first, then the
// centred sum of squares (rows with |h| ~ 1e2 outlier channels keep their variance), y = (x - mean) * rsqrt(var + eps) * g + b.
constexpr int LN_V = 4;

__device__ __forceinline__ float block_sum256(float v, float* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void clip_layernorm_kernel(const float* __restrict__ x, int64_t ldx, void* __restrict__ y, int64_t ldy,
                                                             int split, int d, const float* __restrict__ g, const float* __restrict__ b,
                                                             float eps) {
  __shared__ float part[4];
  const int64_t row = blockIdx.x;
  const float* xr = x + row * ldx;
  const int d4 = d >> 2;
  f32x4 v[LN_V];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const int c = threadIdx.x + i * 256;
    v[i] = c < d4 ? reinterpret_cast<const f32x4*>(xr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = block_sum256(s, part) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c < d4) {
      const f32x4 e = v[i] - mean;
      q += (e.x * e.x + e.y * e.y) + (e.z * e.z + e.w * e.w);
    }
  }
  const float r = 1.0f / sqrtf(block_sum256(q, part) / (float)d + eps);
#pragma unroll
  for (int i = 0; i < LN_V; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c >= d4) continue;
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[c], bb = reinterpret_cast<const f32x4*>(b)[c];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaf((v[i][e] - mean) * r, gg[e], bb[e]);
    if (split) {
      bf16_t* yr = reinterpret_cast<bf16_t*>(y) + row * ldy + 4 * c;
      bf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hi[e] = (bf16_t)o[e];
        lo[e] = (bf16_t)(o[e] - (float)hi[e]);
      }
      *reinterpret_cast<bf16x4*>(yr) = hi;
      *reinterpret_cast<bf16x4*>(yr + (ldy >> 1)) = lo;       // lo plane: the second half of the row
    } else {
      reinterpret_cast<f32x4*>(reinterpret_cast<float*>(y) + row * ldy)[c] = o;
    }
  }
}

// ---- attention ------------------------------------------------------------------------------------------
// Workgroup = 4 waves = 64 queries of one (frame, head); a query is owned by 4 adjacent lanes, lane s holding dims [28 s, 28 s + 28) of
// q and of the output (head dims padded to 112 = 4 x 7 float4: 104 is no multiple of 16; the pad dims read as zero and are never
// stored).  Keys and values stream through LDS in blocks of 32 rows; per block the scores are formed, the running max and sum are
// rescaled once and the probabilities are applied to V (fp32 FMA throughout: exact-fp32 grade in both compute modes).
constexpr int CA_KB = 32;
constexpr int CA_DP = 112;
constexpr int CA_V4 = CA_DP / 16;     // float4 per lane

__device__ __forceinline__ float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // [2,3,0,1]
  return v;
}

__global__ __launch_bounds__(256) void clip_attention_kernel(v2a_clip_attn_args a) {
  __shared__ __attribute__((aligned(16))) float ks[CA_KB][CA_DP];
  __shared__ __attribute__((aligned(16))) float vs[CA_KB][CA_DP];
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x;
  const int s = tid & 3;
  const int N = a.N, D = a.d_head;
  const int qi = blockIdx.x * 64 + (tid >> 2);
  const int qrow = qi < N ? qi : N - 1;
  const float* qp = a.q + (int64_t)b * a.batch_stride + (int64_t)qrow * a.row_stride + h * D + s * 28;
  f32x4 q[CA_V4], o[CA_V4];
#pragma unroll
  for (int t = 0; t < CA_V4; ++t) {
    q[t] = (s * 28 + 4 * t < D) ? reinterpret_cast<const f32x4*>(qp)[t] : f32x4{0.f, 0.f, 0.f, 0.f};
    o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = a.scale * 1.4426950408889634f;     // softmax in base 2: exp(x) = exp2(x log2 e)
  const float* kb = a.k + (int64_t)b * a.batch_stride + h * D;
  const float* vb = a.v + (int64_t)b * a.batch_stride + h * D;
  const int D4 = D >> 2;
  float mx = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < N; j0 += CA_KB) {
    __syncthreads();
    // stage 64 rows x 28 float4 of K and of V (7 + 7 per thread), zero past the head and past the last key
    for (int e = tid; e < CA_KB * (CA_DP / 4); e += 256) {
      const int kr = e / (CA_DP / 4), c4 = e % (CA_DP / 4);
      const int j = j0 + kr;
      f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (j < N && c4 < D4) {
        kv = reinterpret_cast<const f32x4*>(kb + (int64_t)j * a.row_stride)[c4];
        vv = reinterpret_cast<const f32x4*>(vb + (int64_t)j * a.row_stride)[c4];
      }
      reinterpret_cast<f32x4*>(&ks[kr][0])[c4] = kv;
      reinterpret_cast<f32x4*>(&vs[kr][0])[c4] = vv;
    }
    __syncthreads();
    const int nk = min(CA_KB, N - j0);
    float sc[CA_KB];
    float bm = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < CA_KB; ++jj) {
      float v = -INFINITY;
      if (jj < nk) {
        const f32x4* kr = reinterpret_cast<const f32x4*>(&ks[jj][s * 28]);
        float p = 0.f;
#pragma unroll
        for (int t = 0; t < CA_V4; ++t) {
          const f32x4 kk = kr[t];
          p = fmaf(q[t].x, kk.x, p);
          p = fmaf(q[t].y, kk.y, p);
          p = fmaf(q[t].z, kk.z, p);
          p = fmaf(q[t].w, kk.w, p);
        }
        v = quad_sum(p) * sl2;
      }
      sc[jj] = v;
      bm = fmaxf(bm, v);
    }
    const float mn = fmaxf(mx, bm);
    const float corr = exp2f(mx - mn);                 // mx = -inf on the first block: corr = 0
    mx = mn;
    l *= corr;
#pragma unroll
    for (int t = 0; t < CA_V4; ++t) o[t] *= corr;
#pragma unroll
    for (int jj = 0; jj < CA_KB; ++jj) {
      const float p = exp2f(sc[jj] - mn);               // exp2(-inf) = 0 past the last key
      l += p;
      const f32x4* vr = reinterpret_cast<const f32x4*>(&vs[jj][s * 28]);
#pragma unroll
      for (int t = 0; t < CA_V4; ++t) {
        const f32x4 vv = vr[t];
        o[t].x = fmaf(p, vv.x, o[t].x);
        o[t].y = fmaf(p, vv.y, o[t].y);
        o[t].z = fmaf(p, vv.z, o[t].z);
        o[t].w = fmaf(p, vv.w, o[t].w);
      }
    }
  }
  if (qi >= N) return;
  const float inv = 1.0f / l;
  const int64_t orow = (int64_t)b * a.out_batch_stride + (int64_t)qi * a.out_row_stride;
  const int c0 = h * D + s * 28;
#pragma unroll
  for (int t = 0; t < CA_V4; ++t) {
    if (s * 28 + 4 * t >= D) continue;
    const f32x4 r = o[t] * inv;
    if (a.out_split) {
      bf16_t* op = reinterpret_cast<bf16_t*>(a.out) + orow + c0 + 4 * t;
      bf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hi[e] = (bf16_t)r[e];
        lo[e] = (bf16_t)(r[e] - (float)hi[e]);
      }
      *reinterpret_cast<bf16x4*>(op) = hi;
      *reinterpret_cast<bf16x4*>(op + (a.out_row_stride >> 1)) = lo;   // lo plane: the second half of the row
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + orow + c0 + 4 * t) = r;
    }
  }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int v2a_clip_resize_h(const uint8_t* frames, int32_t F, int32_t H, int32_t W, uint8_t* tmp, int32_t y0, int32_t rows, int32_t S,
                                 const int32_t* bounds, const int32_t* coef, int32_t ksize, v2a_stream_t stream) {
  V2A_REQUIRE(frames && tmp && bounds && coef, "v2a_clip_resize_h: null pointer");
  V2A_REQUIRE(F > 0 && H > 0 && W > 0 && S > 0 && ksize > 0 && rows > 0 && y0 >= 0 && y0 + rows <= H,
              "v2a_clip_resize_h: F=%d H=%d W=%d S=%d rows [%d, %d) ksize=%d", F, H, W, S, y0, y0 + rows, ksize);
  const int64_t n = (int64_t)F * rows * S * 3;
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, frames, (int64_t)F, H, W, tmp, y0, rows, S,
                     bounds, coef, ksize);
  return v2a_check_launch("v2a_clip_resize_h");
}

extern "C" int v2a_clip_resize_v(const uint8_t* tmp, int32_t F, int32_t rows, int32_t S, int32_t P, const int32_t* bounds, const int32_t* coef,
                                 int32_t ksize, const float* lut, void* patches, int64_t ldp, int32_t out_dtype, int64_t lo_offset,
                                 uint8_t* crop, v2a_stream_t stream) {
  V2A_REQUIRE(tmp && bounds && coef && lut && patches, "v2a_clip_resize_v: null pointer");
  V2A_REQUIRE(F > 0 && rows > 0 && S > 0 && P > 0 && S % P == 0 && ksize > 0, "v2a_clip_resize_v: F=%d rows=%d S=%d P=%d", F, rows, S, P);
  V2A_REQUIRE(out_dtype == V2A_F32 || out_dtype == V2A_BF16_SPLIT, "v2a_clip_resize_v: out_dtype %d (V2A_F32 or V2A_BF16_SPLIT)", out_dtype);
  V2A_REQUIRE(ldp >= 3 * P * P, "v2a_clip_resize_v: ldp %lld < 3 P^2", (long long)ldp);
  if (out_dtype == V2A_BF16_SPLIT)
    V2A_REQUIRE(lo_offset >= 3 * P * P && ldp >= lo_offset + 3 * P * P, "v2a_clip_resize_v: split rows need lo_offset >= 3 P^2 and ldp >= lo_offset + 3 P^2");
  const int64_t n = (int64_t)F * S * S * 3;
  hipLaunchKernelGGL(clip_resize_v_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, tmp, (int64_t)F, rows, S, P, bounds, coef, ksize,
                     lut, patches, ldp, out_dtype == V2A_BF16_SPLIT ? 1 : 0, lo_offset, crop);
  return v2a_check_launch("v2a_clip_resize_v");
}

extern "C" int v2a_clip_embed_init(float* h, int64_t ldh, int64_t rows, int32_t T, int32_t d, const float* cls, const float* pos,
                                   v2a_stream_t stream) {
  V2A_REQUIRE(h && cls && pos, "v2a_clip_embed_init: null pointer");
  V2A_REQUIRE(rows > 0 && T > 0 && d > 0 && d % 4 == 0 && ldh % 4 == 0 && ((uintptr_t)h & 15) == 0 && ((uintptr_t)cls & 15) == 0 &&
                  ((uintptr_t)pos & 15) == 0,
              "v2a_clip_embed_init: d=%d ldh=%lld need multiples of 4 and 16-byte aligned rows", d, (long long)ldh);
  const int64_t n = rows * (d / 4);
  hipLaunchKernelGGL(clip_embed_init_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, h, ldh, rows, T, d, cls, pos);
  return v2a_check_launch("v2a_clip_embed_init");
}

extern "C" int v2a_clip_layernorm(const float* x, int64_t ldx, void* y, int64_t ldy, int32_t y_dtype, int64_t rows, int32_t d, const float* gamma,
                                  const float* beta, float eps, v2a_stream_t stream) {
  V2A_REQUIRE(x && y && gamma && beta, "v2a_clip_layernorm: null pointer");
  V2A_REQUIRE(y_dtype == V2A_F32 || y_dtype == V2A_BF16_SPLIT, "v2a_clip_layernorm: y_dtype %d (V2A_F32 or V2A_BF16_SPLIT)", y_dtype);
  V2A_REQUIRE(rows > 0 && d > 0 && d % 4 == 0 && d <= 1024 * LN_V && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)gamma & 15) == 0 &&
                  ((uintptr_t)beta & 15) == 0,
              "v2a_clip_layernorm: d=%d (a multiple of 4, <= 4096), 16-byte aligned rows", d);
  if (y_dtype == V2A_F32) V2A_REQUIRE(ldy >= d && ldy % 4 == 0 && ((uintptr_t)y & 15) == 0, "v2a_clip_layernorm: fp32 output rows");
  else V2A_REQUIRE(ldy >= 2 * (int64_t)d && ldy % 4 == 0 && ((uintptr_t)y & 7) == 0, "v2a_clip_layernorm: split output rows hold 2d bf16");
  hipLaunchKernelGGL(clip_layernorm_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, y_dtype == V2A_BF16_SPLIT ? 1 : 0,
                     d, gamma, beta, eps);
  return v2a_check_launch("v2a_clip_layernorm");
}

extern "C" int v2a_clip_attention(const v2a_clip_attn_args* a, v2a_stream_t stream) {
  V2A_REQUIRE(a && a->q && a->k && a->v && a->out, "v2a_clip_attention: null pointer");
  V2A_REQUIRE(a->B > 0 && a->H > 0 && a->N > 0 && a->N <= 4096 && a->d_head > 0 && a->d_head <= CA_DP && a->d_head % 4 == 0,
              "v2a_clip_attention: B=%d H=%d N=%d d_head=%d (d_head a multiple of 4, <= %d)", a->B, a->H, a->N, a->d_head, CA_DP);
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  V2A_REQUIRE(al16(a->q) && al16(a->k) && al16(a->v) && a->row_stride % 4 == 0 && a->batch_stride % 4 == 0,
              "v2a_clip_attention: q / k / v need 16-byte aligned rows");
  if (a->out_split)
    V2A_REQUIRE(((uintptr_t)a->out & 7) == 0 && a->out_row_stride >= 2 * (int64_t)a->H * a->d_head && a->out_row_stride % 4 == 0 &&
                    a->out_batch_stride % 4 == 0,
                "v2a_clip_attention: split output rows hold 2 * H * d_head bf16, 8-byte aligned");
  else
    V2A_REQUIRE(al16(a->out) && a->out_row_stride >= (int64_t)a->H * a->d_head && a->out_row_stride % 4 == 0 && a->out_batch_stride % 4 == 0,
                "v2a_clip_attention: fp32 output rows, 16-byte aligned");
  hipLaunchKernelGGL(clip_attention_kernel, dim3((a->N + 63) / 64, a->H, a->B), dim3(256), 0, (hipStream_t)stream, *a);
  return v2a_check_launch("v2a_clip_attention");
}
