// The arithmetic that the MFMA attention kernels share (attn_mfma_kernel, attn_mfma_split_kernel, attn_mfma_f32_kernel in
// attention.hip, qproj_xattn_kernel in qproj_xattn.hip; the clamp / softmax step also xattn_absorbed_kernel in xattn_absorbed.hip), each piece defined once: the kernels differ in how an operand becomes an
// MFMA fragment, not in what happens between S^T = K Q^T and O^T += V^T P^T or after the key loop.  The one-launch cross attention
// promises the bits of the two-launch path; it keeps that promise by calling these functions, not by repeating their text.
//
// Common geometry (see attn_mfma_kernel): a wave owns 16 queries, the query sits on the lane (lr = lane & 15), g = lane >> 4;
// register j of s[t] is key j0 + 16 t + 4 g + j of the 64-key tile, register j of o[dt] is head dimension 16 dt + 4 g + j.
#pragma once
#include "v2a_common.h"
#include <type_traits>

// ---- operands ---------------------------------------------------------------------------
// hi | lo bf16 planes of eight fp32 values: hi = bf16(v), lo = bf16(v - hi)
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16_t ha = (bf16_t)a[e], hb = (bf16_t)b[e];
    hi[e] = ha;
    hi[4 + e] = hb;
    lo[e] = (bf16_t)(a[e] - (float)ha);
    lo[4 + e] = (bf16_t)(b[e] - (float)hb);
  }
}

// V^T fragment of O^T = V^T P^T for d tile dt and k-step ks2 (32 keys) from a row-major [key][64] bf16 plane whose 16-B chunks are
// XOR-swizzled by (key & 7), by the transposing LDS read (ds_read_b64_tr_b16): per 16-lane group a block of 4 keys x 16 head
// dimensions, lane 4q+p of the group supplies the address of (key q, dimensions 4p..4p+3), lane i receives dimension i of the 4
// keys.  Two reads 16 keys apart make the k-slot order (g, jj) <-> key 32 ks2 + 16 (jj / 4) + 4 g + jj % 4, which is the order
// in which attn_pack_weights lays P out.  EXEC is all ones wherever this is read.
__device__ __forceinline__ bf16x8 attn_vt_frag(const bf16_t* vs, int ks2, int dt, int g, int lr) {
  const int vq = lr >> 2, vp = lr & 3;
  bf16x4 half[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int key = 32 * ks2 + 16 * i + 4 * g + vq;
    const int chunk = 2 * dt + (vp >> 1);
    const bf16_t* ad = vs + key * 64 + ((chunk ^ (key & 7)) << 3) + 4 * (vp & 1);
    half[i] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)ad);
  }
  bf16x8 vf;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vf[j] = half[0][j];
    vf[4 + j] = half[1][j];
  }
  return vf;
}

// ---- logits -> weights ------------------------------------------------------------------
// zc: raw QK^T -> argument of the base-2 exponential (2x*log2e with x = scale*s/clamp), or -> log2 units without a clamp;
// c2 = clamp*log2e
struct AttnLogitScale {
  float zc, c2;
};
__device__ __forceinline__ AttnLogitScale attn_logit_scale(float scale, float clamp) {
  constexpr float LOG2E = 1.4426950408889634f;
  return {clamp > 0.f ? 2.0f * LOG2E * scale / clamp : scale * LOG2E, clamp * LOG2E};
}

// Raw S^T of the 64-key tile at key j0 -> fp32 softmax weights in s: soft clamp, key mask (keys >= kvn), exponential, all in
// base-2 units:
//   clamp*tanh(x)*log2e = C - 2C / (2^(2x log2e) + 1),  C = clamp*log2e   -> v_exp, v_rcp, 1 fma
//   p = 2^(t - m)                                                          -> 1 sub, v_exp
// CLAMP: 0 = plain logits, 1 = soft clamp, 2 = soft clamp with bounded weights, p = 2^(C - 2C / (..)) directly: no maximum (see
// attn_clamp_mode).  ONLINE: the tile is one of several -- m is the running maximum, l and o are rescaled to the new one.  A
// single-tile caller passes ONLINE = false: m, l and o are left alone (0 * alpha is not dropped without fast-math, so a call
// with dummy state would not be the same code).  NT (deduced) = 16-key register tiles of the key tile: 4 in the attention kernels, 1 or 2
// tiles of key slots per head in the absorbed cross-attention (xattn_absorbed.hip).
template <int CLAMP, bool ONLINE, int NT>
__device__ __forceinline__ void attn_weights(f32x4 (&s)[NT], float& m, float& l, f32x4 (&o)[4], int j0, int kvn, int g, AttnLogitScale sc) {
  const float zc = sc.zc, c2 = sc.c2;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (CLAMP == 2) {
        const float e = __builtin_amdgcn_exp2f(s[t][j] * zc);
        s[t][j] = __builtin_amdgcn_exp2f(fmaf(__builtin_amdgcn_rcpf(e + 1.0f), -2.0f * c2, c2));
      } else if constexpr (CLAMP == 1) {
        const float e = __builtin_amdgcn_exp2f(s[t][j] * zc);
        s[t][j] = fmaf(__builtin_amdgcn_rcpf(e + 1.0f), -2.0f * c2, c2);
      } else {
        s[t][j] = s[t][j] * zc;
      }
    }
  if (j0 + 16 * NT > kvn) {             // only the last tile can be partial (wave-uniform branch)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j0 + 16 * t + 4 * g + j >= kvn) s[t][j] = CLAMP == 2 ? 0.f : -INFINITY;
  }
  if constexpr (CLAMP != 2) {
    float mn = -INFINITY;            // row maximum: 16 keys of the lane, then the four key groups of the wave
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) mn = fmaxf(mn, s[t][j]);
    mn = fmaxf(mn, __shfl_xor(mn, 16, 64));
    mn = fmaxf(mn, __shfl_xor(mn, 32, 64));
    if constexpr (ONLINE) {
      mn = fmaxf(m, mn);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[dt][j] *= alpha;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[t][j] = __builtin_amdgcn_exp2f(s[t][j] - mn);
  }
}

// fp32 weights -> row sum l (in (t, j) order) and the P^T operand of the bf16 MFMA, packed in place of the accumulator layout, so
// P never touches LDS: pf[0], and with NPL = 2 the lo plane of the split arithmetic in pf[1].
template <int NPL>
__device__ __forceinline__ void attn_pack_weights(const f32x4 (&s)[4], float& l, bf16x8 (&pf)[NPL][2]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16_t hv = (bf16_t)s[t][j];
      pf[0][t >> 1][(t & 1) * 4 + j] = hv;
      if constexpr (NPL == 2) pf[1][t >> 1][(t & 1) * 4 + j] = (bf16_t)(s[t][j] - (float)hv);
    }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) l += s[t][j];
}

// ---- after the key loop -----------------------------------------------------------------
// NG = 2: key group 1 hands (m, l, O) to group 0, lane for lane (same query / d mapping), through xch = its own dead LDS ring
// (18 floats x 256 lanes = 18 KB).  Every thread of the workgroup calls this; false = group 1, which is done.
__device__ __forceinline__ bool attn_merge_key_groups(float* xch, int grp, int tid, float& m, float& l, f32x4 (&o)[4]) {
  __syncthreads();
  if (grp == 1) {
    float* dst = xch + tid;
    dst[0] = m;
    dst[256] = l;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[(2 + dt * 4 + j) * 256] = o[dt][j];
  }
  __syncthreads();
  if (grp == 1) return false;
  const float* src = xch + tid;
  const float m2 = src[0], l2 = src[256];
  const float mn = fmaxf(m, m2);
  // a group without a key (its tiles all at or beyond kv_len; both groups when kv_len is 0) has m = -inf: weight 0, not 2^(-inf + inf)
  const float a1 = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - mn), a2 = (m2 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m2 - mn);
  l = l * a1 + l2 * a2;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[dt][j] = o[dt][j] * a1 + src[(2 + dt * 4 + j) * 256] * a2;
  return true;
}

// what O is multiplied by on its way out: sigmoid(gate) / l; 0 for queries beyond q_len[b] and for rows without a key
__device__ __forceinline__ float attn_out_factor(const int32_t* q_len, int b, int nq, int query, float l, float gt) {
  const int qn = q_len ? min(q_len[b], nq) : nq;
  return (query < qn && l > 0.f) ? gt / l : 0.f;
}

// O * f of one query to op = its output row at head dimension 4 g: four pieces of four dimensions, 16 apart
template <typename T>
__device__ __forceinline__ void attn_store(T* op, const f32x4 (&o)[4], float f) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    if constexpr (std::is_same<T, float>::value) {
      *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt] * f;
    } else {
      bf16x4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = (bf16_t)(o[dt][j] * f);
      *reinterpret_cast<bf16x4*>(op + 16 * dt) = ov;
    }
  }
}
// the same as hi | lo bf16 planes, the lo plane lo_off elements further: the operand of the out-projection's split GEMM directly
__device__ __forceinline__ void attn_store_split(bf16_t* op, int lo_off, const f32x4 (&o)[4], float f) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // the split of the fp32 value attn_store would have stored: without the barrier -ffp-contract=fast fuses the multiplication
      // by f into the subtraction, and lo then splits the unrounded product (it differs where v - hi is a bf16 rounding tie)
      float v = o[dt][e] * f;
      asm volatile("" : "+v"(v));
      hi[e] = (bf16_t)v;
      lo[e] = (bf16_t)(v - (float)hi[e]);
    }
    *reinterpret_cast<bf16x4*>(op + 16 * dt) = hi;
    *reinterpret_cast<bf16x4*>(op + lo_off + 16 * dt) = lo;
  }
}

// ---- host: which CLAMP instantiation runs -----------------------------------------------
// 0 = no soft clamp, 1 = soft clamp with the running maximum, 2 = soft clamp with BOUNDED weights: logits lie in +-clamp, so
// p = 2^(logit * log2 e) lies in 2^(+-clamp * log2 e) and no maximum has to be tracked -- as long as the fp32 sums l = sum p
// and O = sum p v stay finite: Nk * max|v| * 2^(clamp * log2 e) < 2^128.  Mode 2 is taken while clamp * log2 e + log2 Nk <= 90
// (the shipped clamp 50 with 782 keys: 72.1 + 9.6), which leaves |v| up to 2^38; beyond that the running-maximum kernel runs.
static inline int attn_clamp_mode(float softclamp, int Nk) {
  if (!(softclamp > 0.f)) return 0;
  return softclamp * 1.4426950408889634f + log2f((float)(Nk > 1 ? Nk : 1)) <= 90.f ? 2 : 1;
}
// launch(std::integral_constant<int, CLAMP>) for the mode cl
template <typename F>
static inline int attn_with_clamp(int cl, F&& launch) {
  if (cl == 2) return launch(std::integral_constant<int, 2>{});
  return cl == 1 ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 0>{});
}
