// Shared pieces of the MFMA GEMM kernels (gemm.hip, gemm_8phase.hip, and through xattn_ring.h qproj_xattn.hip and xattn_absorbed.hip): kernel
// parameter block, XCD chunk position (all four), counted ring wait (gemm.hip and xattn_ring.h), row-scale fill and consumer, register staging
// helpers of the v1 kernel, the direct and the LDS-staged fused epilogues.  Everything lives in an anonymous namespace: each
// translation unit gets its own copy.
#pragma once
#include "v2a_common.h"
#include <stdlib.h>
#include <type_traits>

namespace v2a_detail {

struct GemmParams {
  const void* a[3];
  int64_t lda[3];
  int32_t kend[3];  // cumulative K end of each segment
  int32_t nseg;
  const void* w;
  int64_t ldw;
  const float* bias;
  int32_t M, N, K;
  void* out;
  int64_t ldo;
  bf16_t* out2;      // optional bf16 shadow of an fp32 output (operand of a later GEMM)
  int64_t ldo2;
  const float* resid;
  int64_t ldr;
  const float* gate;
  const int32_t* step;
  int64_t gss, gbs;
  int32_t rpb;
  const float* rope;     // cos/sin table [pos][32][2] or null: rotate interleaved pairs of columns < rope_cols (STORE epilogue)
  int32_t rope_cols, rope_pos_off;
  int32_t vec_epi;  // all epilogue pointers / strides allow 16-byte row pieces
  int32_t relu;     // clamp the result at zero (conv + BatchNorm + ReLU blocks of the Video2Roll encoder)
  // implicit-GEMM convolution (DMA kernel only): A row m starts at a[0] + a_rowoff[m], K tile kt adds a_koff[kt] (elements);
  // out / resid / out2 row m starts at base + o_rowoff[m] instead of m * ld
  const int32_t* a_rowoff;
  const int32_t* a_koff;
  const int32_t* o_rowoff;
  int32_t krot;     // start each M band's K walk at a different K tile (see the kernel)
  // RMSNorm folded into its neighbours (v2a_gemm_args: norm_gamma .. row_norm_dim).  Producer: out2 = bf16(out * gamma),
  // ssq[m][n / 32] = sum of squares of 32 output columns.  Consumer: acc row m is scaled by rnorm / max(sqrt(sum_j rssq[m][j]), eps)
  const float* ngam;
  int64_t ngss, ngbs;
  int32_t nsw_row, nsw_off;
  float* ssq;
  int64_t ssq_ld;
  const float* rssq;
  int64_t rssq_ld;
  int32_t rssq_parts;
  float rnorm;
  int32_t xcd_gm, xcd_gn;   // the 8 XCDs of the launch as a gm x gn grid over the tile space (gm * gn == 8): see tile_of_block
  // the rectangles of the tile order, filled on the host once the tile shape is known (fill_tile_map): first tile, height and
  // tile count of each, and 1 / height so that the workgroup's tile costs one multiply and a correction instead of ~40 integer
  // divisions at the head of every kernel
  struct Rect { int32_t m_lo, n_lo, cnt, hm; float rcp; } rect[8];
  int32_t nrect, tiles_m, tiles_n;
  // split (hi | lo plane) outputs of the bf16x3 mode: out2 = the shadow (lo plane N columns after hi), out = the GEGLU hidden
  // (lo plane N / 2 columns after hi)
  int32_t out2_split, out_split;
  int64_t alo[3];           // split operands: elements from a row's hi plane to its lo plane, per segment (default: the segment's K extent)
  int64_t out2_lo;          // split shadow: elements from the hi plane to the lo plane of a shadow row (default: N)
  // 8-phase kernel, split (hi | lo plane) operands: s3_kl = K = the LOGICAL K (sum of the segments' extents).  The K loop walks it once in
  // stages of 32 k, each staged as [32 k hi | 32 k lo] rows of both operands, and adds A_lo x W_hi, A_hi x W_lo, A_hi x W_hi per stage -- over all (up
  // to three) logical segments, whose rows are [hi k | lo k] (lda >= 2k), against weight rows [W_hi (s3_kl) | W_lo (s3_kl)].  0 = plain operands
  int32_t s3_kl;
  int32_t dbg;              // probe builds only (-DV2A_GEMM_PROBE, scripts/probes/kloop_probe.py): K-loop parts switched off by bit
  // step seam (v2a_gemm_cfg_euler, gemm.hip): what the CFG + Euler epilogue of the to_pred GEMM needs besides the GEMM's own operands.  Read by
  // that one instantiation only
  struct Seam {
    float* y;               // latent (B, T, N), updated in place
    const float* dt;        // step sizes, indexed by step[0]
    int32_t* step;          // device step counter: read by every workgroup, advanced by the one that arrives last
    uint32_t* arrive;       // arrival counter of the launch: zero before and after
    bf16_t* planes;         // operand planes of y: rows as the GEMM's A rows (both halves), hi plane at column c, lo plane lo_off further
    int64_t ldp, lo_off;
    int32_t rows_per_seq, row_off, T;
    float s;                // CFG strength
  } seam;
};

// tile-shape selectors of the LDS-DMA bf16 kernels (v2a_set_tuning)
struct GemmTuning {
  int force_tile;        // -1 = by shape
  int krot;              // K rotation (see gemm_bf16_dma_kernel)
  int use_8phase;        // 256x256 phase-interleaved kernel for wide outputs: 0 off, 1 staggered wave rows, 2 lock-step
  int min_tiles_8phase;  // ... when the problem has at least this many 256x256 tiles
  int xcd_grid;          // 1: XCD rectangle grid chosen per shape, 0: always 1 x 8 (every XCD walks all M of its column strip)
  int dbg;               // probe builds only: v2a_tuning.reserved[0]
};
extern GemmTuning g_gemm_tuning;
extern int g_attn_one_group_from;    // v2a_attention: workgroup count from which one wave group per workgroup is used
extern int g_dwconv_rows_per_wave;   // 4 or 8 (v2a_set_tuning)
extern int g_probe_dbg;              // v2a_tuning.reserved[0] (probe builds)
extern int g_dwconv_stream;          // 0: never use the streaming depthwise conv (v2a_tuning.dwconv_rows_per_wave = -1)

// Where a launcher sends its instantiation: to a stream, or -- v2a_gemm_choose -- into a report.  Every launcher calls chosen() with its
// own template constants after its last argument check and in front of its first HIP call, and returns at once when that answers true:
// what is reported is what that very code would have launched.
struct GemmTarget {
  hipStream_t stream;
  v2a_gemm_choice* report;   // null: launch
  bool chosen(const GemmParams& p, int family, bool split, int bm, int bn, int bk, int waves_m, int waves_n, int stages, int tiles) const {
    if (report) *report = {family, split, bm, bn, bk, waves_m, waves_n, stages, tiles, p.xcd_gm, p.xcd_gn, p.vec_epi};
    return report != nullptr;
  }
};

// 256x256 8-phase kernel (gemm_8phase.hip)
int launch_gemm_8phase(const GemmParams& p, int epilogue, int out_dtype, GemmTarget to);

// host: the gm x gn rectangles of the tile space for a BM x BN tile shape (xcd_gm / xcd_gn chosen by v2a_gemm)
inline void fill_tile_map(GemmParams& p, int BM, int BN) {
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  const int gm = p.xcd_gm, gn = p.xcd_gn;
  p.nrect = gm * gn;
  for (int r = 0; r < p.nrect; ++r) {
    const int xm = r / gn, xn = r % gn;
    const int m_lo = xm * p.tiles_m / gm, m_hi = (xm + 1) * p.tiles_m / gm;
    const int n_lo = xn * p.tiles_n / gn, n_hi = (xn + 1) * p.tiles_n / gn;
    const int hm = m_hi - m_lo;
    p.rect[r].m_lo = m_lo;
    p.rect[r].n_lo = n_lo;
    p.rect[r].cnt = hm * (n_hi - n_lo);
    p.rect[r].hm = hm > 0 ? hm : 1;
    p.rect[r].rcp = 1.0f / (float)(hm > 0 ? hm : 1);
  }
}

// host: the consumer side of a folded RMSNorm (row_ssq .. row_norm_dim of v2a_gemm_args and v2a_xattn_absorbed_args) into the parameter
// block, with what rowscale_load needs of it.  who = the entry point that refuses.
inline int fill_row_scale(GemmParams& p, const float* row_ssq, int64_t ld_row_ssq, int row_ssq_parts, int row_norm_dim, const char* who) {
  p.rssq = row_ssq;
  p.rssq_ld = ld_row_ssq;
  p.rssq_parts = row_ssq_parts;
  p.rnorm = sqrtf((float)row_norm_dim);
  if (row_ssq)
    V2A_REQUIRE(row_ssq_parts > 0 && row_ssq_parts <= 40 && row_norm_dim > 0 && ld_row_ssq >= (row_ssq_parts + 3) / 4 * 4 && ld_row_ssq % 4 == 0 &&
                    ((uintptr_t)row_ssq & 15) == 0,
                "%s: row_ssq needs row_ssq_parts <= 40 (%d), row_norm_dim (%d) and rows of whole float4 (zero padded)", who, row_ssq_parts, row_norm_dim);
  return V2A_OK;
}

}  // namespace v2a_detail

namespace {

using v2a_detail::GemmParams;
using v2a_detail::GemmTarget;

// Workgroup -> output tile, XCD-aware.  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the L2 a block
// uses), every XCD has its own 4 MB L2, and an operand panel shared by workgroups on different XCDs is fetched once per XCD.
// The tile space (tiles_m x tiles_n) is therefore cut into a gm x gn grid of rectangles, one per XCD label: the A rows of a
// rectangle are then pulled by gn XCDs and the W rows by gm XCDs, and the host picks (gm, gn) to minimise
// A_bytes * gn + W_bytes * gm (wide outputs: 1 x 8, W read once; narrow ones with long K: 4 x 2 or 2 x 4).  Tiles are
// numbered rectangle by rectangle (M-fastest inside one, so consecutive workgroups of an XCD share a W panel) and label x takes
// the x-th contiguous chunk of that order; chunk and rectangle sizes differ by at most a few tiles, which costs locality only.
// position L of the linear tile order (rectangle by rectangle, M-fastest inside one) -> tile coordinates
__device__ __forceinline__ void tile_of_index(const GemmParams& p, int L, int& tm, int& tn) {
  tm = tn = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (r < p.nrect) {
      const int cnt = p.rect[r].cnt;
      if (L >= 0 && L < cnt) {
        const int hm = p.rect[r].hm;
        int q = (int)((float)L * p.rect[r].rcp);           // L / hm within one for L < 2^24 (checked on the host), corrected below
        int rem = L - q * hm;
        if (rem < 0) { --q; rem += hm; }
        else if (rem >= hm) { ++q; rem -= hm; }
        tn = p.rect[r].n_lo + q;
        tm = p.rect[r].m_lo + rem;
      }
      L -= cnt;          // negative from the containing rectangle on: no later one matches
    }
  }
}
// workgroup bid of nwg -> position in a linear order of the launch's work: XCD x (bid & 7) takes the x-th contiguous chunk.  Bijective.
__device__ __forceinline__ int xcd_chunk_position(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
__device__ __forceinline__ void tile_of_block(const GemmParams& p, int bid, int& tm, int& tn) {
  tile_of_index(p, xcd_chunk_position(bid, p.tiles_m * p.tiles_n), tm, tn);
}

// LDS-DMA rings: wait until at most min(J, younger) of the youngest K tiles' DMAs (LPW instructions per wave each) are still outstanding.
// The counted s_waitcnt needs an immediate, so the tail of the K loop walks down a chain of them.
template <int J, int LPW>
__device__ __forceinline__ void ring_wait(int younger) {
  if constexpr (J == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    static_assert(J * LPW <= 63, "vmcnt is a 6-bit field");
    if (younger >= J) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(J * LPW) : "memory");
    else ring_wait<J - 1, LPW>(younger);
  }
}

// the gated-linear-unit epilogues share the [16 value | 16 gate] row packing and the N / 2 output columns; they differ in the gate's activation
__host__ __device__ constexpr bool is_glu(int epi) { return epi == V2A_EPI_GEGLU || epi == V2A_EPI_SWIGLU; }
// FAST: the forms whose result is rounded to bf16 planes anyway (Abramowitz-Stegun erf; v_exp based silu); otherwise exact erff / expf and division
template <int EPI, bool FAST> __device__ __forceinline__ float glu_act(float g) {
  if constexpr (EPI == V2A_EPI_SWIGLU) return FAST ? silu_f(g) : silu_exact_f(g);
  else return FAST ? gelu_fast_f(g) : gelu_erf_f(g);
}

// the pointwise activation epilogues (CLIP's MLPs): out = act(acc + bias) on all N columns; they share every dispatch path, restriction and store form
__host__ __device__ constexpr bool is_act(int epi) { return epi == V2A_EPI_GELU || epi == V2A_EPI_QUICK_GELU; }
// FAST: as for glu_act (Abramowitz-Stegun erf; v_exp / v_rcp based QuickGELU)
template <int EPI, bool FAST> __device__ __forceinline__ float pointwise_act(float v) {
  if constexpr (EPI == V2A_EPI_QUICK_GELU) return FAST ? quick_gelu_fast_f(v) : quick_gelu_exact_f(v);
  else return FAST ? gelu_fast_f(v) : gelu_erf_f(v);
}

template <typename T> struct TileCfg;
template <> struct TileCfg<bf16_t> {
  static constexpr int BK = 64;
  static constexpr int LDS_ROW = 64;  // elements per LDS row (128 B)
};
template <> struct TileCfg<float> {
  static constexpr int BK = 16;
  static constexpr int LDS_ROW = 20;  // padded: 80 B rows keep float4 writes aligned, 2-way max on reads
};

// ---- global -> register staging ----------------------------------------------------------
// bf16 tile: ROWS x 64 bf16; thread t covers 16-B chunk (t & 7) of rows (t >> 3) + 32*i.
template <int ROWS, bool SRC_F32> struct StageBf16 {
  static constexpr int N = ROWS / 32;
  bf16x8 r[N];
  __device__ __forceinline__ void load(const void* base, int64_t ld, int row0, int rows_total, int k0, int tid) {
    const int chunk = tid & 7;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int row = row0 + (tid >> 3) + 32 * i;
      row = row < rows_total ? row : rows_total - 1;
      if constexpr (SRC_F32) {
        const float* p = reinterpret_cast<const float*>(base) + (int64_t)row * ld + k0 + chunk * 8;
        f32x4 lo = *reinterpret_cast<const f32x4*>(p);
        f32x4 hi = *reinterpret_cast<const f32x4*>(p + 4);
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = (bf16_t)lo[j];
          v[4 + j] = (bf16_t)hi[j];
        }
        r[i] = v;
      } else {
        const bf16_t* p = reinterpret_cast<const bf16_t*>(base) + (int64_t)row * ld + k0 + chunk * 8;
        r[i] = *reinterpret_cast<const bf16x8*>(p);
      }
    }
  }
  __device__ __forceinline__ void store(bf16_t* lds, int tid) const {
    const int chunk = tid & 7;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int row = (tid >> 3) + 32 * i;
      *reinterpret_cast<bf16x8*>(lds + row * 64 + ((chunk ^ (row & 7)) << 3)) = r[i];
    }
  }
};

// fp32 tile: ROWS x 16 floats; thread t covers float4 (t & 3) of rows (t >> 2) + 64*i.
template <int ROWS> struct StageF32 {
  static constexpr int N = ROWS / 64;
  f32x4 r[N];
  __device__ __forceinline__ void load(const void* base, int64_t ld, int row0, int rows_total, int k0, int tid) {
    const int c4 = tid & 3;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int row = row0 + (tid >> 2) + 64 * i;
      row = row < rows_total ? row : rows_total - 1;
      const float* p = reinterpret_cast<const float*>(base) + (int64_t)row * ld + k0 + c4 * 4;
      r[i] = *reinterpret_cast<const f32x4*>(p);
    }
  }
  __device__ __forceinline__ void store(float* lds, int tid) const {
    const int c4 = tid & 3;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      int row = (tid >> 2) + 64 * i;
      *reinterpret_cast<f32x4*>(lds + row * 20 + c4 * 4) = r[i];
    }
  }
};

template <typename T, bool A_F32, int ROWS> struct StageSel;
template <bool A_F32, int ROWS> struct StageSel<bf16_t, A_F32, ROWS> { using type = StageBf16<ROWS, A_F32>; };
template <bool A_F32, int ROWS> struct StageSel<float, A_F32, ROWS> { using type = StageF32<ROWS>; };

// ---- shared epilogue: C/D layout col = lane & 15, row = (lane >> 4) * 4 + j ------------------
template <int EPI, typename OutT, int TM, int TN, int WM, int WN>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[TM][TN], int m0, int n0, int wm, int wn,
                                              int lr, int lq) {
  OutT* out = reinterpret_cast<OutT*>(p.out);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int m = m0 + wm * WM + i * 16 + lq * 4 + jj;
      if (m >= p.M) continue;
      const float* gvec = nullptr;
      if constexpr (EPI == V2A_EPI_GATE_RESID) gvec = step_vec(p.gate, p.step, p.gss, p.gbs, p.gbs ? m / p.rpb : 0);
      if constexpr (is_glu(EPI)) {
#pragma unroll
        for (int j = 0; j < TN; j += 2) {
          const int n = n0 + wn * WN + j * 16 + lr;  // packed row index of the value
          if (n >= p.N) continue;
          float v = acc[i][j][jj], g = acc[i][j + 1][jj];
          if (p.bias) { v += p.bias[n]; g += p.bias[n + 16]; }
          const int oc = ((n0 + wn * WN) >> 1) + (j >> 1) * 16 + lr;
          const float ge = glu_act<EPI, sizeof(OutT) == 2>(g);
          out[(int64_t)m * p.ldo + oc] = from_f32<OutT>(v * ge);
        }
      } else {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + wn * WN + j * 16 + lr;
          if (n >= p.N) continue;
          float v = acc[i][j][jj];
          if (p.bias) v += p.bias[n];
          if constexpr (EPI == V2A_EPI_SIGMOID) v = sigmoid_f(v);
          if constexpr (is_act(EPI)) v = pointwise_act<EPI, false>(v);
          if constexpr (EPI == V2A_EPI_RESID) v += p.resid[(int64_t)m * p.ldr + n];
          if constexpr (EPI == V2A_EPI_GATE_RESID) v = p.resid[(int64_t)m * p.ldr + n] + gvec[n] * v;
          if (p.relu) v = fmaxf(v, 0.f);
          out[(int64_t)m * p.ldo + n] = from_f32<OutT>(v);
          if constexpr (sizeof(OutT) == 4) {
            if (p.out2) p.out2[(int64_t)m * p.ldo2 + n] = (bf16_t)v;
          }
        }
      }
    }
  }
}


// ---- LDS-staged epilogue (DMA kernels) -----------------------------------------------------
// The MFMA C layout gives a lane 4 ROWS of one column, so direct stores are 2-4 byte pieces.
// Instead every wave parks its WM x WN fp32 tile in a private LDS region (the K-loop stages are
// dead by then), and reads it back row-major 4 columns per lane: bias / GELU / gate / residual run
// on float4s and every global access is a 16-byte (fp32) or 8-byte (bf16) piece of a contiguous row.
// Residual / gate pieces of the vector epilogue, fetched at kernel start so their L2/HBM latency hides under the K loop
// instead of being paid once per 16-row slab at the tail of every workgroup (same lane -> (row, 4 columns) map as below).
template <int EPI, int TM, int WN, bool ON> struct EpiPrefetch {
  static constexpr int LPR = WN / 4, RPI = 64 / LPR, RPS = 16 / RPI;   // lanes per row, rows per pass, rows per slab and lane
  static constexpr bool RES = ON && (EPI == V2A_EPI_RESID || EPI == V2A_EPI_GATE_RESID);
  static constexpr bool GATE = ON && EPI == V2A_EPI_GATE_RESID;
  f32x4 rs[RES ? TM : 1][RES ? RPS : 1];
  f32x4 gt[GATE ? TM : 1][GATE ? RPS : 1];
  static constexpr bool SCAT = RES && !GATE;   // offset tables come with STORE / RESID only (checked on the host)
  int32_t ro[SCAT ? TM : 1][SCAT ? RPS : 1];  // out / resid row offsets when rows are scattered (o_rowoff)
  static constexpr bool ROPE = ON && EPI == V2A_EPI_STORE;
  f32x4 cs[ROPE ? TM : 1][ROPE ? RPS : 1];     // (cos, sin) of the two column pairs a lane rotates
  __device__ __forceinline__ void load(const GemmParams& p, int m_base, int n_base, int lane) {
    if constexpr (ROPE) {
      const int c4 = (lane % LPR) * 4, r0 = lane / LPR;
      const int n = n_base + c4;
      if (p.rope && n < p.rope_cols) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int q = 0; q < RPS; ++q) {
            int m = m_base + i * 16 + r0 + q * RPI;
            m = m < p.M ? m : p.M - 1;
            const int pos = p.rope_pos_off + m % p.rpb;
            cs[i][q] = *reinterpret_cast<const f32x4*>(p.rope + ((int64_t)pos * 32 + ((n & 63) >> 1)) * 2);
          }
      }
    }
    if constexpr (RES) {
      const int c4 = (lane % LPR) * 4, r0 = lane / LPR;
      const int n = n_base + c4;
      // kernel arguments copied once: the loops below stay free of scalar re-loads and branches
      const int M = p.M;
      const bool full = n + 3 < p.N;
      const bool has_res = p.resid != nullptr, has_gate = p.gate != nullptr;     // wave-uniform
      const float* resid = p.resid + n;
      const int64_t ldr = p.ldr;
      const int32_t* orow = SCAT ? p.o_rowoff : nullptr;
      // scattered rows (implicit-GEMM convolution): all row offsets are requested before the first residual row depends on one
      if constexpr (SCAT) {
        if (orow) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < RPS; ++q) {
              int m = m_base + i * 16 + r0 + q * RPI;
              m = m < M ? m : M - 1;
              ro[i][q] = orow[m];
            }
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < RPS; ++q) {
          const int m = m_base + i * 16 + r0 + q * RPI;
          if (m < M && full) {
            int64_t off = (int64_t)m * ldr;
            if constexpr (SCAT) { if (orow) off = ro[i][q]; }
            // absent operands read as 0 / 1 (resid + 1 * acc is exactly the RESID epilogue, 0 + 1 * acc the plain store)
            rs[i][q] = has_res ? *reinterpret_cast<const f32x4*>(resid + off) : f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (GATE) gt[i][q] = has_gate ? *reinterpret_cast<const f32x4*>(step_vec(p.gate, p.step, p.gss, p.gbs, p.gbs ? m / p.rpb : 0) + n) : f32x4{1.f, 1.f, 1.f, 1.f};
          }
        }
    }
  }
};

// Folded RMSNorm, consumer side: 1 / rms of A row m (F.normalize: x / max(||x||, 1e-12), times sqrt(d)) from the sums of squares
// the producer of that row left per 32 columns.  One thread per tile row requests the row's partial sums when the kernel starts
// (before the first operand DMA, so waiting for them drains nothing), adds them up in a fixed order -- the scale does not depend
// on the tile shape -- and leaves the scale in LDS behind the ring for the epilogue.
constexpr int kRowSsqMax = 40;                // partial sums per row: d <= 1280
struct RowScaleLoad {
  f32x4 v[kRowSsqMax / 4];
};
__device__ __forceinline__ void rowscale_load(const GemmParams& p, int m, RowScaleLoad& r) {
  m = m < p.M ? m : p.M - 1;
  const float* q = p.rssq + (int64_t)m * p.rssq_ld;
#pragma unroll
  for (int k = 0; k < kRowSsqMax / 4; ++k) {
    r.v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (4 * k < p.rssq_parts) r.v[k] = *reinterpret_cast<const f32x4*>(q + 4 * k);
  }
}
__device__ __forceinline__ float rowscale_finish(const GemmParams& p, const RowScaleLoad& r) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kRowSsqMax / 4; ++k) s += (r.v[k][0] + r.v[k][1]) + (r.v[k][2] + r.v[k][3]);
  return p.rnorm / fmaxf(sqrtf(s), 1e-12f);
}

// Interleaved RoPE of four columns (two pairs) by cs = (cos, sin, cos, sin) of the pairs.  One fixed contraction: left to
// -ffp-contract the kernels' instantiations picked different multiply-add pairings and the rotated columns differed in the
// last bit between tile shapes.
__device__ __forceinline__ void rope_rotate4(f32x4& v, const f32x4& cs) {
  const float a0 = v[0], b0 = v[1], a1 = v[2], b1 = v[3];
  v[0] = fmaf(a0, cs[0], -(b0 * cs[1]));
  v[1] = fmaf(b0, cs[0], a0 * cs[1]);
  v[2] = fmaf(a1, cs[2], -(b1 * cs[3]));
  v[3] = fmaf(b1, cs[2], a1 * cs[3]);
}

// Position of a row inside its batch element (m % rpb) and the batch elements it lies behind the wave's first row, from the position of the wave's
// first row (one division per wave, gemm_epilogue_lds) and the row's distance d from it: one compare-and-subtract, since rpb need not be a multiple of
// anything here.  A batch element shorter than the wave tile (no shape the engines launch) can be wrapped more than once: the loop behind the test.
__device__ __forceinline__ void row_pos(int p0, int d, int rpb, bool multi, int& pos, int& nb) {
  pos = p0 + d;
  nb = 0;
  if (pos >= rpb) { pos -= rpb; nb = 1; }
  if (multi) {
    while (pos >= rpb) { pos -= rpb; ++nb; }
  }
}

// Epilogue operands and the chain they once formed (PF = false: the 8-phase kernel and the ring tiles whose registers do not allow a prefetch at
// kernel start).  gfx950 counts loads and stores in ONE in-order vmcnt, so a load requested between two rows' stores is waited for with vmcnt(0),
// which also waits for every store before it: with the cos/sin or residual row requested per row, a wave paid one L2 round trip and one store
// drain per row, 32 times in a row (profiles/r07_8phase_epilogue_ab.txt).  Now:
//   * what does not depend on the slab -- the bias pieces of the lane's columns, the device step counter (one wave-uniform load, turned into base
//     pointers of the gate / gamma step vectors), and the gate / gamma pieces of the lane's columns for the one or two batch elements the wave's rows
//     lie in -- is requested once, ahead of the slab loop: in the 8-phase kernel right behind the barrier that ends the K loop, into the registers
//     the fragments free.  It is waited for once, behind the first slab's LDS writes;
//   * what depends on the row -- cos/sin rows (STORE), residual rows (RESID, GATE_RESID) -- runs in a two-slab pipeline: slab i + 1's rows are
//     requested before slab i's stores are issued, so the wait for them can count past those stores.  A wave whose tile lies wholly inside the
//     problem (all but the last row band / a 16-column last tile) and whose rows are dense runs a form of the loop without row or column
//     predicates (ALL): the compiler's counts take the lower bound over every branch, and a row block that may be skipped counts for nothing;
//   * a row's position in its batch element comes from one division per wave (its first row) and a compare-and-subtract per row;
//   * slabs behind the last row end the loop (they are a suffix of the wave's slabs), so nothing is requested for them.
// A batch element shorter than the wave tile (more than two elements under a wave) keeps per-row gate / gamma loads, without the step counter.
// The arithmetic of every element is what it was: same expressions, same order.
// (The two forms are two instantiations of a function, not two calls of a generic lambda: a select between variables a lambda captures by
// reference becomes a load through a selected address and puts the accumulators on the stack.)
template <int EPI, bool PF> constexpr bool epi_pipelined() { return !PF && (EPI == V2A_EPI_STORE || EPI == V2A_EPI_RESID || EPI == V2A_EPI_GATE_RESID); }

template <int EPI, typename OutT, int TM, int TN, int WM, int WN, bool PF, bool ALL>
__device__ __forceinline__ void gemm_epilogue_lds_impl(const GemmParams& p, f32x4 (&acc)[TM][TN], float* tile, int m_base, int n_base, int lane,
                                                       const EpiPrefetch<EPI, TM, WN, PF>& pf, const float* rs_row) {
  constexpr int LD = WN + 4;                   // 16-B aligned rows, <= 2-way write conflicts
  const int lr = lane & 15, lq = lane >> 4;
  OutT* out = reinterpret_cast<OutT*>(p.out);
  // kernel arguments copied once (the slab loops below otherwise re-load them from the argument segment per row)
  const int M = p.M, N = p.N;
  const bool relu = p.relu != 0;
  const int32_t* orow = ALL ? nullptr : p.o_rowoff;   // scattered rows (implicit-GEMM convolution into a bordered map) or null; never in the ALL form
  const int64_t ldo = p.ldo, ldr = p.ldr, ldo2 = p.ldo2;
  bf16_t* out2 = p.out2;
  const float* resid = p.resid;
  const float* bias = p.bias;
  // folded RMSNorm, consumer side: one scale per row this lane touches, all requested before the first slab is staged
  constexpr int LPRX = (is_glu(EPI) ? WN / 2 : WN) / 4;   // lanes per row of the store loops below
  constexpr int RPSX = 16 / (64 / LPRX);                           // rows per lane per slab
  constexpr bool RESF = EPI == V2A_EPI_RESID || EPI == V2A_EPI_GATE_RESID;
  constexpr bool GAMF = RESF && sizeof(OutT) == 4;                 // folded RMSNorm, producer side: the shadow carries the norm's gamma
  constexpr bool PIPE = epi_pipelined<EPI, PF>();                  // row operands in the two-slab pipeline
  static_assert(PIPE || !ALL, "the unpredicated form belongs to the pipeline");
  // lane -> (row, 4 columns) map of the plain store form
  constexpr int LPRV = WN / 4, RPIV = 64 / LPRV, RPSV = 16 / RPIV;
  const int c4v = (lane % LPRV) * 4, r0v = lane / LPRV;
  const int nv = n_base + c4v;
  const bool fullv = nv + 3 < N;               // N is a multiple of 4 for every vector-eligible call (checked on the host)
  const bool scaled = rs_row != nullptr;                           // wave-uniform
  // GEGLU with 16-byte stores (below): needs 16-byte aligned output rows and planes
  const bool geglu_wide = is_glu(EPI) && sizeof(OutT) == 2 && (WN / 2) % 32 == 0 && ((uintptr_t)p.out & 15) == 0 && (p.ldo & 7) == 0 &&
                          ((p.N >> 1) & 7) == 0 && !(p.dbg & 128);       // v2a_tuning.reserved[0] bit 7: the four-column form (A/B)

  // ---- slab-invariant operands -------------------------------------------------------------------------------------------------
  // bias pieces of the lane's columns, by store form: GLU eight-column (value 0-3, 4-7, gate 0-3, 4-7), GLU four-column (value, -, gate, -), plain
  f32x4 bb[is_glu(EPI) ? 4 : 1];
#pragma unroll
  for (int k = 0; k < (is_glu(EPI) ? 4 : 1); ++k) bb[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (is_glu(EPI)) {
    if (geglu_wide) {
      const int c8 = (lane % (WN / 16)) * 8;
      const int n = n_base + (c8 >> 4) * 32 + (c8 & 15);
      if (bias && n < N) {
        bb[0] = *reinterpret_cast<const f32x4*>(bias + n);
        bb[1] = *reinterpret_cast<const f32x4*>(bias + n + 4);
        bb[2] = *reinterpret_cast<const f32x4*>(bias + n + 16);
        bb[3] = *reinterpret_cast<const f32x4*>(bias + n + 20);
      }
    } else {
      const int c4 = (lane % (WN / 8)) * 4;
      const int n = n_base + (c4 >> 4) * 32 + (c4 & 15);
      if (bias && n < N) {
        bb[0] = *reinterpret_cast<const f32x4*>(bias + n);
        bb[2] = *reinterpret_cast<const f32x4*>(bias + n + 16);
      }
    }
  } else {
    if (bias && fullv) bb[0] = *reinterpret_cast<const f32x4*>(bias + nv);
  }
  // the device step counter, read once per wave (a wave-uniform address: a scalar load), as base pointers of the gate / gamma step vectors
  const float* gate_b = nullptr;
  const float* ngam_b = nullptr;
  if constexpr (RESF) {
    const int64_t stepv = p.step ? (int64_t)p.step[0] : 0;
    if (p.gate) gate_b = p.gate + stepv * p.gss;
    if (p.ngam) ngam_b = p.ngam + stepv * p.ngss;
  }
  // the wave's first row inside its batch element: the one division
  const int rpb = p.rpb;
  const bool rope_on = PIPE && EPI == V2A_EPI_STORE && p.rope != nullptr && n_base < p.rope_cols;   // rope_cols % 64 == 0 and the wave's
  static_assert(64 % WN == 0 || EPI != V2A_EPI_STORE || PF, "a wave's columns lie in one 64-column head");   // columns lie in one head: wave-uniform
  const bool gate_pb = PIPE && EPI == V2A_EPI_GATE_RESID && gate_b != nullptr && p.gbs != 0;
  const bool gam_on = GAMF && out2 != nullptr && ngam_b != nullptr;
  const bool gam_pb = gam_on && p.ngbs != 0;
  int b0 = 0, p0 = 0;
  bool onebatch = true, twobatch = true;
  if (rope_on || gate_pb || (PIPE && gam_pb)) {
    const int mb = __builtin_amdgcn_readfirstlane(m_base);
    b0 = mb / rpb;
    p0 = mb - b0 * rpb;
    const int last = p0 + ((mb + WM < M ? mb + WM : M) - 1 - mb);      // the wave's last row, counted from the start of the first row's batch element
    onebatch = last < rpb;
    twobatch = last < 2 * rpb;
  }
  const int m_sw = m_base - p0 + rpb;          // first row of the next batch element
  const bool multi = rpb < WM;                 // a wave tile can span more than two batch elements
  // gate / gamma pieces of the lane's columns, once per wave: shared over the batch, or per batch for the (at most two, unless a batch element is
  // shorter than the wave tile) elements the wave's rows lie in -- the second set is read only when rows of a second element exist.  Then the row picks
  // its set by a compare, as at the switch row.  Waves that span more elements load per row (gate_row / gam_row), without the step counter.
  // PF = true kernels keep their form: shared gamma once, per-batch gamma per row.
  const bool gate_row = gate_pb && !twobatch, gam_row = gam_pb && !(PIPE && twobatch);
  const bool gate_two = gate_pb && !onebatch && !gate_row, gam_two = PIPE && gam_pb && !onebatch && !gam_row;   // rows from m_sw on take the second set
  f32x4 gmA = {1.f, 1.f, 1.f, 1.f}, gmB = gmA, gmC = gmA, gmD = gmA, gt1 = gmA, gt2 = gmA;
  if constexpr (GAMF) {
    if (gam_on && !gam_row && fullv && m_base < M) {
      const float* gb = ngam_b + (gam_pb ? (int64_t)b0 * p.ngbs : 0) + nv;
      gmA = *reinterpret_cast<const f32x4*>(gb);
      gmB = *reinterpret_cast<const f32x4*>(gb + p.nsw_off);
      if constexpr (PIPE) {
        if (gam_two) {
          gmC = *reinterpret_cast<const f32x4*>(gb + p.ngbs);
          gmD = *reinterpret_cast<const f32x4*>(gb + p.ngbs + p.nsw_off);
        }
      }
    }
  }
  if constexpr (PIPE && EPI == V2A_EPI_GATE_RESID) {
    if (gate_b && !gate_row && fullv && m_base < M) {
      const float* gp = gate_b + (gate_pb ? (int64_t)b0 * p.gbs : 0) + nv;
      gt1 = *reinterpret_cast<const f32x4*>(gp);
      if (gate_two) gt2 = *reinterpret_cast<const f32x4*>(gp + p.gbs);
    }
  }
  // (the pipelined form reads a row's scale from LDS when it comes to the row: 32 registers it needs for the rows in flight)
  float rsc[PIPE ? 1 : TM][PIPE ? 1 : RPSX];
  if constexpr (!PIPE) {
    if (scaled) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < RPSX; ++q) rsc[i][q] = rs_row[i * 16 + lane / LPRX + q * (64 / LPRX)];
    }
  }

  // ---- slab-variant operands: two sets, slab i reads set i & 1 while set (i + 1) & 1 is in flight -----------------------------------
  f32x4 q_a[PIPE ? 2 : 1][PIPE ? RPSV : 1];                                                  // STORE: (cos, sin) pairs; RESID / GATE_RESID: residual pieces
  {
    // (the trip i = -1 only requests slab 0: one copy of the request code, in line -- as a lambda called from two places it made the compiler keep
    // both sets in one 32-register tuple, copied whole after every load)
#pragma unroll
    for (int i = -1; i < TM; ++i) {
      // a slab wholly behind the last row (wave-uniform): nothing to stage or store, and so for every slab after it -- nothing was requested for it either
      if (!ALL && m_base + (i < 0 ? 0 : i) * 16 >= M) break;
      if constexpr (PIPE) {
        // slab i + 1's rows go out before slab i's stores (none for a slab behind the last row); the fence keeps them there
        if (i + 1 < TM && (ALL || m_base + (i + 1) * 16 < M)) {
#pragma unroll
          for (int q = 0; q < RPSV; ++q) {
            const int m = m_base + (i + 1) * 16 + r0v + q * RPIV;
            const bool ok = ALL || (m < M && fullv);
            if constexpr (EPI == V2A_EPI_STORE) {
              if (rope_on && ok) {
                int pos, nb;
                row_pos(p0, m - m_base, rpb, multi, pos, nb);
                q_a[(i + 1) & 1][q] = *reinterpret_cast<const f32x4*>(p.rope + ((int64_t)(p.rope_pos_off + pos) * 32 + ((nv & 63) >> 1)) * 2);
              }
            }
            if constexpr (RESF) {
              if (ok) {
                int64_t o_res = (int64_t)m * ldr;
                if constexpr (EPI == V2A_EPI_RESID) { if (orow) o_res = orow[m]; }
                q_a[(i + 1) & 1][q] = *reinterpret_cast<const f32x4*>(resid + o_res + nv);       // (the host requires resid with these epilogues)
              }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i < 0) continue;
      // one 16-row slab of the wave tile at a time: the staging area of a workgroup is a few KB of one ring stage
      // (fences around slabs and rows of the pipelined form: its unpredicated loop is one basic block of eight slabs, and left alone the scheduler
      // lifts addresses and LDS reads of later rows over earlier ones until the accumulators spill)
      if constexpr (PIPE) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) tile[(lq * 4 + jj) * LD + j * 16 + lr] = acc[i][j][jj];
      // same wave wrote and reads: LDS operations of one wave complete in order, no barrier needed
      if (i == 0) {
        // the one wait for the slab-invariant operands, behind the first slab's LDS writes: a use here, so that the compiler waits here once.  Left to
        // the first real use it repeats the wait in every row block (each can be entered past the others) as vmcnt(0), which drains the row's stores
#pragma unroll
        for (int k = 0; k < (is_glu(EPI) ? 4 : 1); ++k) asm volatile("" : "+v"(bb[k]));
        if constexpr (GAMF) asm volatile("" : "+v"(gmA), "+v"(gmB), "+v"(gmC), "+v"(gmD));
        if constexpr (PIPE && EPI == V2A_EPI_GATE_RESID) asm volatile("" : "+v"(gt1), "+v"(gt2));
      }
      if constexpr (is_glu(EPI) && sizeof(OutT) == 2 && (WN / 2) % 32 == 0) {
        // bf16 / hi | lo outputs of a wave tile with >= 32 output columns: EIGHT columns per lane, so that every global store is 16 bytes (the
        // 8-byte pieces of the four-column form below made the 128 KB of a 256x256 tile's planes a store-issue-bound tail); taken when the
        // rows allow it (wave-uniform test), the four-column form otherwise
        if (geglu_wide) {
          constexpr int OC = WN / 2, LPR = OC / 8, RPI = 64 / LPR;
          static_assert(RPI <= 16, "one slab holds 16 rows");
          const int c8 = (lane % LPR) * 8, r0 = lane / LPR;
          const int lc = (c8 >> 4) * 32 + (c8 & 15);            // LDS column of the first value; the gates lie 16 further
          const int n = n_base + lc;
#pragma unroll
          for (int q = 0; q < 16 / RPI; ++q) {
            const int r = r0 + q * RPI;
            const int m = m_base + i * 16 + r;
            if (m >= M || n >= N) continue;
            const float rs = scaled ? rs_row[i * 16 + r] : 1.f;
            bf16x8 hi, lo;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              f32x4 v = *reinterpret_cast<const f32x4*>(tile + r * LD + lc + 4 * h2);
              f32x4 g = *reinterpret_cast<const f32x4*>(tile + r * LD + lc + 16 + 4 * h2);
              if (scaled) {          // (the same expressions as the four-column form: equal bit for bit)
                v *= rs;
                g *= rs;
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float o32 = (v[e] + bb[h2][e]) * glu_act<EPI, true>(g[e] + bb[2 + h2][e]);
                hi[4 * h2 + e] = (bf16_t)o32;
                lo[4 * h2 + e] = (bf16_t)(o32 - (float)hi[4 * h2 + e]);
              }
            }
            OutT* dst = out + (int64_t)m * ldo + (n_base >> 1) + c8;
            *reinterpret_cast<bf16x8*>(dst) = hi;
            if (p.out_split) *reinterpret_cast<bf16x8*>(dst + (N >> 1)) = lo;
          }
          continue;
        }
      }
      if constexpr (is_glu(EPI)) {
        constexpr int OC = WN / 2;                 // output columns of this wave
        constexpr int LPR = OC / 4;                // lanes per row
        constexpr int RPI = 64 / LPR;              // rows per pass
        const int c4 = (lane % LPR) * 4, r0 = lane / LPR;
        const int lc = (c4 >> 4) * 32 + (c4 & 15); // LDS column of the value; gate is 16 further
        const int n = n_base + lc;                 // packed W row of the value
        const f32x4 bv = bb[0], bg = bb[2];
#pragma unroll
        for (int q = 0; q < 16 / RPI; ++q) {
          const int r = r0 + q * RPI;
          const int m = m_base + i * 16 + r;
          if (m >= M || n >= N) continue;
          f32x4 v = *reinterpret_cast<const f32x4*>(tile + r * LD + lc);
          f32x4 g = *reinterpret_cast<const f32x4*>(tile + r * LD + lc + 16);
          if (scaled) {
            v *= rsc[i][q];
            g *= rsc[i][q];
          }
          OutT* dst = out + (int64_t)m * ldo + (n_base >> 1) + c4;
          if constexpr (sizeof(OutT) == 2) {
            if (p.out_split) {
              // bf16x3 mode: the fp32 product stored as hi | lo planes (lo plane N / 2 columns further).  SWIGLU: silu on v_exp_f32 (a few ulp, below the
              // 2^-17 the planes keep).  GEGLU: erf by Abramowitz-Stegun 7.1.26
              // (|error| <= 1.5e-7, two orders below the 2^-17 the planes keep): libm's branchy erff cost ~20 us per 256x256 tile round
              // here against ~6 (64 values per lane), a fifth of a feed-forward launch at 8 clips per GPU
              bf16x4 hi, lo;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float o32 = (v[e] + bv[e]) * glu_act<EPI, true>(g[e] + bg[e]);
                hi[e] = (bf16_t)o32;
                lo[e] = (bf16_t)(o32 - (float)hi[e]);
              }
              *reinterpret_cast<bf16x4*>(dst) = hi;
              *reinterpret_cast<bf16x4*>(dst + (N >> 1)) = lo;
            } else {
              bf16x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = (bf16_t)((v[e] + bv[e]) * glu_act<EPI, true>(g[e] + bg[e]));
              *reinterpret_cast<bf16x4*>(dst) = o;
            }
          } else {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[e] + bv[e]) * glu_act<EPI, false>(g[e] + bg[e]);
            *reinterpret_cast<f32x4*>(dst) = o;
          }
        }
      } else {
        constexpr int RPI = RPIV;
        const int c4 = c4v, r0 = r0v, n = nv;
        const bool full = fullv;
        const f32x4 bv = bb[0];
#pragma unroll
        for (int q = 0; q < 16 / RPI; ++q) {
          const int r = r0 + q * RPI;
          const int m = m_base + i * 16 + r;
          if (!ALL && (m >= M || !full)) continue;
          int64_t o_out = (int64_t)m * ldo, o_res = (int64_t)m * ldr, o_out2 = (int64_t)m * ldo2;
          if constexpr (EPI == V2A_EPI_STORE || EPI == V2A_EPI_RESID) {     // offset tables come with STORE / RESID only
            if (orow) {
              int64_t ro;
              if constexpr (PF && EPI == V2A_EPI_RESID) ro = pf.ro[i][q];
              else ro = orow[m];
              o_out = o_res = o_out2 = ro;
            }
          }
          f32x4 v = *reinterpret_cast<const f32x4*>(tile + r * LD + c4);
          if (scaled) v *= PIPE ? rs_row[i * 16 + r] : rsc[PIPE ? 0 : i][PIPE ? 0 : q];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bv[e];
          if constexpr (EPI == V2A_EPI_SIGMOID) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = sigmoid_f(v[e]);
          }
          if constexpr (is_act(EPI)) {
            // fp32 output: exact erff / expf and division (fp32 parity of CLIPMLP); hi | lo planes: Abramowitz-Stegun erf (|error| <= 1.5e-7,
            // below the 2^-17 the planes keep), as the GEGLU epilogue's split form; QuickGELU on v_exp / v_rcp
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pointwise_act<EPI, sizeof(OutT) == 2>(v[e]);
          }
          if constexpr (EPI == V2A_EPI_STORE) {
            // interleaved RoPE (A6): columns (n, n+1) and (n+2, n+3) are pairs (n & 63) / 2 and +1 of this head
            if constexpr (PF) {
              if (p.rope && n < p.rope_cols) rope_rotate4(v, pf.cs[i][q]);
            } else {
              if (rope_on) rope_rotate4(v, q_a[i & 1][q]);
            }
          }
          if constexpr (RESF) {
            f32x4 rs, gt = {1.f, 1.f, 1.f, 1.f};
            if constexpr (PF) {
              rs = pf.rs[i][q];
              if constexpr (EPI == V2A_EPI_GATE_RESID) gt = pf.gt[i][q];
            } else {
              rs = q_a[i & 1][q];
              if constexpr (EPI == V2A_EPI_GATE_RESID) {
                gt = gate_two && m >= m_sw ? gt2 : gt1;
                if (gate_row) {
                  int pos, nb;
                  row_pos(p0, m - m_base, rpb, true, pos, nb);
                  gt = *reinterpret_cast<const f32x4*>(gate_b + (int64_t)(b0 + nb) * p.gbs + n);
                  asm volatile("" : "+v"(gt));      // a use inside the branch: the wait for this load stays in here, off the path that does not load
                }
              }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rs[e] + gt[e] * v[e];
          }
          if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
          }
          if constexpr (sizeof(OutT) == 2) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
            *reinterpret_cast<bf16x4*>(out + o_out + n) = o;
            if constexpr (is_act(EPI)) {
              if (p.out_split) {       // bf16x3 mode: the lo plane, N columns after the hi plane (the next GEMM's split operand)
                bf16x4 lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) lo[e] = (bf16_t)(v[e] - (float)o[e]);
                *reinterpret_cast<bf16x4*>(out + o_out + N + n) = lo;
              }
            }
          } else {
            *reinterpret_cast<f32x4*>(out + o_out + n) = v;
            if (out2) {
              // folded RMSNorm, producer side: the shadow carries the norm's gamma (the consumer applies 1 / rms per row) and
              // the row's sum of squares is left per 32 columns (8 lanes x 4 columns: a butterfly inside the lane octet)
              f32x4 gm = m >= p.nsw_row ? gmB : gmA;
              if constexpr (GAMF) {
                if constexpr (PIPE) {
                  if (gam_two && m >= m_sw) gm = m >= p.nsw_row ? gmD : gmC;
                }
                if (gam_row) {       // per-batch gamma, by row
                  int pos, nb = 0;
                  if constexpr (PIPE) row_pos(p0, m - m_base, rpb, true, pos, nb);
                  gm = *reinterpret_cast<const f32x4*>(ngam_b + (int64_t)(PIPE ? b0 + nb : m / rpb) * p.ngbs + (m >= p.nsw_row ? p.nsw_off : 0) + n);
                  if constexpr (PIPE) asm volatile("" : "+v"(gm));      // (as for the gate)
                }
              }
              bf16x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(v[e] * gm[e]);
              *reinterpret_cast<bf16x4*>(out2 + o_out2 + n) = o;
              if (p.out2_split) {      // bf16x3 mode: the lo plane of the (gamma-scaled) row, N columns further
                bf16x4 lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) lo[e] = (bf16_t)(v[e] * gm[e] - (float)o[e]);
                *reinterpret_cast<bf16x4*>(out2 + o_out2 + p.out2_lo + n) = lo;
              }
              if (p.ssq) {
                const float ss = octet_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
                if ((lane & 7) == 0) p.ssq[(int64_t)m * p.ssq_ld + (n >> 5)] = ss;
              }
            }
          }
          if constexpr (PIPE) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
}

template <int EPI, typename OutT, int TM, int TN, int WM, int WN, bool PF>
__device__ __forceinline__ void gemm_epilogue_lds(const GemmParams& p, f32x4 (&acc)[TM][TN], float* tile /* wave-private, 16 x (WN+4) floats */,
                                                  int m_base, int n_base, int lane, const EpiPrefetch<EPI, TM, WN, PF>& pf,
                                                  const float* rs_row = nullptr /* LDS: row scales of this wave's rows, or null */) {
  if constexpr (epi_pipelined<EPI, PF>()) {
    // wave-uniform: the wave tile lies wholly inside the problem, rows are dense
    if (__builtin_amdgcn_readfirstlane((int)(m_base + WM <= p.M && n_base + WN <= p.N)) && p.o_rowoff == nullptr)
      gemm_epilogue_lds_impl<EPI, OutT, TM, TN, WM, WN, PF, true>(p, acc, tile, m_base, n_base, lane, pf, rs_row);
    else
      gemm_epilogue_lds_impl<EPI, OutT, TM, TN, WM, WN, PF, false>(p, acc, tile, m_base, n_base, lane, pf, rs_row);
  } else {
    gemm_epilogue_lds_impl<EPI, OutT, TM, TN, WM, WN, PF, false>(p, acc, tile, m_base, n_base, lane, pf, rs_row);
  }
}

}  // namespace
