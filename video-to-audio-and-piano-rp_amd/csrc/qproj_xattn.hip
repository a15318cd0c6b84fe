// Cross-attention of the audio stream as ONE launch: q-projection GEMM (+ folded RMSNorm, bias, RoPE) -> QK^T over the nc <= 64
// context keys of the clip -> soft clamp, softmax -> PV -> per-head sigmoid gate -> bf16 output rows for the out-projection.
// Replaces, at the sizes where the two launches were latency bound (one or two clips per GPU), v2a_gemm(STORE, rope) into the
// [q | gate] buffer followed by v2a_attention: xt Attention.forward with context, x3:1126 (call site), attend.py via x3:881-914.
//
// A workgroup = 64 consecutive tokens of ONE sequence x ONE head (64 q columns): 4 waves, each 16 tokens x all 64 head
// dimensions, so everything after the K loop is wave-private except the shared K / V tile.
//   K loop     the 64x64 LDS-DMA ring of xattn_ring.h (3 stages, counted vmcnt, one barrier per K tile), wave tile 16x64, plus ONE
//              extra MFMA per 32-k step for the head's gate logit: the gate row of W (row H*64 + h) is preloaded into LDS
//              (2 KB, by LDS-DMA ahead of the ring) and read as a B fragment whose 16 columns all hold that row -- the
//              accumulator then carries the logit of each of the wave's 16 tokens with the arithmetic of the plain GEMM.
//   epilogue   acc -> wave-private fp32 slab -> row pieces: x row scale, + bias, RoPE (rope_rotate4 of gemm_common.h, as
//              gemm_epilogue_lds applies it), bf16, so q equals the unfused launch's bit for bit -> wave-private swizzled q tile in
//              LDS; K / V rows of the head (requested when the kernel starts) -> shared swizzled tiles; then one key tile of
//              attn_mfma_kernel (swapped product: the query sits on the lane) through the functions of attn_core.h that the kernels
//              of attention.hip call -- attn_weights, attn_pack_weights, attn_vt_frag, attn_out_factor, attn_store -- and 8-byte
//              stores of O * sigmoid(gate) / l.
// Results equal the two-launch path bit for bit (tests/test_kernels_gpu.py::test_qproj_xattn_equals_two_launches).
// S3 = the bf16x3 mode's arithmetic: hi | lo bf16 planes of A, W, q, K, V and P, three MFMAs per product (XattnRing<true>, in the
// product order of gemm.hip's split ring; split8, the three-product order and attn_store_split of attn_mfma_split_kernel), fp32 K / V
// rows and gate logit, output rows as hi | lo planes for the out-projection's split GEMM.
#include "attn_core.h"
#include "xattn_ring.h"

namespace {

struct QxParams {
  GemmParams g;     // a[0] / lda[0] / K, w / ldw (rows 0 .. H*64-1 = q, rows H*64 .. H*64+H-1 = gates), bias, M, rpb, rope*, rssq*
  const void* k;        // bf16 rows, or fp32 rows (S3)
  const void* v;
  bf16_t* out;          // bf16 rows; S3: hi | lo planes, the lo plane H*64 columns further
  int64_t krs, vrs, ors, kbs, vbs, obs;
  const int32_t* kv_len;
  const int32_t* q_len;
  float scale, clamp;
  int32_t H, Nk, tiles_per_seq, nseq;
};

template <int CLAMP, bool S3>
__global__ __launch_bounds__(256) void qproj_xattn_kernel(QxParams P) {
  using Ring = XattnRing<S3>;
  constexpr int BM = Ring::BM, BN = Ring::BN, NW = Ring::NW, TN = Ring::TN;
  constexpr int SLAB = 16 * (BN + 4) * 4;       // bytes of a wave's fp32 staging slab
  constexpr int TILE = 64 * 128;                // one bf16 64x64 tile
  constexpr int NPL = Ring::NPL;                // planes of q, K and V
  constexpr int Q_OFF = NW * SLAB, K_OFF = Q_OFF + NPL * TILE, V_OFF = K_OFF + NPL * TILE, G_OFF = V_OFF + NPL * TILE;
  static_assert(G_OFF + 64 * 4 <= Ring::RING_BYTES, "post-loop regions alias the ring");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const GemmParams& p = P.g;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;

  // workgroup -> (row tile, head): XCD x (blockIdx & 7) takes a contiguous chunk of the row-tile-fastest order, i.e. ~2 heads'
  // W panels and every A panel (3.7 MB for one clip) per L2
  const int tiles_m = P.nseq * P.tiles_per_seq;
  const int L = xcd_chunk_position(blockIdx.x, tiles_m * P.H);
  const int h = L / tiles_m, tm = L - h * tiles_m;
  const int b = tm / P.tiles_per_seq, t = tm - b * P.tiles_per_seq;
  const int rpb = p.rpb;
  const int m0 = b * rpb + t * BM;              // first row of the tile; rows of the tile beyond the sequence are clamped / dropped
  const int m_end = min((b + 1) * rpb, p.M);
  const int n0 = h * BN;

  // ---- K / V rows of this (sequence, head): requested first, parked in registers until the ring memory is free
  const int kchunk = tid & 7, krow = tid >> 3;
  struct Raw { f32x4 a, b; };
  bf16x8 kreg[S3 ? 1 : 2], vreg[S3 ? 1 : 2];
  Raw kraw[S3 ? 2 : 1], vraw[S3 ? 2 : 1];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int key = krow + 32 * i;
    key = key < P.Nk ? key : P.Nk - 1;
    if constexpr (S3) {
      const float* kpz = reinterpret_cast<const float*>(P.k) + b * P.kbs + h * 64 + (int64_t)key * P.krs + kchunk * 8;
      const float* vpz = reinterpret_cast<const float*>(P.v) + b * P.vbs + h * 64 + (int64_t)key * P.vrs + kchunk * 8;
      kraw[i].a = *reinterpret_cast<const f32x4*>(kpz);
      kraw[i].b = *reinterpret_cast<const f32x4*>(kpz + 4);
      vraw[i].a = *reinterpret_cast<const f32x4*>(vpz);
      vraw[i].b = *reinterpret_cast<const f32x4*>(vpz + 4);
    } else {
      kreg[i] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(P.k) + b * P.kbs + h * 64 + (int64_t)key * P.krs + kchunk * 8);
      vreg[i] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(P.v) + b * P.vbs + h * 64 + (int64_t)key * P.vrs + kchunk * 8);
    }
  }

  f32x4 acc[TN], accg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Ring ring(smem_raw, p, p.w, m0, m_end, n0, wave, lane);          // W rows n0 .. n0 + 63 are q rows: n0 + 63 < H * 64

  // ---- the head's gate row of W, linear in LDS behind the ring: K * 2 bytes = K / 512 wave-instructions.  Issued ahead of the
  // ring's DMAs, so every counted wait of the K loop retires them first.
  char* gate_lds = smem_raw + Ring::RING_BYTES;
  {
    // S3: the row is [W_hi | W_lo], 2 K contiguous elements: the same linear copy, twice as long
    const char* gsrc = reinterpret_cast<const char*>(p.w) + ((int64_t)(P.H * 64 + h) * p.ldw) * 2 + lane * 16;
    const int ngi = (p.K >> 9) * NPL;
    for (int i = wave; i < ngi; i += NW)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc + i * 1024),
                                       (__attribute__((address_space(3))) void*)(gate_lds + i * 1024), 16, 0, 0);
  }
  // folded RMSNorm (consumer): the rows' scales, behind the gate row
  float* rs_lds = reinterpret_cast<float*>(gate_lds + p.K * 2 * NPL);
  const bool scaled = p.rssq != nullptr;
  ring.start(p, scaled, m0, m_end, tid, rs_lds);

  // one K tile: hi fragments, (S3) lo fragments, the next tile's DMAs, then the products
  ring.k_loop([&](auto stage, int kt) {
    bf16x8 af[2], bf[2][TN], gf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      af[kk] = ring.a_frag(stage, 0, kk);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[kk][j] = ring.w_frag(stage, 0, kk, j);
      gf[kk] = *reinterpret_cast<const bf16x8*>(gate_lds + (kt * 64 + kk * 32 + lq * 8) * 2);     // the same row for all 16 columns
    }
    if constexpr (S3) {
      bf16x8 afl[2], bfl[2][TN], gfl[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        afl[kk] = ring.a_frag(stage, 1, kk);
#pragma unroll
        for (int j = 0; j < TN; ++j) bfl[kk][j] = ring.w_frag(stage, 1, kk, j);
        gfl[kk] = *reinterpret_cast<const bf16x8*>(gate_lds + (p.K + kt * 64 + kk * 32 + lq * 8) * 2);
      }
      ring.refill(stage, kt);
      // three products per fragment pair, small terms first (the order of gemm_bf16_dma_kernel<.., S3>)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afl[kk], bf[kk][j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], bfl[kk][j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], bf[kk][j], acc[j], 0, 0, 0);
        }
        accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afl[kk], gf[kk], accg, 0, 0, 0);
        accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], gfl[kk], accg, 0, 0, 0);
        accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], gf[kk], accg, 0, 0, 0);
      }
    } else {
      ring.refill(stage, kt);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], bf[kk][j], acc[j], 0, 0, 0);
        accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk], gf[kk], accg, 0, 0, 0);
      }
    }
  });
  __builtin_amdgcn_s_barrier();      // every wave is done reading the ring; all DMAs were retired by the last counted wait

  // ---- K / V tiles into the dead ring (row-major [key][64], 16-B chunk XOR-swizzled by key & 7, as in attn_mfma_kernel)
  bf16_t* ks = reinterpret_cast<bf16_t*>(smem_raw + K_OFF);      // S3: hi plane, the lo plane one tile further
  bf16_t* vt = reinterpret_cast<bf16_t*>(smem_raw + V_OFF);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = krow + 32 * i;
    const int off = row * 64 + ((kchunk ^ (row & 7)) << 3);
    if constexpr (S3) {
      bf16x8 hi, lo;
      split8(kraw[i].a, kraw[i].b, hi, lo);
      *reinterpret_cast<bf16x8*>(ks + off) = hi;
      *reinterpret_cast<bf16x8*>(ks + 64 * 64 + off) = lo;
      split8(vraw[i].a, vraw[i].b, hi, lo);
      *reinterpret_cast<bf16x8*>(vt + off) = hi;
      *reinterpret_cast<bf16x8*>(vt + 64 * 64 + off) = lo;
    } else {
      *reinterpret_cast<bf16x8*>(ks + off) = kreg[i];
      *reinterpret_cast<bf16x8*>(vt + off) = vreg[i];
    }
  }
  // ---- q rows of this wave: the STORE epilogue of gemm_epilogue_lds (row scale, bias, RoPE, bf16) into a swizzled LDS tile
  float* slab = reinterpret_cast<float*>(smem_raw + wave * SLAB);
  bf16_t* qt = reinterpret_cast<bf16_t*>(smem_raw + Q_OFF);
  float* gl = reinterpret_cast<float*>(smem_raw + G_OFF);
  constexpr int LD = BN + 4;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) slab[(lq * 4 + jj) * LD + j * 16 + lr] = acc[j][jj];
  if (lr == 0) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) gl[wave * 16 + lq * 4 + jj] = accg[jj];
  }
  {
    const int c4 = (lane & 15) * 4, r0 = lane >> 4;
    const int n = n0 + c4;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n);
    const bool rope = p.rope && n < p.rope_cols;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + q * 4;
      const int row = wave * 16 + r;
      int m = m0 + row;
      m = m < m_end ? m : m_end - 1;
      f32x4 v = *reinterpret_cast<const f32x4*>(slab + r * LD + c4);
      if (scaled) v *= rs_lds[row];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += bv[e];
      if (rope) rope_rotate4(v, *reinterpret_cast<const f32x4*>(p.rope + ((int64_t)(p.rope_pos_off + m % rpb) * 32 + ((n & 63) >> 1)) * 2));
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
      bf16_t* qd = qt + row * 64 + (((c4 >> 3) ^ (row & 7)) << 3) + (c4 & 7);
      *reinterpret_cast<bf16x4*>(qd) = o;
      if constexpr (S3) {        // the fp32 q of the unfused launch, split as attn_mfma_split_kernel splits it
        bf16x4 lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = (bf16_t)(v[e] - (float)o[e]);
        *reinterpret_cast<bf16x4*>(qd + 64 * 64) = lo;
      }
    }
  }
  __syncthreads();                     // K / V tiles, q tile and gate logits visible

  // ---- single-tile attention of the wave's 16 queries (attn_mfma_kernel<1, CLAMP> / attn_mfma_split_kernel<1, CLAMP> with one key tile)
  const int g = lq;
  const int qrow = wave * 16 + lr;                 // tile row of this lane's query
  const int qi = t * BM + qrow;                    // its index in the sequence
  bf16x8 qf[2], ql[S3 ? 2 : 1];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int off = qrow * 64 + (((kk * 4 + g) ^ (qrow & 7)) << 3);
    qf[kk] = *reinterpret_cast<const bf16x8*>(qt + off);
    if constexpr (S3) ql[kk] = *reinterpret_cast<const bf16x8*>(qt + 64 * 64 + off);
  }
  const int kvn = P.kv_len ? min(P.kv_len[b], P.Nk) : P.Nk;
  const AttnLogitScale sc = attn_logit_scale(P.scale, P.clamp);
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float l = 0.f, m = 0.f;                          // one key tile: no running maximum, attn_weights<.., false> leaves m, l and o alone
  if (kvn > 0) {
    f32x4 s[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      s[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int row = 16 * tt + lr;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int off = row * 64 + (((kk * 4 + g) ^ (row & 7)) << 3);
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + off);
        if constexpr (S3) {
          const bf16x8 kl = *reinterpret_cast<const bf16x8*>(ks + 64 * 64 + off);
          s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qf[kk], s[tt], 0, 0, 0);
          s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, ql[kk], s[tt], 0, 0, 0);
        }
        s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[tt], 0, 0, 0);
      }
    }
    // soft clamp, key mask, softmax weights (fp32) in s; row sum and the P^T operand (S3: hi | lo planes of the fp32 weights)
    attn_weights<CLAMP, false>(s, m, l, o, 0, kvn, g, sc);
    bf16x8 pf[NPL][2];
    attn_pack_weights(s, l, pf);
    // O^T += V^T P^T
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const bf16x8 vf = attn_vt_frag(vt, ks2, dt, g, lr);
        if constexpr (S3) {
          const bf16x8 vfl = attn_vt_frag(vt + 64 * 64, ks2, dt, g, lr);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfl, pf[0][ks2], o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][ks2], o[dt], 0, 0, 0);
        }
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][ks2], o[dt], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (m0 + qrow >= m_end) return;
  // gate logit of this query: the GEMM's STORE epilogue (row scale, bias; bf16 mode: the bf16 rounding of the [q | gate] buffer), then sigmoid
  float gv = gl[qrow];
  if (scaled) gv *= rs_lds[qrow];
  if (p.bias) gv += p.bias[P.H * 64 + h];
  const float gt = S3 ? sigmoid_f(gv) : sigmoid_f((float)(bf16_t)gv);
  const float f = attn_out_factor(P.q_len, b, rpb, qi, l, gt);
  bf16_t* op = P.out + b * P.obs + (int64_t)qi * P.ors + h * 64 + 4 * g;
  if constexpr (S3) attn_store_split(op, P.H * 64, o, f);
  else attn_store(op, o, f);
}

template <int CLAMP, bool S3>
int launch_qx(const QxParams& P, hipStream_t s) {
  constexpr size_t row = 2 * (S3 ? 2 : 1);       // bytes of the gate row per k; the entry point accepts K <= 4096
  static std::atomic<uint64_t> lds_set{0};
  return xattn_ring_launch<S3, 4096 * row>(qproj_xattn_kernel<CLAMP, S3>, P, P.nseq * P.tiles_per_seq * P.H, P.g.K * row, lds_set, "v2a_qproj_xattn", s);
}

}  // namespace

extern "C" int v2a_qproj_xattn(const v2a_gemm_args* a, const v2a_attn_args* at, v2a_stream_t stream) {
  V2A_REQUIRE(a != nullptr && at != nullptr, "v2a_qproj_xattn: null args");
  const bool s3 = a->a_dtype == V2A_BF16_SPLIT;          // the bf16x3 mode: split operands, fp32 K / V, hi | lo output planes
  V2A_REQUIRE(a->nseg == 1 && a->a[0] && (a->a_dtype == V2A_BF16 || s3) && a->compute_dtype == V2A_BF16 && a->epilogue == V2A_EPI_STORE,
              "v2a_qproj_xattn: one bf16 (or split bf16) A segment, bf16 compute, STORE epilogue");
  V2A_REQUIRE(s3 ? (at->dtype == V2A_BF16_SPLIT && at->out_split) : (at->dtype == V2A_BF16 && !at->out_split),
              "v2a_qproj_xattn: bf16 operands go with dtype V2A_BF16, split operands with V2A_BF16_SPLIT and out_split");
  V2A_REQUIRE(at->H > 0 && at->B > 0 && at->Nq > 0 && at->Nk > 0 && at->Nk <= 64, "v2a_qproj_xattn: H=%d B=%d Nq=%d Nk=%d (Nk <= 64)", at->H, at->B, at->Nq, at->Nk);
  const int K = a->ka[0];
  V2A_REQUIRE(K > 0 && K % 512 == 0 && K <= 4096, "v2a_qproj_xattn: K=%d must be a multiple of 512, <= 4096", K);
  V2A_REQUIRE(a->N >= at->H * 65 && a->M == at->B * at->Nq && a->rows_per_batch == at->Nq,
              "v2a_qproj_xattn: W holds H*64 q rows + H gate rows (N=%d, H=%d); M=%d rows = B*Nq = %d*%d, rows_per_batch=%d", a->N, at->H, a->M,
              at->B, at->Nq, a->rows_per_batch);
  const int pl = s3 ? 2 : 1;
  V2A_REQUIRE(((uintptr_t)a->a[0] & 15) == 0 && a->lda[0] % 8 == 0 && a->lda[0] >= (int64_t)pl * K && a->w && ((uintptr_t)a->w & 15) == 0 &&
                  a->ldw % 8 == 0 && a->ldw >= (int64_t)pl * K,
              "v2a_qproj_xattn: A / W rows must be 16-byte aligned and hold K (split: 2 K) elements");
  V2A_REQUIRE(!a->bias || ((uintptr_t)a->bias & 15) == 0, "v2a_qproj_xattn: bias not 16-byte aligned");
  V2A_REQUIRE(!a->a_row_offset && !a->a_ktile_offset && !a->out_row_offset && !a->relu && !a->out_bf16 && !a->norm_gamma && !a->norm_ssq,
              "v2a_qproj_xattn: no offset tables, relu, shadow or norm producer");
  V2A_REQUIRE(at->k && at->v && at->out && (((uintptr_t)at->k | (uintptr_t)at->v) & 15) == 0 && ((uintptr_t)at->out & 7) == 0 &&
                  at->k_row_stride % 8 == 0 && at->v_row_stride % 8 == 0 && at->k_batch_stride % 8 == 0 && at->v_batch_stride % 8 == 0 &&
                  at->out_row_stride % 4 == 0 && at->out_batch_stride % 4 == 0 && (!s3 || at->out_row_stride >= 2 * (int64_t)at->H * 64),
              "v2a_qproj_xattn: k / v head slices must be 16-byte aligned, out rows 8-byte aligned (split: 2 * H * 64 bf16 per row)");
  QxParams P{};
  GemmParams& p = P.g;
  xattn_ring_params(p, a->a[0], a->lda[0], a->w, a->ldw, a->bias, a->M, at->H * 64, K, a->rows_per_batch);
  p.rope = a->rope_table;
  p.rope_cols = a->rope_cols;
  p.rope_pos_off = a->rope_pos_offset;
  if (a->rope_table)
    V2A_REQUIRE(a->rope_cols % 64 == 0 && a->rope_cols <= at->H * 64 && ((uintptr_t)a->rope_table & 15) == 0, "v2a_qproj_xattn: rope_cols %d", a->rope_cols);
  if (int rc = v2a_detail::fill_row_scale(p, a->row_ssq, a->ld_row_ssq, a->row_ssq_parts, a->row_norm_dim, "v2a_qproj_xattn")) return rc;
  P.k = at->k;
  P.v = at->v;
  P.out = reinterpret_cast<bf16_t*>(at->out);
  P.krs = at->k_row_stride; P.vrs = at->v_row_stride; P.ors = at->out_row_stride;
  P.kbs = at->k_batch_stride; P.vbs = at->v_batch_stride; P.obs = at->out_batch_stride;
  P.kv_len = at->kv_len;
  P.q_len = at->q_len;
  P.scale = at->scale;
  P.clamp = at->softclamp;
  P.H = at->H;
  P.Nk = at->Nk;
  P.nseq = at->B;
  P.tiles_per_seq = (at->Nq + 63) / 64;
  hipStream_t s = (hipStream_t)stream;
  // the clamp mode v2a_attention would pick for these keys
  return attn_with_clamp(attn_clamp_mode(at->softclamp, at->Nk), [&](auto c) {
    return s3 ? launch_qx<decltype(c)::value, true>(P, s) : launch_qx<decltype(c)::value, false>(P, s);
  });
}
