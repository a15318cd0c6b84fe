// Cross-attention of the audio stream with the context absorbed into the weights (bf16x3 mode, no rotary in cross-attention, bias-free
// to_q / to_k / to_v / to_out): for clip b, layer l, head h and key slot j
//   logits[n, h, j] = x[n, :] . Wqk[b,l][(h, j), :]       Wqk[(h, j), c] = sum_d K[b,j,l,h,d] * Wq[l][h*64 + d, c]
//   out[n, o]       = sum_{h, j} (P[n,h,j] * sigmoid(gate[n,h])) * Wvo[b,l][o, (h, j)]
//                                                          Wvo[o, (h, j)] = sum_d Wout[l][o, h*64 + d] * V[b,j,l,h,d]
// K and V of the context do not change over the evaluations of a sample() call, so Wqk and Wvo are formed ONCE per call
// (v2a_xattn_absorb_prepare, two launches for all clips, layers and heads) and an evaluation runs
//   v2a_xattn_absorbed   rows x (H*KP + H) x D split GEMM -> row scale, soft clamp, key mask, softmax over the KP key slots of each head,
//                        times sigmoid(gate logit + bias) of the head -> hi | lo planes of P * sigmoid(gate), (rows, H*KP)
//   v2a_gemm(GATE_RESID) rows x D x (H*KP), W = Wvo[b,l], one launch per clip
// instead of the q-projection, QK^T, PV over 64 head dimensions and the out-projection over H*64.  KP = key slots per head (16 or 32),
// slots nc .. KP-1 are zero rows / columns of the operands and masked like every slot >= kv_len[b].
//
// xattn_absorbed_kernel: a workgroup = 64 consecutive rows of ONE clip x 64 rows of Wqk = 64 / KP whole heads, with the gate rows of
// those heads: 4 waves, each 16 rows x all 64 columns.  K loop: the 64x64 split LDS-DMA ring of xattn_ring.h, XattnRing<true> (3 stages,
// counted vmcnt, one barrier per K tile; per 32 k three products A_lo W_hi + A_hi W_lo + A_hi W_hi), the product SWAPPED (W rows are the
// MFMA's rows, the token sits on the lane) so that the accumulators have the layout attn_weights of attn_core.h works on; plus one
// product per 32 k for the gate logits: the gate rows of the heads are preloaded into LDS by DMA ahead of the ring and read as a
// fragment whose row r is the gate row of head r % (64 / KP).  After the loop everything is lane-private: no LDS, no barrier.
#include "attn_core.h"
#include "xattn_ring.h"

namespace {

struct XaParams {
  GemmParams g;     // a[0] / lda[0] / K, w / ldw (rows 0 .. H*KP-1 = key slots, rows H*KP .. H*KP+H-1 = gates), bias = gate bias [H], M, rpb, rssq*
  int64_t wbs;      // elements from Wqk of one clip to the next
  bf16_t* out;      // hi | lo planes, the lo plane H*KP columns further
  int64_t ldo;
  const int32_t* kv_len;
  const int32_t* q_len;
  float scale, clamp;
  int32_t H, tiles_per_seq, nseq;
};

template <int CLAMP, int KP>
__global__ __launch_bounds__(256) void xattn_absorbed_kernel(XaParams P) {
  using Ring = XattnRing<true>;
  constexpr int BM = Ring::BM, BN = Ring::BN, NW = Ring::NW, TN = Ring::TN;
  constexpr int NH = BN / KP;                   // heads of a workgroup
  constexpr int NT = KP / 16;                   // 16-slot accumulator tiles of a head
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const GemmParams& p = P.g;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;

  // workgroup -> (row tile, column group): XCD x (blockIdx & 7) takes a contiguous chunk of the row-tile-fastest order
  const int tiles_m = P.nseq * P.tiles_per_seq;
  const int L = xcd_chunk_position(blockIdx.x, tiles_m * (P.H / NH));
  const int cg = L / tiles_m, tm = L - cg * tiles_m;
  const int b = tm / P.tiles_per_seq, t = tm - b * P.tiles_per_seq;
  const int rpb = p.rpb;
  const int m0 = b * rpb + t * BM;              // first row of the tile; rows of the tile beyond the sequence are clamped / dropped
  const int m_end = min((b + 1) * rpb, p.M);
  const int n0 = cg * BN;
  const int h0 = cg * NH;
  const char* wb = reinterpret_cast<const char*>(p.w) + (int64_t)b * P.wbs * 2;     // Wqk of this clip

  f32x4 acc[TN], accg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Ring ring(smem_raw, p, wb, m0, m_end, n0, wave, lane);          // W rows n0 .. n0 + 63 are key-slot rows: n0 + 63 < H * KP

  // ---- the gate rows of the NH heads, each [W_hi | W_lo] = 2 K contiguous elements, linear in LDS behind the ring, GPITCH bytes apart
  // (64 bytes of padding: the fragment reads of the four rows and the four k chunks of a lane group fall into different banks).
  // Issued ahead of the ring's DMAs, so every counted wait of the K loop retires them first.
  const int GPITCH = p.K * 4 + 64;
  char* gate_lds = smem_raw + Ring::RING_BYTES;
  {
    const int ngi = p.K >> 8;                 // 1024-byte wave instructions per gate row
    for (int i = wave; i < NH * ngi; i += NW) {
      const int gr = i / ngi, gc = i - gr * ngi;
      const char* gsrc = wb + ((int64_t)(P.H * KP + h0 + gr) * p.ldw) * 2 + gc * 1024 + lane * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                       (__attribute__((address_space(3))) void*)(gate_lds + gr * GPITCH + gc * 1024), 16, 0, 0);
    }
  }
  // folded RMSNorm (consumer): the rows' scales, behind the gate rows
  float* rs_lds = reinterpret_cast<float*>(gate_lds + NH * GPITCH);
  const bool scaled = p.rssq != nullptr;
  ring.start(p, scaled, m0, m_end, tid, rs_lds);

  const char* grow = gate_lds + (lr & (NH - 1)) * GPITCH + lq * 16;      // fragment row lr = the gate row of head h0 + lr % NH
  // one K tile: hi and lo fragments side by side, the next tile's DMAs, then the products
  ring.k_loop([&](auto stage, int kt) {
    bf16x8 af[2], bf[2][TN], gf[2], afl[2], bfl[2][TN], gfl[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      af[kk] = ring.a_frag(stage, 0, kk);
      afl[kk] = ring.a_frag(stage, 1, kk);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bf[kk][j] = ring.w_frag(stage, 0, kk, j);
        bfl[kk][j] = ring.w_frag(stage, 1, kk, j);
      }
      gf[kk] = *reinterpret_cast<const bf16x8*>(grow + (kt * 64 + kk * 32) * 2);
      gfl[kk] = *reinterpret_cast<const bf16x8*>(grow + (p.K + kt * 64 + kk * 32) * 2);
    }
    ring.refill(stage, kt);
    // three products per fragment pair, small terms first (the order of gemm_bf16_dma_kernel<.., S3>); W supplies the MFMA's rows
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[kk][j], afl[kk], acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfl[kk][j], af[kk], acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[kk][j], af[kk], acc[j], 0, 0, 0);
      }
      accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[kk], afl[kk], accg, 0, 0, 0);
      accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfl[kk], af[kk], accg, 0, 0, 0);
      accg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[kk], af[kk], accg, 0, 0, 0);
    }
  });

  // ---- lane-private from here: register jj of acc[j] is row n0 + 16 j + 4 lq + jj of Wqk for token lr of the wave, i.e. key slot
  // 16 (j % NT) + 4 lq + jj of head h0 + j / NT (the geometry of attn_core.h with g = lq); register jj of accg is the gate logit of
  // head h0 + jj % NH
  const int qrow = wave * 16 + lr;                 // tile row of this lane's token
  const int qi = t * BM + qrow;                    // its index in the sequence
  const bool live = m0 + qrow < m_end;             // rows of the tile beyond the clip computed a copy of its last row: not stored
  const float rs = scaled ? rs_lds[qrow] : 1.0f;
  const int kvn = min(P.kv_len[b], KP);
  const AttnLogitScale sc = attn_logit_scale(P.scale, P.clamp);
  const int hkp = P.H * KP;
  bf16_t* orow = P.out + (int64_t)(m0 + qrow) * P.ldo + n0 + 4 * lq;
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    f32x4 s[NT], o[4];
    float l = 0.f, m = 0.f;                        // one key tile: no running maximum, attn_weights<.., false> leaves m, l and o alone
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) s[tt] = scaled ? acc[hh * NT + tt] * rs : acc[hh * NT + tt];
    if (kvn > 0) {
      attn_weights<CLAMP, false>(s, m, l, o, 0, kvn, lq, sc);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int j = 0; j < 4; ++j) l += s[tt][j];
    } else {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) s[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    float gv = accg[hh] * rs;
    if (p.bias) gv += p.bias[h0 + hh];
    const float f = attn_out_factor(P.q_len, b, rpb, qi, l, sigmoid_f(gv));
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      bf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = s[tt][e] * f;
        asm volatile("" : "+v"(v));                // the planes split the rounded product (attn_store_split)
        hi[e] = (bf16_t)v;
        lo[e] = (bf16_t)(v - (float)hi[e]);
      }
      if (live) {
        *reinterpret_cast<bf16x4*>(orow + (hh * NT + tt) * 16) = hi;
        *reinterpret_cast<bf16x4*>(orow + hkp + (hh * NT + tt) * 16) = lo;
      }
    }
  }
}

template <int CLAMP, int KP>
int launch_xa(const XaParams& P, hipStream_t s) {
  constexpr int NH = 64 / KP;                    // gate rows of a workgroup, GPITCH = 4 K + 64 bytes apart; the entry point accepts K <= 2048
  static std::atomic<uint64_t> lds_set{0};
  return xattn_ring_launch<true, NH * (2048 * 4 + 64)>(xattn_absorbed_kernel<CLAMP, KP>, P, P.nseq * P.tiles_per_seq * (P.H / NH),
                                                       (size_t)NH * (P.g.K * 4 + 64), lds_set, "v2a_xattn_absorbed", s);
}

// ---- once per sample(): the absorbed operands -------------------------------------------------------------------------------------
struct XpParams {
  const float* kv;          // context K / V rows: row b * nc + j, K of layer l at column k_col + l * H * 64, V at v_col + l * H * 64
  int64_t kv_ld;
  int32_t k_col, v_col;
  const float* wq;          // [L][H*64 + H][D]: to_q rows, then the head-gate rows
  const float* wo;          // [L][D][H*64]
  bf16_t* wqk;              // [B][L][H*KP + H][D hi | D lo]
  bf16_t* wvo;              // [B][L][D][H*KP hi | H*KP lo]
  int32_t B, L, H, D, nc;
};

__device__ __forceinline__ void xp_split(float v, bf16_t& hi, bf16_t& lo) {
  hi = (bf16_t)v;
  lo = (bf16_t)(v - (float)hi);
}

// Wqk: block = 256 columns c x one head (blockIdx.y < H) of one (clip, layer); thread = one column, KP fma chains over d = 0 .. 63 in
// order.  blockIdx.y == H: the gate rows, the planes of the fp32 gate weights themselves.
template <int KP>
__global__ __launch_bounds__(256) void absorb_wqk_kernel(XpParams P) {
  __shared__ __attribute__((aligned(16))) float ks[KP][64];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * 256 + tid;
  const int h = blockIdx.y;
  const int b = blockIdx.z / P.L, l = blockIdx.z - b * P.L;
  const int inner = P.H * 64, D = P.D;
  const int64_t nrow = (int64_t)P.H * KP + P.H;
  bf16_t* wout = P.wqk + ((int64_t)b * P.L + l) * nrow * 2 * D;
  const float* wl = P.wq + (int64_t)l * (inner + P.H) * D;
  if (h == P.H) {
    if (c < D)
      for (int g = 0; g < P.H; ++g) {
        bf16_t hi, lo;
        xp_split(wl[(int64_t)(inner + g) * D + c], hi, lo);
        bf16_t* o = wout + ((int64_t)P.H * KP + g) * 2 * D;
        o[c] = hi;
        o[D + c] = lo;
      }
    return;
  }
  for (int i = tid; i < KP * 64; i += 256) {
    const int j = i >> 6, d = i & 63;
    ks[j][d] = j < P.nc ? P.kv[((int64_t)b * P.nc + j) * P.kv_ld + P.k_col + l * inner + h * 64 + d] : 0.f;
  }
  __syncthreads();
  if (c >= D) return;
  float acc[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) acc[j] = 0.f;
  const float* wp = wl + (int64_t)h * 64 * D + c;
  for (int d4 = 0; d4 < 16; ++d4) {
    float w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = wp[(int64_t)(d4 * 4 + e) * D];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(&ks[j][d4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j] = fmaf(k4[e], w[e], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    bf16_t hi, lo;
    xp_split(acc[j], hi, lo);
    bf16_t* o = wout + ((int64_t)h * KP + j) * 2 * D;
    o[c] = hi;
    o[D + c] = lo;
  }
}

// Wvo: block = 64 output rows o x one head of one (clip, layer); thread = one row x KP / 4 key slots, fma chains over d in order
template <int KP>
__global__ __launch_bounds__(256) void absorb_wvo_kernel(XpParams P) {
  constexpr int JT = KP / 4;
  __shared__ float ws[64][65];
  __shared__ float vs[KP][64];
  const int tid = threadIdx.x;
  const int o0 = blockIdx.x * 64;
  const int h = blockIdx.y;
  const int b = blockIdx.z / P.L, l = blockIdx.z - b * P.L;
  const int inner = P.H * 64, D = P.D;
  const int hkp = P.H * KP;
  for (int i = tid; i < 64 * 64; i += 256) {
    const int oo = i >> 6, d = i & 63;
    ws[oo][d] = o0 + oo < D ? P.wo[((int64_t)l * D + o0 + oo) * inner + h * 64 + d] : 0.f;
  }
  for (int i = tid; i < KP * 64; i += 256) {
    const int j = i >> 6, d = i & 63;
    vs[j][d] = j < P.nc ? P.kv[((int64_t)b * P.nc + j) * P.kv_ld + P.v_col + l * inner + h * 64 + d] : 0.f;
  }
  __syncthreads();
  const int oo = tid & 63, jq = tid >> 6;
  if (o0 + oo >= D) return;
  float acc[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) acc[j] = 0.f;
  for (int d = 0; d < 64; ++d) {
    float w = ws[oo][d];
    asm volatile("" : "+v"(w));           // a register of its own: read as the high half of a loaded pair, w made the packed FMAs take the
                                          // high-half broadcast form tests/test_isa_guard.py forbids
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[j] = fmaf(w, vs[jq * JT + j][d], acc[j]);
  }
  bf16_t* o = P.wvo + (((int64_t)b * P.L + l) * D + o0 + oo) * 2 * hkp + h * KP + jq * JT;
#pragma unroll
  for (int j4 = 0; j4 < JT; j4 += 4) {
    bf16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bf16_t a, c;
      xp_split(acc[j4 + e], a, c);
      hi[e] = a;
      lo[e] = c;
    }
    *reinterpret_cast<bf16x4*>(o + j4) = hi;
    *reinterpret_cast<bf16x4*>(o + hkp + j4) = lo;
  }
}

template <int KP>
int launch_xp(const XpParams& P, hipStream_t s) {
  hipLaunchKernelGGL(absorb_wqk_kernel<KP>, dim3((P.D + 255) / 256, P.H + 1, P.B * P.L), dim3(256), 0, s, P);
  if (int rc = v2a_check_launch("v2a_xattn_absorb_prepare (Wqk)")) return rc;
  hipLaunchKernelGGL(absorb_wvo_kernel<KP>, dim3((P.D + 63) / 64, P.H, P.B * P.L), dim3(256), 0, s, P);
  return v2a_check_launch("v2a_xattn_absorb_prepare (Wvo)");
}

}  // namespace

extern "C" int v2a_xattn_absorb_prepare(const v2a_xattn_prepare_args* a, v2a_stream_t stream) {
  V2A_REQUIRE(a != nullptr, "v2a_xattn_absorb_prepare: null args");
  V2A_REQUIRE(a->B > 0 && a->L > 0 && a->H > 0 && a->D > 0 && a->nc > 0 && (a->KP == 16 || a->KP == 32) && a->nc <= a->KP,
              "v2a_xattn_absorb_prepare: B=%d L=%d H=%d D=%d nc=%d KP=%d (KP 16 or 32, nc <= KP)", a->B, a->L, a->H, a->D, a->nc, a->KP);
  V2A_REQUIRE((int64_t)a->B * a->L <= 65535 && a->H < 65535, "v2a_xattn_absorb_prepare: B * L = %lld exceeds the grid", (long long)a->B * a->L);
  V2A_REQUIRE(a->ctx_kv && a->wq && a->wo && a->wqk && a->wvo && ((uintptr_t)a->wvo & 7) == 0, "v2a_xattn_absorb_prepare: null or misaligned buffer");
  V2A_REQUIRE(a->k_col >= 0 && a->v_col >= 0 && a->ctx_ld >= (int64_t)(a->k_col > a->v_col ? a->k_col : a->v_col) + (int64_t)a->L * a->H * 64,
              "v2a_xattn_absorb_prepare: context rows of %lld floats do not hold L * H * 64 columns from k_col=%d / v_col=%d", (long long)a->ctx_ld,
              a->k_col, a->v_col);
  XpParams P{};
  P.kv = a->ctx_kv;
  P.kv_ld = a->ctx_ld;
  P.k_col = a->k_col;
  P.v_col = a->v_col;
  P.wq = a->wq;
  P.wo = a->wo;
  P.wqk = reinterpret_cast<bf16_t*>(a->wqk);
  P.wvo = reinterpret_cast<bf16_t*>(a->wvo);
  P.B = a->B; P.L = a->L; P.H = a->H; P.D = a->D; P.nc = a->nc;
  hipStream_t s = (hipStream_t)stream;
  return a->KP == 16 ? launch_xp<16>(P, s) : launch_xp<32>(P, s);
}

extern "C" int v2a_xattn_absorbed(const v2a_xattn_absorbed_args* a, v2a_stream_t stream) {
  V2A_REQUIRE(a != nullptr, "v2a_xattn_absorbed: null args");
  V2A_REQUIRE(a->H > 0 && a->B > 0 && a->rows_per_batch > 0 && (a->KP == 16 || a->KP == 32) && (a->H * a->KP) % 64 == 0,
              "v2a_xattn_absorbed: H=%d B=%d rows_per_batch=%d KP=%d (KP 16 or 32, H * KP a multiple of 64)", a->H, a->B, a->rows_per_batch, a->KP);
  const int K = a->K;
  V2A_REQUIRE(K > 0 && K % 512 == 0 && K <= 2048, "v2a_xattn_absorbed: K=%d must be a multiple of 512, <= 2048", K);
  V2A_REQUIRE(a->M > 0 && (int64_t)a->M <= (int64_t)a->B * a->rows_per_batch && (int64_t)a->M > (int64_t)(a->B - 1) * a->rows_per_batch,
              "v2a_xattn_absorbed: M=%d rows do not end in clip B-1 (B=%d, rows_per_batch=%d)", a->M, a->B, a->rows_per_batch);
  const int hkp = a->H * a->KP;
  V2A_REQUIRE(a->a && ((uintptr_t)a->a & 15) == 0 && a->lda % 8 == 0 && a->lda >= 2 * (int64_t)K && a->wqk && ((uintptr_t)a->wqk & 15) == 0 &&
                  a->ldw % 8 == 0 && a->ldw >= 2 * (int64_t)K && a->w_batch_stride % 8 == 0 &&
                  (a->B == 1 || a->w_batch_stride >= (int64_t)(hkp + a->H) * a->ldw - (a->ldw - 2 * (int64_t)K)),
              "v2a_xattn_absorbed: A / Wqk rows must be 16-byte aligned and hold 2 K elements, Wqk of a clip H*KP + H rows");
  // the DMA addresses a row as a 32-bit byte offset from the operand's base
  V2A_REQUIRE((int64_t)a->M * a->lda * 2 < ((int64_t)1 << 32) && (int64_t)(hkp + a->H) * a->ldw * 2 < ((int64_t)1 << 32),
              "v2a_xattn_absorbed: operand larger than 4 GB");
  V2A_REQUIRE(a->out && ((uintptr_t)a->out & 7) == 0 && a->ldo % 4 == 0 && a->ldo >= 2 * (int64_t)hkp,
              "v2a_xattn_absorbed: out rows must be 8-byte aligned and hold 2 * H * KP bf16");
  V2A_REQUIRE(a->kv_len != nullptr, "v2a_xattn_absorbed: kv_len is required (the padding slots are masked through it)");
  XaParams P{};
  GemmParams& p = P.g;
  xattn_ring_params(p, a->a, a->lda, a->wqk, a->ldw, a->gate_bias, a->M, hkp, K, a->rows_per_batch);
  if (int rc = v2a_detail::fill_row_scale(p, a->row_ssq, a->ld_row_ssq, a->row_ssq_parts, a->row_norm_dim, "v2a_xattn_absorbed")) return rc;
  P.wbs = a->w_batch_stride;
  P.out = reinterpret_cast<bf16_t*>(a->out);
  P.ldo = a->ldo;
  P.kv_len = a->kv_len;
  P.q_len = a->q_len;
  P.scale = a->scale;
  P.clamp = a->softclamp;
  P.H = a->H;
  P.nseq = a->B;
  P.tiles_per_seq = (a->rows_per_batch + 63) / 64;
  hipStream_t s = (hipStream_t)stream;
  const bool kp16 = a->KP == 16;
  return attn_with_clamp(attn_clamp_mode(a->softclamp, a->KP), [&](auto c) {
    return kp16 ? launch_xa<decltype(c)::value, 16>(P, s) : launch_xa<decltype(c)::value, 32>(P, s);
  });
}
