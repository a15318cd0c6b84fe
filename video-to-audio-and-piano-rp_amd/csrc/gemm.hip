// MFMA GEMM with fused epilogues for gfx950:  acc[m][n] = sum_k A[m][k] * W[n][k].
//
// Both operands are K-contiguous (activations row-major, nn.Linear weights [N][K]), which
// is exactly the MFMA A/B fragment order, so no transposes are needed anywhere.
//   bf16 : v_mfma_f32_16x16x32_bf16, BK = 64, LDS rows of 128 B with the 16-B chunk index
//          XOR-swizzled by (row & 7) -> conflict-free ds_read_b128 fragment reads.
//   fp32 : v_mfma_f32_16x16x4_f32 (exact fp32 == fmaf chain), BK = 16, rows padded to 20
//          floats -- the parity mode, 1/16 of the bf16 rate by design.
// Block = 256 threads = 4 waves in a 2x2 grid; wave tile (BM/2)x(BN/2) in 16x16 MFMA tiles.
// Register-staged global->LDS with a 2-deep LDS ring and one barrier per K tile.
#include "gemm_common.h"

namespace {


// ---- the kernel ---------------------------------------------------------------------------
template <typename T, bool A_F32, int EPI, typename OutT, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_kernel(GemmParams p) {
  constexpr int BK = TileCfg<T>::BK;
  constexpr int LR = TileCfg<T>::LDS_ROW;
  constexpr int WM = BM / 2, WN = BN / 2;   // wave tile
  constexpr int TM = WM / 16, TN = WN / 16; // MFMA tiles per wave
  static_assert(!is_glu(EPI) || (TN % 2 == 0), "GEGLU / SWIGLU need value/gate tile pairs");

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  // ring: [2][ A tile (BM rows) | W tile (BN rows) ]
  constexpr int STAGE_ELEMS = (BM + BN) * LR;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 15, lq = lane >> 4;

  // XCD-aware tile order: blocks that share an XCD (same blockIdx % 8) get consecutive
  // tiles of the same M-row band, so the A band and neighbouring W panels stay in that L2.
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int bid = xcd_chunk_position(blockIdx.x, tiles_m * tiles_n);
  const int tm = bid / tiles_n, tn = bid % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  typename StageSel<T, A_F32, BM>::type sa;
  typename StageSel<T, false, BN>::type sw;

  const int nk = p.K / BK;

  auto seg_load = [&](int kt) {
    const int k0 = kt * BK;
    int s = 0, kbeg = 0;
    if (p.nseg > 1 && k0 >= p.kend[0]) { s = 1; kbeg = p.kend[0]; }
    if (p.nseg > 2 && k0 >= p.kend[1]) { s = 2; kbeg = p.kend[1]; }
    sa.load(p.a[s], p.lda[s], m0, p.M, k0 - kbeg, tid);
    sw.load(p.w, p.ldw, n0, p.N, k0, tid);
  };

  seg_load(0);
  sa.store(smem, tid);
  sw.store(smem + BM * LR, tid);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const T* As = smem + (kt & 1) * STAGE_ELEMS;
    const T* Ws = As + BM * LR;
    if (kt + 1 < nk) seg_load(kt + 1);

    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WM + i * 16 + lr;
          af[i] = *reinterpret_cast<const bf16x8*>(As + row * 64 + (((kk * 4 + lq) ^ (row & 7)) << 3));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = wn * WN + j * 16 + lr;
          bf[j] = *reinterpret_cast<const bf16x8*>(Ws + row * 64 + (((kk * 4 + lq) ^ (row & 7)) << 3));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = As[(wm * WM + i * 16 + lr) * 20 + kk * 4 + lq];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = Ws[(wn * WN + j * 16 + lr) * 20 + kk * 4 + lq];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    }

    if (kt + 1 < nk) {
      T* An = smem + ((kt + 1) & 1) * STAGE_ELEMS;
      sa.store(An, tid);
      sw.store(An + BM * LR, tid);
    }
    __syncthreads();
  }

  gemm_epilogue<EPI, OutT, TM, TN, WM, WN>(p, acc, m0, n0, wm, wn, lr, lq);
}

template <typename T, bool A_F32, int EPI, typename OutT, int BM, int BN>
int launch(const GemmParams& p, GemmTarget to) {
  constexpr int LR = TileCfg<T>::LDS_ROW;
  constexpr size_t smem = 2 * (size_t)(BM + BN) * LR * sizeof(T);
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  auto kern = gemm_kernel<T, A_F32, EPI, OutT, BM, BN>;
  if (to.chosen(p, V2A_GEMM_REGISTER_STAGED, false, BM, BN, TileCfg<T>::BK, 2, 2, 2, tiles)) return V2A_OK;
  if constexpr (smem > 48 * 1024) {
    static std::atomic<uint64_t> lds_set{0};
    if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(kern), smem, lds_set, "v2a_gemm")) return rc;
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), smem, to.stream, p);
  return v2a_check_launch("v2a_gemm");
}

template <typename T, bool A_F32, int BM, int BN>
int dispatch_epi(const v2a_gemm_args* a, const GemmParams& p, GemmTarget to) {
  const bool out_f32 = a->out_dtype == V2A_F32;
  switch (a->epilogue) {
    case V2A_EPI_STORE:
      if (out_f32) return launch<T, A_F32, V2A_EPI_STORE, float, BM, BN>(p, to);
      if constexpr (sizeof(T) == 2) return launch<T, A_F32, V2A_EPI_STORE, bf16_t, BM, BN>(p, to);
      break;
    case V2A_EPI_SIGMOID:
      if (out_f32) return launch<T, A_F32, V2A_EPI_SIGMOID, float, BM, BN>(p, to);
      break;
    case V2A_EPI_GELU:
      if (out_f32) return launch<T, A_F32, V2A_EPI_GELU, float, BM, BN>(p, to);
      break;
    case V2A_EPI_QUICK_GELU:   // exact-fp32 compute only (gemm_prepare refuses plain bf16 compute)
      if constexpr (sizeof(T) == 4) {
        if (out_f32) return launch<T, A_F32, V2A_EPI_QUICK_GELU, float, BM, BN>(p, to);
      }
      break;
    case V2A_EPI_GEGLU:
      if (out_f32) {
        if constexpr (sizeof(T) == 4) return launch<T, A_F32, V2A_EPI_GEGLU, float, BM, BN>(p, to);
      } else {
        if constexpr (sizeof(T) == 2) return launch<T, A_F32, V2A_EPI_GEGLU, bf16_t, BM, BN>(p, to);
      }
      break;
    case V2A_EPI_SWIGLU:   // exact-fp32 compute only (gemm_prepare refuses plain bf16 compute)
      if constexpr (sizeof(T) == 4) {
        if (out_f32) return launch<T, A_F32, V2A_EPI_SWIGLU, float, BM, BN>(p, to);
      }
      break;
    case V2A_EPI_RESID:
      if (out_f32) return launch<T, A_F32, V2A_EPI_RESID, float, BM, BN>(p, to);
      break;
    case V2A_EPI_GATE_RESID:
      if (out_f32) return launch<T, A_F32, V2A_EPI_GATE_RESID, float, BM, BN>(p, to);
      break;
  }
  return v2a_fail(V2A_ERR_ARG, "v2a_gemm: unsupported epilogue %d / out_dtype %d for compute dtype %d", a->epilogue,
                  a->out_dtype, a->compute_dtype);
}


// Step seam (v2a_gemm_cfg_euler): the epilogue of the to_pred GEMM that also does the CFG combine, the Euler update, the operand planes of the new
// y and the step counter.  The workgroup's BM x BN accumulators are staged in LDS (the ring is dead), so that the thread that holds four columns of
// a conditional row finds the same columns of its null row (BM/2 tile rows further, another wave's).  Both predictions are formed by the expressions
// of the STORE epilogue (1 / rms per row, then the bias) and stored for every row the plain launch writes, register rows included; frame rows then
// update y by cfg_euler_axpy, the expression of v2a_cfg_euler, and store its hi | lo planes (split_bf16's rounding) for both halves.
// Step counter: every wave reads dt[step[0]] first; behind the barrier that follows, one thread counts the workgroup in.  The workgroup that finds
// all others counted in advances the counter and puts the arrival counter back to zero; nobody waits for anybody.
template <int TM, int TN, int WM, int WN, int BM, int BN>
__device__ __forceinline__ void gemm_epilogue_cfg_euler(const GemmParams& p, f32x4 (&acc)[TM][TN], float* tile, const float* rs, int tm, int n0,
                                                        int wm, int wn, int tid) {
  constexpr int LD = BN + 4, HB = BM / 2;
  static_assert(BN / 4 == 16 && HB == 2 * 16, "256 threads: 16 lanes of four columns per row, two rows each");
  const int lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int32_t stepv = p.seam.step[0];
  float h = p.seam.dt[stepv];
  float sv = p.seam.s;
  asm volatile("" : "+v"(h), "+v"(sv));     // h has arrived before the workgroup counts in; s in a register of its own (as cfg_euler_planes_kernel)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) tile[(wm * WM + i * 16 + lq * 4 + jj) * LD + wn * WN + j * 16 + lr] = acc[i][j][jj];
  __syncthreads();
  if (tid == 0) {
    const uint32_t nwg = gridDim.x;
    if (atomicAdd(p.seam.arrive, 1u) == nwg - 1) {      // every workgroup has read the step
      atomicExch(p.seam.arrive, 0u);
      p.seam.step[0] = stepv + 1;
    }
  }
  const int c4 = (tid & 15) * 4, r0 = tid >> 4;
  const int n = n0 + c4;                    // N % BN == 0 (host): every column exists
  const int mh = p.M >> 1, N = p.N;
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n);
  float* out = reinterpret_cast<float*>(p.out);
  const int rps = p.seam.rows_per_seq, row_off = p.seam.row_off, T = p.seam.T;
#pragma unroll
  for (int q = 0; q < HB / 16; ++q) {
    const int r = r0 + q * 16;
    const int m = tm * HB + r;              // row of the conditional half; the null half's lies mh further
    if (m >= mh) continue;
    f32x4 pc = *reinterpret_cast<const f32x4*>(tile + r * LD + c4);
    f32x4 pn = *reinterpret_cast<const f32x4*>(tile + (r + HB) * LD + c4);
    if (rs) {
      pc *= rs[r];
      pn *= rs[r + HB];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pc[e] += bv[e];
      pn[e] += bv[e];
    }
    *reinterpret_cast<f32x4*>(out + (int64_t)m * p.ldo + n) = pc;
    *reinterpret_cast<f32x4*>(out + (int64_t)(mh + m) * p.ldo + n) = pn;
    const int b = m / rps, t = m - b * rps - row_off;
    if (t < 0 || t >= T) continue;          // register rows (and rows a padded sequence keeps behind its frames): the predictions only
    float* yp = p.seam.y + ((int64_t)b * T + t) * N + n;
    f32x4 yv = *reinterpret_cast<const f32x4*>(yp);
#pragma unroll
    for (int e = 0; e < 4; ++e) yv[e] = cfg_euler_axpy(yv[e], pc[e], pc[e] - pn[e], h, sv);
    *reinterpret_cast<f32x4*>(yp) = yv;
    bf16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      hi[e] = (bf16_t)yv[e];
      lo[e] = (bf16_t)(yv[e] - (float)hi[e]);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      bf16_t* row = p.seam.planes + (int64_t)(k * mh + m) * p.seam.ldp + n;
      *reinterpret_cast<bf16x4*>(row) = hi;
      *reinterpret_cast<bf16x4*>(row + p.seam.lo_off) = lo;
    }
  }
}

// ---- v2: bf16 x bf16, LDS-DMA staging, 3-deep ring -------------------------------------------
// Both tiles arrive by global_load_lds_dwordx4 (1 KiB = 8 rows x 128 B per wave-instruction, LDS
// image linear per wave, XOR swizzle applied to the per-lane SOURCE chunk: rule 21 of the CDNA guide),
// two K tiles stay in flight across the single raw s_barrier of each iteration (counted vmcnt),
// and no VGPRs or ds_writes are spent on staging.
// (the counted wait is ring_wait of gemm_common.h; the cross-attention kernels run the 64x64 form of this ring from xattn_ring.h)

// S3 (the "bf16x3" mode natively): both operands arrive as hi | lo bf16 planes (V2A_BF16_SPLIT rows of A, W rows [W_hi | W_lo]),
// a ring stage holds the four plane tiles of a K step and every fragment pair feeds three MFMAs,
//   acc += A_lo W_hi + A_hi W_lo + A_hi W_hi   (fp32-grade product, relative error ~2^-16),
// so a K step moves 2x the bytes of a bf16 step for 3x its flops -- where the three-segment form on the plain kernel
// ([A_hi | A_hi | A_lo] x [W_hi | W_lo | W_hi]) moved 3x the bytes and needed one launch per logical K segment.
// (Round 4 measured a software-pipelined form of the K loop -- the fragment reads of tile k + 1 issued behind the barrier of step k into a
// second register set, landing under the MFMAs of tile k: 1-5 % SLOWER at equal occupancy, 16-27 % where the extra registers cost a
// resident workgroup, profiles/r04_ring_pipe_probe.txt.  The exposed part of a K step is not the LDS read latency; the form is not kept.)
// BK (round 5): K extent of a ring stage, 64 or 32.  With 32 the LDS rows are 64 B -- a 1 KB DMA instruction then covers 16 rows, the
// 16-B chunk index of a row is XOR-ed with 3 for rows 8..15 of each 16-row group (conflict-free for the lane groups of ds_read_b128:
// every 16 lanes of a group then cover all 16 slots of a 256-B bank row) -- and a stage holds half the bytes: the split-operand 128x256
// tile (hi + lo planes) fits three stages in 144 KB.
template <int EPI, typename OutT, int BM, int BN, int WGM, int WGN, int NST = 3, bool S3 = false, int BK = 64>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_bf16_dma_kernel(const GemmParams p) {
  static_assert(BK == 64 || BK == 32, "K extent of a stage");
  constexpr int NW = WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr int ROWB = BK * 2;                            // bytes of an LDS row
  constexpr int RPG = 1024 / ROWB;                        // rows per DMA instruction (1 KB per wave-instruction)
  constexpr int CPR = BK / 8;                             // 16-B chunks per row
  constexpr int KK = BK / 32;                             // MFMA K steps per stage
  constexpr int PLANE_BYTES = (BM + BN) * ROWB;           // one A tile + one W tile of a K step
  constexpr int STAGE_BYTES = PLANE_BYTES * (S3 ? 2 : 1); // S3: [A_hi | W_hi | A_lo | W_lo]
  constexpr int GA = BM / RPG, GW = BN / RPG;   // DMA groups (RPG rows each) of the A and W tiles
  constexpr int LPW = (GA + GW) / NW;           // DMA instructions per wave per K tile
  static_assert((GA + GW) % NW == 0, "DMA groups must divide evenly over the waves");
  // chunk swizzle of a row inside its DMA group (applied to the DMA source address and to the fragment reads)
  auto swz = [](int row) { return BK == 64 ? (row & 7) : (((row >> 3) & 1) * 3); };
  static_assert(!is_glu(EPI) || (TN % 2 == 0), "GEGLU / SWIGLU need value/gate tile pairs");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int lr = lane & 15, lq = lane >> 4;

  int tm, tn;
  tile_of_block(p, blockIdx.x, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  // step seam (v2a_gemm_cfg_euler): tile row j of band tm is row tm * BM/2 + (j mod BM/2) of the conditional (j < BM/2) or the null half of the
  // M rows, so that a tile holds both predictions of its BM/2 rows of y; same K loop, rows are only fetched from elsewhere
  constexpr bool SEAM = EPI == V2A_EPI_CFG_EULER;
  static_assert(!SEAM || (S3 && BK == 64), "the step seam runs on the 64-wide K stage split ring");
  auto seam_row = [&](int j) {
    const int mh = p.M >> 1, r = tm * (BM / 2) + (j & (BM / 2 - 1));
    return (j >= BM / 2 ? mh : 0) + (r < mh ? r : mh - 1);
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane source geometry: lane -> (row in 8-row group = lane >> 3, physical chunk = lane & 7);
  // DMA group g (0 .. GA+GW-1) is handled by wave g % NW; groups < GA are A rows, the rest W rows.
  // Each slot keeps ONE 32-bit per-lane byte offset for the whole K loop; the K advance and the
  // operand base are wave-uniform (SGPR), so an issue costs no vector address arithmetic.
  const int srow = lane / CPR;
  const int schunk = ((lane % CPR) ^ swz(srow)) << 3;  // logical chunk (elements) fetched into physical slot lane % CPR
  int grow[LPW];
  uint32_t goff[LPW];
  auto set_offsets = [&](int64_t lda) {
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
      const int g = wave + i * NW;
      const int64_t rbase = g < GA ? (p.a_rowoff ? (int64_t)p.a_rowoff[grow[i]] : (int64_t)grow[i] * lda) : (int64_t)grow[i] * p.ldw;
      goff[i] = (uint32_t)((rbase + schunk) * 2);
    }
  };
#pragma unroll
  for (int i = 0; i < LPW; ++i) {
    const int g = wave + i * NW;
    if (g < GA) {
      const int r = SEAM ? seam_row(g * RPG + srow) : m0 + g * RPG + srow;
      grow[i] = r < p.M ? r : p.M - 1;
    } else {
      const int r = n0 + (g - GA) * RPG + srow;
      grow[i] = r < p.N ? r : p.N - 1;
    }
  }
  set_offsets(p.lda[0]);
  // K-tile offset table read through the constant address space: a scalar load (lgkmcnt).  As a plain global load inside
  // the K loop it became a VECTOR load (the LDS-DMA stores "clobber" memory for the compiler) followed by s_waitcnt vmcnt(0)
  // -- on the dense path too, at the join of the two branches -- which drained the staged tiles in flight every K tile.
  typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
  const const_i32_ptr koff_tab = (const_i32_ptr)p.a_koff;

  // Operand stream state, all wave-uniform: K tiles are issued strictly in order, so the A / W tile bases are running pointers
  // stepped by 128 B per K tile and the (at most two) segment switches are counted down.  The first version recomputed the
  // segment of every K tile from the kernel arguments -- p.a[sgi] / p.lda[sgi] with a run-time sgi are two dependent scalar
  // loads from the argument segment, plus ~60 scalar and vector-select instructions -- between the barrier and the first DMA of
  // EVERY K step: ~500 cycles per step for 128 cycles of MFMA on a 64x64 tile (ISA listing and K-loop probe in DESIGN.md section 4).
  const char* a_run = reinterpret_cast<const char*>(p.a[0]);
  const char* w_run = reinterpret_cast<const char*>(p.w);
  const char* const a_first = a_run;
  const int nseg = p.nseg;
  int seg = 0;
  int seg_left = (nseg > 1 ? p.kend[0] : p.K) / BK;       // K tiles left in the current segment
  // S3: byte offset of the lo plane inside an A row (= the segment's K extent) and inside a W row (= K)
  int64_t a_lo_bytes = S3 ? p.alo[0] * 2 : 0;
  const int64_t w_lo_bytes = S3 ? (int64_t)p.K * 2 : 0;
  int kt_next = 0;                                        // index of the next K tile to issue (offset-table path only)
  auto issue = [&](int stage) {
    if (seg_left == 0) {                                  // at most twice per kernel: the next A segment has its own base and row stride
      ++seg;
      a_run = reinterpret_cast<const char*>(seg == 1 ? p.a[1] : p.a[2]);
      seg_left = (seg == 1 ? (nseg > 2 ? p.kend[1] : p.K) - p.kend[0] : p.K - p.kend[1]) / BK;
      if constexpr (S3) a_lo_bytes = (seg == 1 ? p.alo[1] : p.alo[2]) * 2;
      set_offsets(seg == 1 ? p.lda[1] : p.lda[2]);
    }
    const char* ab = a_run;
    if (koff_tab) ab = a_first + (int64_t)koff_tab[kt_next] * 2;     // implicit-GEMM convolution: wave-uniform scalar load
    const char* wb = w_run;
    char* st = smem_raw + stage * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
      const int g = wave + i * NW;
      if (g < GA)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ab + goff[i]),
                                         (__attribute__((address_space(3))) void*)(st + g * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wb + goff[i]),
                                         (__attribute__((address_space(3))) void*)(st + g * 1024), 16, 0, 0);
    }
    if constexpr (S3) {          // the lo planes: same rows, the segment's / the weight's plane offset further
#pragma unroll
      for (int i = 0; i < LPW; ++i) {
        const int g = wave + i * NW;
        if (g < GA)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ab + a_lo_bytes + goff[i]),
                                           (__attribute__((address_space(3))) void*)(st + PLANE_BYTES + g * 1024), 16, 0, 0);
        else
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wb + w_lo_bytes + goff[i]),
                                           (__attribute__((address_space(3))) void*)(st + PLANE_BYTES + g * 1024), 16, 0, 0);
      }
    }
    a_run += ROWB;
    w_run += ROWB;
    --seg_left;
    ++kt_next;
  };

  // epilogue operands are prefetched unless registers are short: the 256x256 tile (128 accumulators per lane) and the
  // 8-wave 128x256 tile with BOTH residual and gate rows (64 + 64 registers on top of two fragment sets)
  // (round 4: the STORE epilogue's RoPE prefetch on that tile -- 64 more registers -- spilled 78 VGPRs to scratch, found by
  // tests/test_isa_guard.py: off there too)
  constexpr bool PF = BM * BN <= 128 * 256 && !((EPI == V2A_EPI_GATE_RESID || EPI == V2A_EPI_STORE) && BM * BN == 128 * 256);
  EpiPrefetch<EPI, TM, WN, PF> pf;
  if constexpr (!SEAM) {
    if (p.vec_epi) pf.load(p, m0 + wm * WM, n0 + wn * WN, lane);
  }
  // folded RMSNorm (consumer): the row's partial sums are requested ahead of the first operand DMA ...
  static_assert(BM <= 64 * NW, "one thread per tile row");
  float* rs_lds = reinterpret_cast<float*>(smem_raw + NST * STAGE_BYTES);
  const bool scaled = p.rssq != nullptr && p.vec_epi;
  RowScaleLoad rsl;
  if (scaled && tid < BM) rowscale_load(p, SEAM ? seam_row(tid) : m0 + tid, rsl);
  const int nk = p.K / BK;
  // ring of NST stages, NST - 1 K tiles in flight while one is computed (3 by default; 2: the 256x256 tile, whose 64 KB
  // stages leave room for only two; 6: the small tiles of a one-clip launch, which has at most one workgroup per CU and is
  // bound by DMA latency x bytes in flight -- a K step of the 3-deep 64x64 ring took 1020 cycles for 128 cycles of MFMA)
#pragma unroll
  for (int s0 = 0; s0 < NST - 1; ++s0)
    if (s0 < nk) issue(s0);
  // ... and turned into the row's scale behind them (visible to every wave after the K loop's barriers)
  if (scaled && tid < BM) rs_lds[tid] = rowscale_finish(p, rsl);
  // one K tile; STAGE is a compile-time ring position so every LDS address is base + immediate
  auto tile = [&](auto stage_c, int kt) {
    constexpr int STAGE = decltype(stage_c)::value;
    // tile kt has landed for this wave once only the younger tile's DMAs remain outstanding
#ifdef V2A_GEMM_PROBE   // K-loop attribution (scripts/probes/kloop_probe.py): bit 0 = no fragment reads / MFMAs, bit 1 = no DMA and no wait in the loop
    if (!(p.dbg & 2))
#endif
    ring_wait<NST - 2 < 0 ? 0 : NST - 2, LPW * (S3 ? 2 : 1)>(nk - 1 - kt);
    __builtin_amdgcn_s_barrier();   // ... and for every wave; also: everyone is done reading stage (kt-1) % NST
#ifdef V2A_GEMM_PROBE
    if (p.dbg & 1) {
      if (kt + NST - 1 < nk) issue((STAGE + NST - 1) % NST);
      return;
    }
#endif
    const bf16_t* As = reinterpret_cast<const bf16_t*>(smem_raw + STAGE * STAGE_BYTES);
    const bf16_t* Ws = As + BM * BK;
    // all 32-wide K steps of the tile are requested before the first MFMA: the later ones' LDS latency runs under the
    // first one's MFMA cluster instead of being exposed (the compiler otherwise emits read / wait / MFMA per step)
    bf16x8 af[KK][TM], bf[KK][TN];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WM + i * 16 + lr;
        af[kk][i] = *reinterpret_cast<const bf16x8*>(As + row * BK + (((kk * 4 + lq) ^ swz(row)) << 3));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WN + j * 16 + lr;
        bf[kk][j] = *reinterpret_cast<const bf16x8*>(Ws + row * BK + (((kk * 4 + lq) ^ swz(row)) << 3));
      }
    }
    if constexpr (S3) {
      // lo planes of the same rows; three products per fragment pair, small terms first
      const bf16_t* Al = As + PLANE_BYTES / 2;
      const bf16_t* Wl = Al + BM * BK;
      bf16x8 afl[KK][TM], bfl[KK][TN];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WM + i * 16 + lr;
          afl[kk][i] = *reinterpret_cast<const bf16x8*>(Al + row * BK + (((kk * 4 + lq) ^ swz(row)) << 3));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = wn * WN + j * 16 + lr;
          bfl[kk][j] = *reinterpret_cast<const bf16x8*>(Wl + row * BK + (((kk * 4 + lq) ^ swz(row)) << 3));
        }
      }
#ifdef V2A_GEMM_PROBE
      if (!(p.dbg & 2))
#endif
      if (kt + NST - 1 < nk) issue((STAGE + NST - 1) % NST);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
#ifdef V2A_GEMM_PROBE     // error attribution (tests/precision_attribution.py): bit 5 drops the two cross products = plain bf16 arithmetic
            if (!(p.dbg & 32)) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afl[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk][i], bfl[kk][j], acc[i][j], 0, 0, 0);
            }
#else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afl[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk][i], bfl[kk][j], acc[i][j], 0, 0, 0);
#endif
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
          }
    } else {
    // the next tile's DMA is issued behind the first half's fragment reads: their LDS latency runs under the DMA issue
    // (~4 x LPW scalar instructions and LPW address translations) instead of after it
#ifdef V2A_GEMM_PROBE
    if (!(p.dbg & 2))
#endif
    if (kt + NST - 1 < nk) issue((STAGE + NST - 1) % NST);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
    // pin that order (the scheduler otherwise sinks the second half's reads back below the first MFMA cluster):
    // [first half's reads] [the DMA issue] then {a few MFMAs, one read of the second half} ... then the remaining MFMAs
    if constexpr (BK == 64) {
      constexpr int NL = TM + TN, NM = TM * TN, PER = NM / NL > 0 ? NM / NL : 1;
      __builtin_amdgcn_sched_group_barrier(0x100, NL, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, LPW, 0);
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - PER * NL, 0);
    }
    }
  };
  static_assert(NST >= 2 && NST <= 6, "ring depth");
  for (int kt = 0; kt < nk; kt += NST) {
    tile(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) tile(std::integral_constant<int, 1>{}, kt + 1);
    if constexpr (NST > 2) { if (kt + 2 < nk) tile(std::integral_constant<int, 2>{}, kt + 2); }
    if constexpr (NST > 3) { if (kt + 3 < nk) tile(std::integral_constant<int, 3>{}, kt + 3); }
    if constexpr (NST > 4) { if (kt + 4 < nk) tile(std::integral_constant<int, 4>{}, kt + 4); }
    if constexpr (NST > 5) { if (kt + 5 < nk) tile(std::integral_constant<int, 5>{}, kt + 5); }
  }
  if constexpr (SEAM) {
    __builtin_amdgcn_s_barrier();   // every wave is done reading the K-loop stages; all DMAs were retired above
    static_assert(BM * (BN + 4) * 4 <= NST * STAGE_BYTES, "the staged tile must fit in the ring memory");
    gemm_epilogue_cfg_euler<TM, TN, WM, WN, BM, BN>(p, acc, reinterpret_cast<float*>(smem_raw), scaled ? rs_lds : nullptr, tm, n0, wm, wn, tid);
  } else if (p.vec_epi) {
    __builtin_amdgcn_s_barrier();   // every wave is done reading the K-loop stages; all DMAs were retired above
    static_assert(NW * 16 * (WN + 4) * 4 <= NST * STAGE_BYTES, "epilogue slabs must fit in the ring memory");
    float* tile = reinterpret_cast<float*>(smem_raw) + wave * (16 * (WN + 4));
    gemm_epilogue_lds<EPI, OutT, TM, TN, WM, WN, PF>(p, acc, tile, m0 + wm * WM, n0 + wn * WN, lane, pf, scaled ? rs_lds + wm * WM : nullptr);
  } else {
    gemm_epilogue<EPI, OutT, TM, TN, WM, WN>(p, acc, m0, n0, wm, wn, lr, lq);
  }
}

template <int EPI, typename OutT, int BM, int BN, int WGM, int WGN, int NST, bool S3 = false, int BK = 64>
int launch_dma(const GemmParams& p_in, GemmTarget to) {
  GemmParams p = p_in;
  v2a_detail::fill_tile_map(p, BM, BN);
  V2A_REQUIRE((int64_t)p.tiles_m * p.tiles_n < (1 << 24), "v2a_gemm: %d x %d tiles exceed the tile map", p.tiles_m, p.tiles_n);
  constexpr size_t smem = NST * (size_t)(BM + BN) * (BK * 2) * (S3 ? 2 : 1) + BM * 4 + 16;    // the ring + one row scale per tile row (folded RMSNorm)
  static_assert(smem <= 160 * 1024, "ring does not fit the LDS");
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  // W loads keep the default cache policy: non-temporal (aux = 2) measured 9 % slower end to end here, the W
  // panel being re-read from L2 by the 13-25 M-band workgroups of its XCD (profiles/ notes in DESIGN.md)
  auto kern = gemm_bf16_dma_kernel<EPI, OutT, BM, BN, WGM, WGN, NST, S3, BK>;
  if constexpr (BK != 64) V2A_REQUIRE(!p.a_koff, "v2a_gemm(dma): K-tile offset tables are laid out for 64-wide K tiles");
  if (to.chosen(p, V2A_GEMM_RING, S3, BM, BN, BK, WGM, WGN, NST, tiles)) return V2A_OK;
  static std::atomic<uint64_t> lds_set{0};
  if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(kern), smem, lds_set, "v2a_gemm(dma)")) return rc;
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(64 * WGM * WGN), smem, to.stream, p);
  return v2a_check_launch("v2a_gemm(dma)");
}

template <int BM, int BN, int WGM, int WGN, int NST = 3>
int dispatch_dma(const v2a_gemm_args* a, const GemmParams& p, GemmTarget to) {
  const bool out_f32 = a->out_dtype == V2A_F32;
  switch (a->epilogue) {
    case V2A_EPI_STORE:
      return out_f32 ? launch_dma<V2A_EPI_STORE, float, BM, BN, WGM, WGN, NST>(p, to) : launch_dma<V2A_EPI_STORE, bf16_t, BM, BN, WGM, WGN, NST>(p, to);
    case V2A_EPI_GEGLU:   // fp32 output: the hidden activation of the bf16x3 mode, split into hi / lo planes afterwards
      if constexpr ((BN / WGN / 16) % 2 == 0)
        return out_f32 ? launch_dma<V2A_EPI_GEGLU, float, BM, BN, WGM, WGN, NST>(p, to) : launch_dma<V2A_EPI_GEGLU, bf16_t, BM, BN, WGM, WGN, NST>(p, to);
      break;
    case V2A_EPI_RESID:
      if (out_f32) return launch_dma<V2A_EPI_RESID, float, BM, BN, WGM, WGN, NST>(p, to);
      break;
    case V2A_EPI_GATE_RESID:
      if (out_f32) return launch_dma<V2A_EPI_GATE_RESID, float, BM, BN, WGM, WGN, NST>(p, to);
      break;
  }
  return v2a_fail(V2A_ERR_ARG, "v2a_gemm(dma): unsupported epilogue %d / out_dtype %d", a->epilogue, a->out_dtype);
}

// split-bf16 operands (bf16x3 mode): the epilogues that mode uses
template <int BM, int BN, int WGM, int WGN, int NST, int BK = 64>
int dispatch_s3(const v2a_gemm_args* a, const GemmParams& p, GemmTarget to) {
  const bool out_f32 = a->out_dtype == V2A_F32;
  switch (a->epilogue) {
    case V2A_EPI_STORE:
      if (out_f32) return launch_dma<V2A_EPI_STORE, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      break;
    case V2A_EPI_GEGLU:
      if constexpr ((BN / WGN / 16) % 2 == 0) {
        if (a->out_dtype == V2A_BF16_SPLIT) return launch_dma<V2A_EPI_GEGLU, bf16_t, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      }
      break;
    case V2A_EPI_SWIGLU:
      if constexpr ((BN / WGN / 16) % 2 == 0) {
        if (out_f32) return launch_dma<V2A_EPI_SWIGLU, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
        if (a->out_dtype == V2A_BF16_SPLIT) return launch_dma<V2A_EPI_SWIGLU, bf16_t, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      }
      break;
    case V2A_EPI_GELU:
      if (out_f32) return launch_dma<V2A_EPI_GELU, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      if (a->out_dtype == V2A_BF16_SPLIT) return launch_dma<V2A_EPI_GELU, bf16_t, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      break;
    case V2A_EPI_QUICK_GELU:
      if (out_f32) return launch_dma<V2A_EPI_QUICK_GELU, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      if (a->out_dtype == V2A_BF16_SPLIT) return launch_dma<V2A_EPI_QUICK_GELU, bf16_t, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      break;
    case V2A_EPI_RESID:
      if (out_f32) return launch_dma<V2A_EPI_RESID, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      break;
    case V2A_EPI_GATE_RESID:
      if (out_f32) return launch_dma<V2A_EPI_GATE_RESID, float, BM, BN, WGM, WGN, NST, true, BK>(p, to);
      break;
  }
  return v2a_fail(V2A_ERR_ARG, "v2a_gemm(split bf16): unsupported epilogue %d / out_dtype %d for this tile shape", a->epilogue, a->out_dtype);
}

// ---- the ring tile shapes: each is stated in its list below and instantiated by launch_ring_tile, nowhere else (the tile_hint comment of
// include/v2a_cfm.h documents the same rows).  Plain bf16 x bf16 operands, keyed by k = v2a_tuning.gemm_force_tile = v2a_gemm_args.tile_hint - 1:
//   X(k, BM, BN, wave rows, wave columns, ring depth)
#define V2A_RING_TILES(X)                                                                    \
  X(0, 128, 256, 2, 4, 3)  /* 8 waves, 144 KB LDS, 1 workgroup/CU */                         \
  X(1, 128, 128, 2, 2, 3)  /* 4 waves,  96 KB */                                             \
  X(2, 128, 64, 2, 2, 3)   /* 4 waves,  72 KB, 2 workgroups/CU */                            \
  X(3, 64, 64, 2, 2, 3)    /* 4 waves,  48 KB, 3 workgroups/CU */                            \
  X(5, 256, 256, 2, 4, 2)  /* 8 waves, 128x64 wave tiles, 2-deep ring of 64 KB stages */     \
  X(7, 64, 128, 2, 2, 6)   /* 4 waves, 144 KB: 6-deep ring, 1 workgroup/CU (<= 256 tiles) */ \
  X(8, 64, 64, 2, 2, 6)    /* 4 waves,  96 KB: 6-deep ring, 1 workgroup/CU (<= 256 tiles) */ \
  X(9, 64, 64, 2, 2, 4)                                                                      \
  X(10, 64, 64, 2, 2, 5)                                                                     \
  X(11, 128, 128, 2, 2, 4)                                                                   \
  X(12, 128, 128, 2, 4, 3) /* 8 waves (two per SIMD), wave tile 64x32 */                     \
  X(13, 64, 64, 2, 4, 3)   /* 8 waves, wave tile 32x16 (no GEGLU) */                         \
  X(14, 128, 64, 4, 2, 3)  /* 8 waves, wave tile 32x32 */                                    \
  X(15, 64, 128, 2, 4, 3)  /* 8 waves, wave tile 32x32 */
// the ids the code below names.  kTile8Phase is no ring shape: the 256x256 phase-interleaved kernel (gemm_8phase.hip); v2a_tuning.gemm_force_tile
// reaches the ids up to kTileForceMax, the later shapes are asked for by hint only
enum { kTile128x256 = 0, kTile128x128 = 1, kTile128x64 = 2, kTile64x64 = 3, kTile64x64Again = 4, kTile256x256 = 5, kTile8Phase = 6,
       kTileForceMax = 8, kTile64x64Waves8 = 13, kTileMax = 15 };
// Split (hi | lo plane) operands, keyed by the tile_hint itself; the planes double a stage.  (64x128 with four waves on 32-wide stages -- 72 KB,
// two workgroups per CU -- measured 15-25 % slower than shape 4 at every size: profiles/r05_split_probe.txt; not kept.)
//   X(hint, BM, BN, wave rows, wave columns, ring depth, K extent of a stage); offset tables run on the 64-wide K stage shapes, up to kSplitScatteredMax
#define V2A_SPLIT_RING_TILES(X)                                                            \
  X(1, 64, 64, 2, 2, 3, 64)    /*  96 KB */                                                \
  X(2, 128, 64, 2, 2, 3, 64)   /* 144 KB */                                                \
  X(3, 128, 128, 2, 4, 2, 64)  /* 8 waves, 128 KB */                                       \
  X(4, 64, 128, 2, 4, 3, 64)   /* 8 waves, 144 KB */                                       \
  X(6, 128, 256, 2, 4, 3, 32)  /* 8 waves, wave tile 64x64; 3 stages of 48 KB (round 5) */ \
  X(7, 128, 128, 2, 4, 3, 32)  /* 8 waves, 3 stages of 32 KB (round 5) */
enum { kSplit64x64 = 1, kSplit128x64 = 2, kSplit128x128 = 3, kSplit64x128 = 4, kSplit8Phase = 5, kSplit128x256K32 = 6, kSplitMax = 7, kSplitScatteredMax = 4 };

#define V2A_TILE_CASE(id, ...) case id:
constexpr bool is_ring_tile(int k) { switch (k) { V2A_RING_TILES(V2A_TILE_CASE) return true; } return false; }
#define V2A_LAUNCH_PLAIN(id, BM, BN, WGM, WGN, NST) case id: return dispatch_dma<BM, BN, WGM, WGN, NST>(a, p, to);
#define V2A_LAUNCH_SPLIT(id, BM, BN, WGM, WGN, NST, BK) case id: return dispatch_s3<BM, BN, WGM, WGN, NST, BK>(a, p, to);
int launch_ring_tile(bool split, int id, const v2a_gemm_args* a, const GemmParams& p, GemmTarget to) {
  if (split) switch (id) { V2A_SPLIT_RING_TILES(V2A_LAUNCH_SPLIT) }
  else switch (id == kTile64x64Again ? kTile64x64 : id) { V2A_RING_TILES(V2A_LAUNCH_PLAIN) }
  return v2a_fail(V2A_ERR_ARG, "v2a_gemm: no %s ring tile %d", split ? "split" : "plain", id);
}

// ---- selection by shape: pure functions of the problem's extents, a few flags and the tuning; each returns an id of the lists above, chosen
// by the workgroups the problem yields on bm x bn tiles (256 CUs)
constexpr int64_t ntiles(int M, int N, int bm, int bn) { return (int64_t)((M + bm - 1) / bm) * ((N + bn - 1) / bn); }
// register-staged exact-fp32 kernel, tile edge: 64x64 tiles while 128x128 ones would leave CUs idle (one clip: 13 x 8 tiles for N = 1024);
// the K order of an output element does not depend on the tile, so the result is the same bit for bit
int fp32_tile_by_shape(int M, int N) { return ntiles(M, N, 128, 128) < 224 && M > 64 ? 64 : 128; }

// Plain bf16 x bf16.  dense: no offset tables and 16-byte aligned epilogue operands, what the 8-phase kernel needs.  Stand-alone launches
// measured with scripts/gemm_probe.py; M = 1564 / 3128 / 6256 / 12512 rows = 1 / 2 / 4 / 8 clips:
//   * 256x256 phase-interleaved kernel: wide outputs from min_tiles_8phase tiles; narrow outputs (512 < N < 2048) once they
//     fill >= 150 CUs with one tile each (8 clips: 1045 vs 793 TF/s at 12512x1024x4096, 1135 vs 967 at 12512x1280x5120);
//   * 128x256 ring kernel: wide outputs below that, narrow ones from ~4 clips (778 vs 534 TF/s at 6256x1024x4096) and N <= 512 at 8 clips (653 vs 450 TF/s at 12512x512x2048);
//   * 128x128 from ~2 clips, 64x64 below (one clip: only small tiles give every CU work).
int plain_tile_by_shape(int M, int N, bool dense, const v2a_detail::GemmTuning& tune) {
  const bool can8 = tune.use_8phase && dense;
  auto nt = [&](int bm, int bn) { return ntiles(M, N, bm, bn); };
  if (N <= 64) return nt(128, 64) >= 512 ? kTile128x64 : kTile64x64;          // conv layers with few output channels
  if (N <= 128) return nt(128, 128) >= 512 ? kTile128x128 : (nt(128, 64) >= 512 ? kTile128x64 : kTile64x64);
  if (N >= 2048) {
    if (can8 && nt(256, 256) >= tune.min_tiles_8phase) return kTile8Phase;
    if (nt(256, 256) >= 512) return kTile256x256;                             // 8-phase kernel switched off: 2-deep ring of 64 KB stages
    return nt(128, 256) >= 96 ? kTile128x256 : kTile64x64;
  }
  if (N > 512) {
    if (can8 && nt(256, 256) >= 150) return kTile8Phase;
    if (nt(128, 256) >= 180) return kTile128x256;
    if (nt(128, 128) >= 180) return kTile128x128;
  } else {
    if (nt(128, 256) >= 150) return kTile128x256;
    if (nt(128, 128) >= 256) return kTile128x128;
  }
  return nt(64, 64) >= 2048 && nt(128, 64) >= 512 ? kTile128x64 : kTile64x64;
}

// Split operands; glu: a GEGLU / SWIGLU epilogue; scattered: offset tables (implicit-GEMM convolution).  Stand-alone launches measured with
// scripts/split_probe.py, profiles/r05_split_probe.txt.  (A 128x128 tile whose two wave groups alternate along K -- one multiplies a stage while the
// other reads and stages the next -- was built and measured in round 5: 20-25 % slower than shape 7, bound by the DMA issue of its loading waves;
// profiles/r05_pingpong_probe.txt, source kept as scripts/probes/gemm_pingpong.hip.txt)
int split_tile_by_shape(int M, int N, bool glu, bool scattered, const v2a_detail::GemmTuning& tune) {
  auto nt = [&](int bm, int bn) { return ntiles(M, N, bm, bn); };
  if (scattered) {
    // Video2Roll convolutions (scripts/v2r_split_tiles.py, one 251-frame clip per launch, RESID + ReLU + split shadow; us for shapes 1 / 2 / 3 / 4):
    // N = 64,  M 1.41e6, K 576:  899 / 740 / 846 / 984;   N = 128, M 3.7e5, K 1152: 677 / 584 / 406 / 450;  N = 256, M 1.0e5, K 2304: 590 / 534 / 396 / 416;
    // N = 512, M 2.9e4, K 4608: 632 / 620 / 401 / 450;  N = 128, M 4.7e4, K 512 (FTB4 conv0): 61 / 57 / 42 / 40.  128x64 for the 64-channel layers, the
    // 8-wave 128x128 tile from N = 128 on; 64x128 only below 256 tiles of 128x128 (unmeasured for the encoder: its smallest launch has 365)
    return N <= 64 ? kSplit128x64 : (nt(128, 128) >= 256 ? kSplit128x128 : kSplit64x128);
  }
  // the phase-interleaved 256x256 kernel on stages of 32 logical k x (hi | lo) planes, three products per stage (lo x hi, hi x lo, hi x hi; every plane is
  // staged and read once, and its K loop hides the operand stream behind the MFMAs): wide outputs from 150 tiles (audio feed-forward at one clip, measured
  // on the earlier three-pass form: 76 us against 102 us on the best split ring tile) and -- round 5 -- narrow ones (512 < N < 2048, any number of logical
  // segments) from 150 tiles, i.e. from ~6 clips per GPU: at 8 clips the 64x128 split ring ran them at 28 % of the MFMA peak (issued products) against 46 % here
  if (tune.use_8phase && N > 512 && nt(256, 256) >= 150) return kSplit8Phase;
  if (glu || N >= 2048) return nt(128, 128) >= 200 ? kSplit128x128 : kSplit64x128;
  // N <= 512 with many rows (the frames stream at 8 clips per GPU: 98 tiles of 256x256 cannot fill the chip on the 8-phase kernel):
  // 128x256 tiles on 32-wide K stages, 960 against 721 TF/s (64x128) at 12512x512x2048
  if (N <= 512 && nt(128, 256) >= 128) return kSplit128x256K32;
  return nt(64, 128) >= 160 ? kSplit64x128 : kSplit64x64;
}

}  // namespace

// defaults: phase-interleaved 256x256 kernel for wide outputs once a launch has >= 400 tiles, i.e. from two clips per GPU on
// (A/B on MI355X: +1..2 % at 8 clips per GPU end to end).  At one clip its 224-280 workgroups of 128 KB LDS take every CU for
// 35-70 us: alone it is the fastest choice for the feed-forward GEMMs (774 vs 644 TF/s), beside the other two streams of the
// sampler it costs 1.3 % end to end, and with fewer tiles the 128x256 ring kernel fills the chip better anyway.
static constexpr v2a_detail::GemmTuning kDefaultTuning = {-1, 0, 1, 400, 1, 0};
v2a_detail::GemmTuning v2a_detail::g_gemm_tuning = kDefaultTuning;
int v2a_detail::g_dwconv_rows_per_wave = 4;
int v2a_detail::g_attn_one_group_from = 1536;
int v2a_detail::g_probe_dbg = 0;       // v2a_tuning.reserved[0]: read by probe builds only
int v2a_detail::g_dwconv_stream = 1;   // streaming depthwise conv for chip-filling launches (dwconv_rows_per_wave = -1 switches it off: A/B)

extern "C" int v2a_gemm_args_size(void) { return (int)sizeof(v2a_gemm_args); }

extern "C" int v2a_set_tuning(const v2a_tuning* t) {
  if (!t) {
    v2a_detail::g_gemm_tuning = kDefaultTuning;
    v2a_detail::g_dwconv_rows_per_wave = 4;
    v2a_detail::g_dwconv_stream = 1;
    v2a_detail::g_attn_one_group_from = 1536;
    v2a_detail::g_probe_dbg = 0;
    return V2A_OK;
  }
  // every field is checked before any is assigned: a rejected call leaves the previous tuning whole
  V2A_REQUIRE(t->dwconv_rows_per_wave == 0 || t->dwconv_rows_per_wave == 4 || t->dwconv_rows_per_wave == 6 || t->dwconv_rows_per_wave == -1,
              "v2a_set_tuning: dwconv_rows_per_wave %d", t->dwconv_rows_per_wave);
  V2A_REQUIRE(t->gemm_force_tile == -1 || (t->gemm_force_tile <= kTileForceMax && (t->gemm_force_tile == kTile8Phase || is_ring_tile(t->gemm_force_tile))),
              "v2a_set_tuning: gemm_force_tile %d", t->gemm_force_tile);
  V2A_REQUIRE(t->gemm_8phase >= 0 && t->gemm_8phase <= 2, "v2a_set_tuning: gemm_8phase %d", t->gemm_8phase);
  V2A_REQUIRE(t->gemm_8phase_min_tiles >= 0 && t->attn_one_group_from >= 0, "v2a_set_tuning: negative threshold");
  v2a_detail::g_dwconv_rows_per_wave = t->dwconv_rows_per_wave > 0 ? t->dwconv_rows_per_wave : 4;
  v2a_detail::g_dwconv_stream = t->dwconv_rows_per_wave == -1 ? 0 : 1;
  v2a_detail::g_attn_one_group_from = t->attn_one_group_from > 0 ? t->attn_one_group_from : 1536;
  v2a_detail::g_gemm_tuning = {t->gemm_force_tile, t->gemm_k_rotation ? 1 : 0, t->gemm_8phase,
                               t->gemm_8phase_min_tiles > 0 ? t->gemm_8phase_min_tiles : kDefaultTuning.min_tiles_8phase,
                               t->gemm_xcd_order_1x8 ? 0 : 1, t->reserved[0]};
  v2a_detail::g_probe_dbg = t->reserved[0];
  return V2A_OK;
}

// argument checks + the kernel parameter block
static int gemm_prepare(const v2a_gemm_args* a, GemmParams& p) {
  V2A_REQUIRE(a != nullptr, "v2a_gemm: null args");
  V2A_REQUIRE(a->nseg >= 1 && a->nseg <= 3, "v2a_gemm: nseg=%d", a->nseg);
  V2A_REQUIRE(a->M > 0 && a->N > 0, "v2a_gemm: M=%d N=%d", a->M, a->N);
  V2A_REQUIRE(a->compute_dtype == V2A_F32 || a->compute_dtype == V2A_BF16, "v2a_gemm: compute dtype %d", a->compute_dtype);
  const bool split_in = a->a_dtype == V2A_BF16_SPLIT;   // A rows and W rows as hi | lo bf16 planes: three MFMA products per fp32 product
  V2A_REQUIRE(a->a_dtype == a->compute_dtype || a->a_dtype == V2A_F32 || (split_in && a->compute_dtype == V2A_BF16),
              "v2a_gemm: A dtype %d with compute dtype %d", a->a_dtype, a->compute_dtype);
  const int bk = a->compute_dtype == V2A_BF16 ? 64 : 16;
  const int a_vec = a->a_dtype == V2A_F32 ? 4 : 8;  // elements per 16-byte load
  p = GemmParams{};
  int K = 0;
  for (int s = 0; s < a->nseg; ++s) {
    V2A_REQUIRE(a->a[s] != nullptr, "v2a_gemm: segment %d null", s);
    V2A_REQUIRE(a->ka[s] > 0 && a->ka[s] % bk == 0, "v2a_gemm: segment %d K=%d not a multiple of %d", s, a->ka[s], bk);
    V2A_REQUIRE(a->lda[s] % a_vec == 0 && ((uintptr_t)a->a[s] & 15) == 0, "v2a_gemm: segment %d not 16-byte aligned", s);
    // with offset tables (implicit-GEMM convolution) lda is ignored: the planes are a_lo_offset apart, checked below
    if (split_in && !a->a_row_offset) V2A_REQUIRE(a->lda[s] >= 2 * (int64_t)a->ka[s], "v2a_gemm: split segment %d needs lda >= 2 * K (hi | lo planes)", s);
    p.a[s] = a->a[s];
    p.lda[s] = a->lda[s];
    K += a->ka[s];
    p.kend[s] = K;
  }
  p.nseg = a->nseg;
  V2A_REQUIRE(a->w != nullptr && ((uintptr_t)a->w & 15) == 0 && a->ldw % (a->compute_dtype == V2A_BF16 ? 8 : 4) == 0 && a->ldw >= (split_in ? 2 : 1) * (int64_t)K,
              "v2a_gemm: W pointer/ldw (%lld) misaligned or < K=%d (x2 for split operands)", (long long)a->ldw, K);
  V2A_REQUIRE(a->out != nullptr, "v2a_gemm: out null");
  p.w = a->w;
  p.ldw = a->ldw;
  p.bias = a->bias;
  p.M = a->M;
  p.N = a->N;
  p.K = K;
  p.out = a->out;
  p.ldo = a->ldo;
  p.out2 = reinterpret_cast<bf16_t*>(a->out_bf16);
  p.ldo2 = a->ld_out_bf16;
  const bool glu = is_glu(a->epilogue);
  if (a->out_bf16) V2A_REQUIRE(a->out_dtype == V2A_F32 && !glu, "v2a_gemm: out_bf16 shadows an fp32 output only");
  p.out2_split = a->out_bf16 && a->out_bf16_split ? 1 : 0;
  p.out2_lo = a->out_bf16_lo_offset > 0 ? a->out_bf16_lo_offset : a->N;
  if (p.out2_split && a->out_row_offset)      // scattered rows (a bordered map): the lo plane is a whole map further, not a row part
    V2A_REQUIRE(a->out_bf16_lo_offset > 0 && a->out_bf16_lo_offset % 4 == 0,
                "v2a_gemm: a split shadow with out_row_offset needs an explicit out_bf16_lo_offset (%lld) > 0, a multiple of 4",
                (long long)a->out_bf16_lo_offset);
  else if (p.out2_split)
    V2A_REQUIRE(p.out2_lo >= a->N && p.out2_lo % 4 == 0 && a->ld_out_bf16 >= p.out2_lo + (int64_t)a->N,
                "v2a_gemm: a split shadow needs out_bf16_lo_offset (%lld) >= N, a multiple of 4, and ld_out_bf16 >= lo offset + N", (long long)p.out2_lo);
  else
    V2A_REQUIRE(a->out_bf16_lo_offset == 0, "v2a_gemm: out_bf16_lo_offset goes with out_bf16_split");
  for (int sg = 0; sg < a->nseg; ++sg) {
    p.alo[sg] = a->a_lo_offset[sg] > 0 ? a->a_lo_offset[sg] : a->ka[sg];
    if (split_in && a->a_row_offset)     // the caller guarantees that every hi-plane row / K-tile offset stays below a_lo_offset
      V2A_REQUIRE(a->a_lo_offset[sg] > 0 && a->a_lo_offset[sg] % 8 == 0,
                  "v2a_gemm: split operands with offset tables need an explicit a_lo_offset (%lld) > 0, a multiple of 8",
                  (long long)a->a_lo_offset[sg]);
    else if (split_in)
      V2A_REQUIRE(p.alo[sg] >= a->ka[sg] && p.alo[sg] % 8 == 0 && a->lda[sg] >= p.alo[sg] + (int64_t)a->ka[sg],
                  "v2a_gemm: split segment %d: a_lo_offset (%lld) must be >= K, a multiple of 8, and lda >= lo offset + K", sg, (long long)p.alo[sg]);
    else
      V2A_REQUIRE(a->a_lo_offset[sg] == 0, "v2a_gemm: a_lo_offset goes with split operands");
  }
  p.out_split = a->out_dtype == V2A_BF16_SPLIT ? 1 : 0;
  if (p.out_split)
    V2A_REQUIRE((a->epilogue == V2A_EPI_GEGLU && a->ldo >= a->N) || (a->epilogue == V2A_EPI_SWIGLU && split_in && a->ldo >= a->N) ||
                    (is_act(a->epilogue) && split_in && a->ldo >= 2 * (int64_t)a->N),
                "v2a_gemm: out_dtype V2A_BF16_SPLIT goes with the GEGLU epilogue and ldo >= N, SWIGLU on split operands and ldo >= N, or GELU / QUICK_GELU "
                "on split operands and ldo >= 2N");
  // GELU (CLIP's MLP): the exact-fp32 kernel and the split-operand kernels carry it; plain bf16 compute has no GELU instantiation
  if (a->epilogue == V2A_EPI_GELU)
    V2A_REQUIRE((a->compute_dtype == V2A_F32 || split_in) && !a->out_bf16 && !a->relu && !a->rope_table && !a->a_row_offset && !a->out_row_offset &&
                    !a->norm_gamma && !a->norm_ssq && !a->row_ssq,
                "v2a_gemm: the GELU epilogue needs fp32 compute or split operands, dense rows, and none of out_bf16 / relu / rope / norm folding");
  // QUICK_GELU (the ViT-L/14-336 CLIP's MLP): exactly as GELU
  if (a->epilogue == V2A_EPI_QUICK_GELU)
    V2A_REQUIRE((a->compute_dtype == V2A_F32 || split_in) && !a->out_bf16 && !a->relu && !a->rope_table && !a->a_row_offset && !a->out_row_offset &&
                    !a->norm_gamma && !a->norm_ssq && !a->row_ssq,
                "v2a_gemm: the QUICK_GELU epilogue needs fp32 compute or split operands, dense rows, and none of out_bf16 / relu / rope / norm folding");
  // SWIGLU (DINOv2's feed-forward): as GELU, built for the exact-fp32 kernel and the split-operand kernels only
  if (a->epilogue == V2A_EPI_SWIGLU)
    V2A_REQUIRE((a->compute_dtype == V2A_F32 || split_in) && !a->relu && !a->rope_table && !a->a_row_offset && !a->out_row_offset && !a->norm_gamma &&
                    !a->norm_ssq && !a->row_ssq && a->ldo >= a->N / 2,
                "v2a_gemm: the SWIGLU epilogue needs fp32 compute or split operands (plain bf16 compute has no SWIGLU instantiation), dense rows, "
                "ldo >= N / 2 and none of relu / rope / norm folding");
  p.resid = a->resid;
  p.ldr = a->ldr;
  p.gate = a->gate;
  p.step = a->step;
  p.gss = a->gate_step_stride;
  p.gbs = a->gate_batch_stride;
  p.rpb = a->rows_per_batch > 0 ? a->rows_per_batch : a->M;
  {
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    const int osz = a->out_dtype == V2A_F32 ? 4 : 2;      // V2A_BF16 and V2A_BF16_SPLIT: bf16 elements
    const int ncols = glu ? a->N / 2 : a->N;
    bool ok = a->N % 4 == 0 && ncols % 4 == 0 && ((uintptr_t)a->out % (4 * osz)) == 0 && (a->ldo * osz) % (4 * osz) == 0;
    if (a->bias) ok = ok && al16(a->bias);
    if (a->resid) ok = ok && al16(a->resid) && a->ldr % 4 == 0;
    if (a->gate) ok = ok && al16(a->gate) && a->gate_step_stride % 4 == 0 && a->gate_batch_stride % 4 == 0;
    if (a->out_bf16) ok = ok && ((uintptr_t)a->out_bf16 & 7) == 0 && a->ld_out_bf16 % 4 == 0;
    p.vec_epi = ok ? 1 : 0;
  }
  // only the LDS-staged epilogue of the ring and 8-phase kernels writes the lo plane of a split shadow; the scalar epilogue (the exact-fp32
  // kernel, fp32 A on bf16 compute, the bf16 SIGMOID kernel, and the ring kernels without 16-byte aligned operands) writes bf16(v) alone
  if (p.out2_split)
    V2A_REQUIRE(a->compute_dtype == V2A_BF16 && a->a_dtype != V2A_F32 && a->epilogue != V2A_EPI_SIGMOID && p.vec_epi,
                "v2a_gemm: out_bf16_split needs bf16 compute on bf16 or split A, an epilogue other than SIGMOID and 16-byte aligned epilogue "
                "operands (compute dtype %d, A dtype %d, epilogue %d): no other kernel writes the lo plane",
                a->compute_dtype, a->a_dtype, a->epilogue);
  p.relu = a->relu;
  // off by default: +0.7 % throughput, but the fp32 summation order of a row then depends on how many rows the call has, so a
  // clip's result would change (in the last bits) with the batch it is sampled in; v2a_set_tuning enables it
  const v2a_detail::GemmTuning tune = v2a_detail::g_gemm_tuning;
  p.krot = 0;
  p.dbg = tune.dbg;
  {
    // XCD grid over the tile space: minimise A_bytes * gn + W_bytes * gm (gemm_common.h, tile_of_block); v2a_set_tuning can
    // pin the old 1 x 8 order for A/B measurements
    const double ab = (double)a->M * K * (a->a_dtype == V2A_F32 ? 4 : 2), wb = (double)a->N * K * (a->compute_dtype == V2A_F32 ? 4 : 2);
    int best_gm = 1;
    double best = ab * 8 + wb;
    // (PMC, one clip: FETCH of the narrow GEMMs -30 %, L2 hit rate 0.71 -> 0.80; end to end +1.5 % at 8 clips per GPU and
    // -0.5 % .. +0.3 % at one clip, inside the run-to-run spread)
    if (tune.xcd_grid) {
      for (int gm = 2; gm <= 8; gm *= 2) {
        const double c = ab * (8 / gm) + wb * gm;
        if (c < best * 0.95) { best = c; best_gm = gm; }
      }
    }
    p.xcd_gm = best_gm;
    p.xcd_gn = 8 / best_gm;
  }
  p.a_rowoff = a->a_row_offset;
  p.a_koff = a->a_ktile_offset;
  p.o_rowoff = a->out_row_offset;
  if (a->a_row_offset || a->a_ktile_offset || a->out_row_offset) {
    V2A_REQUIRE((a->a_row_offset != nullptr) == (a->a_ktile_offset != nullptr), "v2a_gemm: a_row_offset and a_ktile_offset go together");
    V2A_REQUIRE(a->nseg == 1 && a->compute_dtype == V2A_BF16 && (a->a_dtype == V2A_BF16 || split_in) && p.vec_epi &&
                    (a->epilogue == V2A_EPI_STORE || a->epilogue == V2A_EPI_RESID) && !a->rope_table,
                "v2a_gemm: row/K-tile offset tables need one bf16 (or split bf16) segment, bf16 compute, STORE/RESID and 16-byte aligned rows");
  }
  V2A_REQUIRE(!a->relu || !glu, "v2a_gemm: relu with GEGLU / SWIGLU");
  p.ngam = a->norm_gamma;
  p.ngss = a->norm_step_stride;
  p.ngbs = a->norm_batch_stride;
  p.nsw_row = a->norm_switch_row > 0 ? a->norm_switch_row : INT32_MAX;
  p.nsw_off = a->norm_switch_offset;
  p.ssq = a->norm_ssq;
  p.ssq_ld = a->ld_norm_ssq;
  if (a->norm_gamma || a->norm_ssq || a->row_ssq) {
    V2A_REQUIRE(a->compute_dtype == V2A_BF16 && (a->a_dtype == V2A_BF16 || split_in) && p.vec_epi && a->epilogue != V2A_EPI_SIGMOID && !a->out_row_offset,
                "v2a_gemm: a folded RMSNorm needs bf16 x bf16 (or split bf16) operands, dense rows and 16-byte aligned epilogue operands");
    if (a->norm_gamma || a->norm_ssq)
      V2A_REQUIRE(a->out_bf16 && (a->epilogue == V2A_EPI_RESID || a->epilogue == V2A_EPI_GATE_RESID) && a->N % 32 == 0 &&
                      (!a->norm_gamma || (((uintptr_t)a->norm_gamma & 15) == 0 && a->norm_step_stride % 4 == 0 && a->norm_batch_stride % 4 == 0 &&
                                          a->norm_switch_offset % 4 == 0)) &&
                      (!a->norm_ssq || a->ld_norm_ssq >= a->N / 32),
                  "v2a_gemm: norm_gamma / norm_ssq go with RESID / GATE_RESID, an out_bf16 shadow and N %% 32 == 0 (N=%d)", a->N);
  }
  if (int rc = v2a_detail::fill_row_scale(p, a->row_ssq, a->ld_row_ssq, a->row_ssq_parts, a->row_norm_dim, "v2a_gemm")) return rc;
  p.rope = a->rope_table;
  p.rope_cols = a->rope_cols;
  p.rope_pos_off = a->rope_pos_offset;
  if (a->rope_table) {
    V2A_REQUIRE(a->epilogue == V2A_EPI_STORE && a->compute_dtype == V2A_BF16 && (a->a_dtype == V2A_BF16 || split_in) && p.vec_epi &&
                    a->rope_cols % 64 == 0 && a->rope_cols <= a->N && ((uintptr_t)a->rope_table & 15) == 0,
                "v2a_gemm: fused RoPE needs the bf16 STORE epilogue with 16-byte aligned rows and rope_cols %% 64 == 0");
  }
  if (a->epilogue == V2A_EPI_RESID || a->epilogue == V2A_EPI_GATE_RESID)
    V2A_REQUIRE(a->resid != nullptr, "v2a_gemm: epilogue %d needs resid", a->epilogue);
  if (a->epilogue == V2A_EPI_GATE_RESID) V2A_REQUIRE(a->gate != nullptr, "v2a_gemm: GATE_RESID needs gate");
  if (glu) V2A_REQUIRE(a->N % 32 == 0, "v2a_gemm: GEGLU / SWIGLU need N %% 32 == 0 (N=%d)", a->N);
  return V2A_OK;
}

// gemm_prepare -> kernel family -> tile id (asked for by hint, forced by v2a_set_tuning, or by shape) -> that tile's launcher
static int gemm_dispatch(const v2a_gemm_args* a, GemmTarget to) {
  GemmParams p;
  if (int rc = gemm_prepare(a, p)) return rc;
  const v2a_detail::GemmTuning tune = v2a_detail::g_gemm_tuning;
  const bool scattered = a->a_row_offset || a->out_row_offset;
  if (a->compute_dtype == V2A_F32)
    return fp32_tile_by_shape(a->M, a->N) == 64 ? dispatch_epi<float, false, 64, 64>(a, p, to) : dispatch_epi<float, false, 128, 128>(a, p, to);
  if (a->a_dtype == V2A_BF16_SPLIT) {
    V2A_REQUIRE(p.vec_epi, "v2a_gemm: split operands need 16-byte aligned epilogue operands");
    V2A_REQUIRE(a->tile_hint >= 0 && a->tile_hint <= kSplitMax, "v2a_gemm: tile_hint %d with split operands (0 = by shape, 1..7)", a->tile_hint);
    // implicit-GEMM convolution (the bf16x3 Video2Roll encoder): offset tables run on the BK = 64 split ring shapes 1..4 only -- the
    // 8-phase kernel knows dense rows only, and the K-tile tables are laid out for 64-wide K tiles (shapes 6 / 7 stage 32)
    V2A_REQUIRE(!scattered || a->tile_hint <= kSplitScatteredMax,
                "v2a_gemm: tile_hint %d with split operands and offset tables (0 = by shape, 1..4: the 64-wide K stage ring shapes)", a->tile_hint);
    int id = a->tile_hint ? a->tile_hint : split_tile_by_shape(a->M, a->N, is_glu(a->epilogue), scattered, tune);
    if (id == kSplit8Phase && !tune.use_8phase) id = kSplit64x128;      // asked for by hint with the kernel switched off
    if (id != kSplit8Phase) return launch_ring_tile(true, id, a, p, to);
    p.s3_kl = p.K;      // marks the launch as split: 32 logical k of the hi and the lo plane of both operands per stage, K stays the logical K
#ifdef V2A_GEMM_PROBE
    if (tune.dbg & 32) p.s3_kl = 0;                     // error attribution: hi x hi only (the plain form on the hi planes)
#endif
    return v2a_detail::launch_gemm_8phase(p, a->epilogue, a->out_dtype == V2A_BF16_SPLIT ? V2A_BF16 : a->out_dtype, to);
  }
  if (a->a_dtype == V2A_F32) return dispatch_epi<bf16_t, true, 128, 128>(a, p, to);
  if (a->epilogue == V2A_EPI_SIGMOID) return dispatch_epi<bf16_t, false, 128, 128>(a, p, to);
  // bf16 x bf16: the LDS-DMA ring kernel or the 8-phase kernel
  V2A_REQUIRE(a->tile_hint >= 0 && a->tile_hint <= kTileMax + 1, "v2a_gemm: tile_hint %d", a->tile_hint);
  // the producer's partial sums are butterflies over the 8 lanes that hold 32 columns of ONE row: with 16-column wave tiles a row has 4 lanes,
  // an octet would add 16 columns each of two rows, and the two waves of a 32-column group would write the same entry
  V2A_REQUIRE(a->tile_hint != kTile64x64Waves8 + 1 || !a->norm_ssq,
              "v2a_gemm: tile_hint 14 (64x64 tiles, wave tile 32x16) cannot write norm_ssq: the partial sums per 32 columns need wave tiles of "
              "at least 32 columns");
  const bool dense = !scattered && p.vec_epi;
  const bool hinted = a->tile_hint > 0 && tune.force_tile < 0;
  V2A_REQUIRE(!hinted || a->tile_hint - 1 != kTile8Phase || dense, "v2a_gemm: tile_hint 7 (256x256 8-phase) needs dense rows and 16-byte aligned epilogue operands");
  // a forced 8-phase kernel applies to dense launches only: it knows nothing of the implicit-GEMM offset tables (Video2Roll
  // convolutions), which keep their by-shape choice
  const bool forced = tune.force_tile >= 0 && (tune.force_tile != kTile8Phase || dense);
  const int k = hinted ? a->tile_hint - 1 : (forced ? tune.force_tile : plain_tile_by_shape(a->M, a->N, dense, tune));
  if (k == kTile8Phase) return v2a_detail::launch_gemm_8phase(p, a->epilogue, a->out_dtype, to);
  return launch_ring_tile(false, k, a, p, to);
}

extern "C" int v2a_gemm(const v2a_gemm_args* a, v2a_stream_t stream) { return gemm_dispatch(a, {(hipStream_t)stream, nullptr}); }

// The step seam in one launch (include/v2a_cfm.h): gemm_prepare's checks for the to_pred GEMM, then the 64x64 split ring with the seam's row map and
// epilogue.  One workgroup per 32 rows of a half x 64 columns.
extern "C" int v2a_gemm_cfg_euler(const v2a_gemm_args* a, const v2a_step_seam* s, v2a_stream_t stream) {
  GemmParams p;
  if (int rc = gemm_prepare(a, p)) return rc;
  V2A_REQUIRE(s && s->y && s->dt && s->step && s->arrive && s->planes, "v2a_gemm_cfg_euler: null pointer");
  V2A_REQUIRE(a->a_dtype == V2A_BF16_SPLIT && a->compute_dtype == V2A_BF16 && a->epilogue == V2A_EPI_STORE && a->out_dtype == V2A_F32 && p.vec_epi &&
                  !a->out_bf16 && !a->rope_table && !a->relu && !a->a_row_offset && !a->a_ktile_offset && !a->out_row_offset && a->ldo >= a->N,
              "v2a_gemm_cfg_euler: the GEMM must be a split-operand STORE launch with dense fp32 rows and no shadow, rope, relu or offset tables");
  V2A_REQUIRE(a->N % 64 == 0 && s->B > 0 && s->T > 0 && s->row_off >= 0 && s->rows_per_seq >= s->row_off + s->T &&
                  (int64_t)a->M == 2 * (int64_t)s->B * s->rows_per_seq,
              "v2a_gemm_cfg_euler: N=%d (%% 64), M=%d = 2 * B (%d) * rows_per_seq (%d), rows_per_seq >= row_off (%d) + T (%d)", a->N, a->M, s->B,
              s->rows_per_seq, s->row_off, s->T);
  V2A_REQUIRE(((uintptr_t)s->y & 15) == 0 && ((uintptr_t)s->planes & 7) == 0 && s->lo_offset >= a->N && s->lo_offset % 4 == 0 && s->ld % 4 == 0 &&
                  s->ld >= s->lo_offset + a->N,
              "v2a_gemm_cfg_euler: y needs 16-byte, planes 8-byte alignment, lo_offset (%lld) >= N, ld (%lld) >= lo_offset + N, both multiples of 4",
              (long long)s->lo_offset, (long long)s->ld);
  constexpr int BM = 64, BN = 64, NST = 3, BK = 64;
  const int bands = (a->M / 2 + BM / 2 - 1) / (BM / 2);
  const int m_real = p.M;
  p.M = bands * BM;               // the tile map counts row bands of BM/2 rows per half
  v2a_detail::fill_tile_map(p, BM, BN);
  p.M = m_real;
  p.seam = {s->y, s->dt, s->step, s->arrive, reinterpret_cast<bf16_t*>(s->planes), s->ld, s->lo_offset, s->rows_per_seq, s->row_off, s->T, s->cfg_strength};
  constexpr size_t smem = NST * (size_t)(BM + BN) * (BK * 2) * 2 + BM * 4 + 16;      // as launch_dma: the ring + one row scale per tile row
  auto kern = gemm_bf16_dma_kernel<V2A_EPI_CFG_EULER, float, BM, BN, 2, 2, NST, true, BK>;
  static std::atomic<uint64_t> lds_set{0};
  if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(kern), smem, lds_set, "v2a_gemm_cfg_euler")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(256), smem, (hipStream_t)stream, p);
  return v2a_check_launch("v2a_gemm_cfg_euler");
}

extern "C" int v2a_gemm_choose(const v2a_gemm_args* a, v2a_gemm_choice* choice) {
  V2A_REQUIRE(choice != nullptr, "v2a_gemm_choose: null choice");
  *choice = {};
  return gemm_dispatch(a, {nullptr, choice});
}

