// The GEMM half that the two cross-attention kernels share (qproj_xattn_kernel in qproj_xattn.hip, xattn_absorbed_kernel in
// xattn_absorbed.hip), defined once: a 64-row x 64-column tile of A x W^T over K, 4 waves of 16 rows x all 64 columns, on the 3-stage
// LDS-DMA ring of gemm.hip's gemm_bf16_dma_kernel -- stages of 64 k, 1 KB wave-instructions of 8 rows x 128 B whose 16-B chunk is XOR-swizzled
// by (row & 7) on the SOURCE side, one 32-bit byte offset per lane and slot for the whole K loop, running operand pointers stepped by
// 128 B, counted vmcnt (ring_wait) and one barrier per K tile.  S3: hi | lo bf16 planes of both operands, the lo plane K elements further
// in a row, a stage = [A_hi | W_hi | A_lo | W_lo].  Rows of the tile behind the clip's last row read a copy of that row.
// What the two kernels do NOT share stays in them: the operand order of the MFMAs (qproj: A x W; absorbed: W supplies the MFMA's rows),
// the order in which a tile's fragments are read, the gate fragment (qproj: one linear row for all 16 columns; absorbed: NH rows GPITCH
// bytes apart, fragment row lr = head lr % NH), size and place of the gate rows behind the ring, and everything after the K loop.
#pragma once
#include "gemm_common.h"

namespace {

template <bool S3>
struct XattnRing {
  static constexpr int BM = 64, BN = 64, NW = 4, NST = 3, TN = 4;
  static constexpr int NPL = S3 ? 2 : 1;                       // planes of an operand
  static constexpr int PLANE_BYTES = (BM + BN) * 128;
  static constexpr int STAGE_BYTES = PLANE_BYTES * NPL;
  static constexpr int RING_BYTES = NST * STAGE_BYTES;         // the kernels' gate rows and the 64 row scales lie behind
  static constexpr int GA = BM / 8;
  static constexpr int LPW = 4;                                // DMA instructions per wave per K tile and plane: groups wave, wave+4 (A), wave+8, wave+12 (W)

  char* smem;
  int wave, lr, lq;
  int nk;                                                      // K tiles: 0 until start(), so a k_loop() without start() runs no tile
  uint32_t goff[LPW];
  const char* a_run;
  const char* w_run;
  int64_t lo_bytes;

  // source geometry: lane -> (row of the 8-row group, physical 16-B chunk).  w: the W rows of the launch or of the clip; rows n0 .. n0 + 63 exist
  __device__ __forceinline__ XattnRing(char* smem_, const GemmParams& p, const void* w, int m0, int m_end, int n0, int wave_, int lane)
      : smem(smem_), wave(wave_), lr(lane & 15), lq(lane >> 4), nk(0) {
    const int srow = lane >> 3;
    const int schunk = ((lane & 7) ^ srow) << 3;
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
      const int g = wave + i * NW;
      if (g < GA) {
        int r = m0 + g * 8 + srow;
        r = r < m_end ? r : m_end - 1;
        goff[i] = (uint32_t)(((int64_t)r * p.lda[0] + schunk) * 2);
      } else {
        const int r = n0 + (g - GA) * 8 + srow;
        goff[i] = (uint32_t)(((int64_t)r * p.ldw + schunk) * 2);
      }
    }
    a_run = reinterpret_cast<const char*>(p.a[0]);
    w_run = reinterpret_cast<const char*>(w);
    lo_bytes = (int64_t)p.K * 2;
  }

  // the next K tile into `stage`: hi planes, then the lo planes K elements further in the A row and in the W row
  __device__ __forceinline__ void issue(int stage) {
    char* st = smem + stage * STAGE_BYTES;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
      for (int i = 0; i < LPW; ++i) {
        const int g = wave + i * NW;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((g < GA ? a_run : w_run) + pl * lo_bytes + goff[i]),
                                         (__attribute__((address_space(3))) void*)(st + pl * PLANE_BYTES + g * 1024), 16, 0, 0);
      }
    }
    a_run += 128;
    w_run += 128;
  }

  // folded RMSNorm (consumer) around the first NST - 1 K tiles: one thread per tile row requests the row's partial sums ahead of the
  // DMAs and leaves the row's scale in rs_lds behind them.  DMAs a kernel issued before this call are retired by the loop's first wait.
  // scaled = p.rssq != nullptr, which the kernel needs again behind the loop
  __device__ __forceinline__ void start(const GemmParams& p, bool scaled, int m0, int m_end, int tid, float* rs_lds) {
    RowScaleLoad rsl;
    if (scaled && tid < BM) rowscale_load(p, min(m0 + tid, m_end - 1), rsl);
    nk = p.K / 64;      // here, not in the constructor: with K read earlier all twelve kernels compile differently (profiles/xattn_ring_isa.txt)
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
      if (s0 < nk) issue(s0);
    if (scaled && tid < BM) rs_lds[tid] = rowscale_finish(p, rsl);
  }

  // fragments of a landed stage, plane pl, 32-k step kk: the wave's A row wave * 16 + lr, W row j * 16 + lr
  template <int STAGE>
  __device__ __forceinline__ const bf16_t* plane(int pl) const { return reinterpret_cast<const bf16_t*>(smem + STAGE * STAGE_BYTES + pl * PLANE_BYTES); }
  __device__ __forceinline__ bf16x8 frag(const bf16_t* tile, int row, int kk) const {
    return *reinterpret_cast<const bf16x8*>(tile + row * 64 + (((kk * 4 + lq) ^ (row & 7)) << 3));
  }
  template <int STAGE>
  __device__ __forceinline__ bf16x8 a_frag(std::integral_constant<int, STAGE>, int pl, int kk) const { return frag(plane<STAGE>(pl), wave * 16 + lr, kk); }
  template <int STAGE>
  __device__ __forceinline__ bf16x8 w_frag(std::integral_constant<int, STAGE>, int pl, int kk, int j) const {
    return frag(plane<STAGE>(pl) + BM * 64, j * 16 + lr, kk);
  }

  // the K loop: body(stage, kt) runs behind the wait and the barrier of K tile kt, with the ring position as a compile-time constant (every
  // LDS address is base + immediate); it reads its fragments, calls refill(stage, kt), then multiplies
  template <int STAGE>
  __device__ __forceinline__ void refill(std::integral_constant<int, STAGE>, int kt) {
    if (kt + NST - 1 < nk) issue((STAGE + NST - 1) % NST);
  }
  template <int STAGE, typename Body>
  __device__ __forceinline__ void tile(Body& body, int kt) {
    ring_wait<NST - 2, LPW * NPL>(nk - 1 - kt);     // tile kt has landed for this wave once only the younger tile's DMAs remain outstanding
    __builtin_amdgcn_s_barrier();                   // ... and for every wave; also: everyone is done reading stage (kt - 1) % NST
    body(std::integral_constant<int, STAGE>{}, kt);
  }
  template <typename Body>
  __device__ __forceinline__ void k_loop(Body&& body) {
    for (int kt = 0; kt < nk; kt += NST) {
      tile<0>(body, kt);
      if (kt + 1 < nk) tile<1>(body, kt + 1);
      if (kt + 2 < nk) tile<2>(body, kt + 2);
    }
  }
};

// ---- host: what v2a_qproj_xattn and v2a_xattn_absorbed do alike ---------------------------------------------------------------------
// the ring's part of the parameter block: one A segment of K columns (split: 2 K), the W rows, N = the rows of W the ring multiplies
inline void xattn_ring_params(GemmParams& p, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int M, int N, int K, int rpb) {
  p.a[0] = a;
  p.lda[0] = lda;
  p.kend[0] = K;
  p.nseg = 1;
  p.w = w;
  p.ldw = ldw;
  p.bias = bias;
  p.M = M;
  p.N = N;
  p.K = K;
  p.rpb = rpb;
}

// dynamic LDS = ring + gate rows + 64 row scales.  The gate rows grow with K while the opt-in above 64 KB is set ONCE per (kernel, device):
// it is set for GATE_MAX, the gate rows of the largest K the entry point accepts, so a later launch with a larger K than the first one is not
// refused.  lds_set: one static per kernel instantiation (v2a_enable_lds).
template <bool S3, size_t GATE_MAX, typename Params>
int xattn_ring_launch(void (*kern)(Params), const Params& P, int nwg, size_t gate_bytes, std::atomic<uint64_t>& lds_set, const char* who, hipStream_t s) {
  constexpr size_t smem_max = XattnRing<S3>::RING_BYTES + GATE_MAX + 64 * 4;
  static_assert(smem_max <= 160 * 1024, "xattn_ring_launch: ring + GATE_MAX + row scales exceed the 160 KB of LDS (the instantiation note names the kernel)");
  if (int rc = v2a_enable_lds(reinterpret_cast<const void*>(kern), smem_max, lds_set, who)) return rc;
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), XattnRing<S3>::RING_BYTES + gate_bytes + 64 * 4, s, P);
  return v2a_check_launch(who);
}

}  // namespace
