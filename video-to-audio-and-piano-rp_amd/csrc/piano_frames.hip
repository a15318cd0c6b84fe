// Piano-frame preprocessing kernels for gfx950: decoded RGB video frames -> the grey Ho x Wo float32 images of the V2P frame encoder,
// equal bit for bit to the reference's Pillow path (`Image.convert('L')`, `Image.resize((900, 100))` with BICUBIC, `/ 255.`;
// x3:60-63, 1876-1891):
//   v2a_piano_resize_h   rgb2l grey byte of every tap formed in registers + horizontal pass (22-bit fixed-point integer sums,
//                        clipped to uint8) for the input rows the vertical pass reads -> uint8 tmp
//   v2a_piano_resize_v   vertical pass over tmp, clipped to uint8, mapped through the host table u -> float32(u / 255.) -> fp32
//   v2a_piano_resize_vt  the same with a transposed store, out[f][x][y]: the 88-key configuration resizes to 100 wide x 900 tall
//                        and transposes (`Image.resize((100, 900))`, transpose [2, 1, 0]; x3_2 = e2_tts_crossatt3_2.py:65-68)
// Bounds and coefficients come from the host (Pillow's precompute_coeffs / normalize_coeffs_8bpc); the host also guarantees that
// every tap lies inside the image.  Memory-bound integer kernels: no MFMA.
#include "v2a_common.h"

namespace {

constexpr int PF_ROWS = 4;          // input rows per block of the horizontal pass: a column's coefficients are fetched once for all of them
constexpr int PF_THREADS = 256;

// Dword `dw` of the frame buffer (base 4-byte aligned).  The buffer's last total % 4 bytes form no whole dword: they are fetched
// as bytes, and what lies behind the buffer reads as zero (such bytes are never part of a pixel).
__device__ __forceinline__ uint32_t pf_load_dword(const uint8_t* __restrict__ base, int64_t dw, int64_t total) {
  if (4 * dw + 4 <= total) return reinterpret_cast<const uint32_t*>(base)[dw];
  uint32_t v = 0;
  for (int b = 0; b < 4; ++b)
    if (4 * dw + b < total) v |= (uint32_t)base[4 * dw + b] << (8 * b);
  return v;
}

__device__ __forceinline__ uint32_t pf_rgb2l(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

__device__ __forceinline__ uint32_t pf_clip8(int32_t s) {
  s >>= 22;
  return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// ---- grey + horizontal pass ------------------------------------------------------------------------------------------------------
// Block (bx, j): rows y0 + PF_ROWS * bx ... of frame sel[j] (or j).  Phase 1: every lane fetches the 12 bytes of 4 consecutive
// pixels as 4 aligned dwords (a row need not start on a dword), forms their 4 grey bytes and writes them to LDS as one dword.  Phase 2: every lane owns 4 consecutive output columns; per column the taps' coefficients are read once and applied to
// the PF_ROWS grey rows in LDS; the 4 clipped bytes of a row leave as one dword.
__global__ __launch_bounds__(PF_THREADS) void piano_resize_h_kernel(const uint8_t* __restrict__ in, int64_t total, int H, int W,
                                                                    const int32_t* __restrict__ sel, uint8_t* __restrict__ tmp, int ldt,
                                                                    int y0, int rows, int Wo, const int32_t* __restrict__ bounds,
                                                                    const int32_t* __restrict__ coef, int ksize) {
  extern __shared__ uint32_t pf_grey[];          // PF_ROWS rows of W4 = ceil(W / 4) dwords
  const int W4 = (W + 3) >> 2;
  const int j = blockIdx.y;
  const int64_t f = sel ? sel[j] : j;
  const int r0 = blockIdx.x * PF_ROWS;
  const int nr = min(PF_ROWS, rows - r0);
  if (f < 0 || (f + 1) * (int64_t)H * W * 3 > total) return;          // a frame number outside the buffer (block-uniform): nothing is read
  // all nr rows as one index space, so that every lane keeps several independent loads in flight; only a block that touches the
  // buffer's last dwords takes the guarded loads (block-uniform)
  const int64_t row0 = ((f * H + y0 + r0) * (int64_t)W) * 3;          // first byte of the block's first row
  const bool safe = ((row0 + (int64_t)(nr - 1) * W * 3) >> 2) + 3 * (int64_t)W4 + 1 <= (total >> 2);
  for (int idx = threadIdx.x; idx < nr * W4; idx += PF_THREADS) {
    const int r = idx / W4, p = idx - r * W4;
    const int64_t start = row0 + (int64_t)r * W * 3;
    const int64_t d = (start >> 2) + 3 * (int64_t)p;
    const int sh = (int)(start & 3) * 8;
    uint32_t a, b, c, e;
    if (safe) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(in) + d;
      a = q[0], b = q[1], c = q[2], e = q[3];
    } else {
      a = pf_load_dword(in, d, total), b = pf_load_dword(in, d + 1, total), c = pf_load_dword(in, d + 2, total), e = pf_load_dword(in, d + 3, total);
    }
    // the 12 bytes from `start` on: a = R0 G0 B0 R1, b = G1 B1 R2 G2, c = B2 R3 G3 B3 (lowest byte first); pixels behind the row's
    // end give unused bytes
    a = (uint32_t)((((uint64_t)b << 32) | a) >> sh);
    b = (uint32_t)((((uint64_t)c << 32) | b) >> sh);
    c = (uint32_t)((((uint64_t)e << 32) | c) >> sh);
    const uint32_t l0 = pf_rgb2l(a & 255, (a >> 8) & 255, (a >> 16) & 255);
    const uint32_t l1 = pf_rgb2l(a >> 24, b & 255, (b >> 8) & 255);
    const uint32_t l2 = pf_rgb2l((b >> 16) & 255, b >> 24, c & 255);
    const uint32_t l3 = pf_rgb2l((c >> 8) & 255, (c >> 16) & 255, c >> 24);
    pf_grey[idx] = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
  }
  __syncthreads();
  const uint8_t* grey = reinterpret_cast<const uint8_t*>(pf_grey);
  const int gs = 4 * W4;
  for (int q = threadIdx.x; 4 * q < Wo; q += PF_THREADS) {
    uint32_t pack[PF_ROWS] = {};
    for (int c = 0; c < 4; ++c) {
      const int x = 4 * q + c;
      if (x >= Wo) break;
      const int xs = min(bounds[2 * x + 1], min(ksize, W));          // the host checks the tables; the clamps keep a wrong one inside LDS
      const int xmin = max(0, min(bounds[2 * x], W - xs));
      const int32_t* k = coef + (int64_t)x * ksize;
      int32_t acc[PF_ROWS];
#pragma unroll
      for (int r = 0; r < PF_ROWS; ++r) acc[r] = 1 << 21;
      for (int i = 0; i < xs; ++i) {
        const int32_t kv = k[i];
#pragma unroll
        for (int r = 0; r < PF_ROWS; ++r) acc[r] += kv * (int32_t)grey[r * gs + xmin + i];          // rows >= nr: stale LDS, never stored
      }
#pragma unroll
      for (int r = 0; r < PF_ROWS; ++r) pack[r] |= pf_clip8(acc[r]) << (8 * c);
    }
#pragma unroll
    for (int r = 0; r < PF_ROWS; ++r)
      if (r < nr) reinterpret_cast<uint32_t*>(tmp + ((int64_t)j * rows + r0 + r) * ldt)[q] = pack[r];          // ldt % 4 == 0, 4 q < ldt
  }
}

// ---- vertical pass + table ---------------------------------------------------------------------------------------------------------
// Block (y, j): output row y of frame j; its bounds and coefficients are the same for every lane (scalar loads).  A lane owns 4
// consecutive columns: one dword of tmp per tap, four integer sums, four table values, one 16-byte store when rows of Wo floats keep
// that alignment.
__global__ __launch_bounds__(PF_THREADS) void piano_resize_v_kernel(const uint8_t* __restrict__ tmp, int rows, int ldt, int Ho, int Wo,
                                                                    const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                                    int ksize, const float* __restrict__ lut, float* __restrict__ out) {
  __shared__ float tab[256];
  tab[threadIdx.x] = lut[threadIdx.x];          // PF_THREADS == 256
  __syncthreads();
  const int y = blockIdx.x;
  const int64_t j = blockIdx.y;
  const int ys = min(bounds[2 * y + 1], min(ksize, rows));          // the host checks the tables; the clamps keep a wrong one inside tmp
  const int ymin = max(0, min(bounds[2 * y], rows - ys));
  const int32_t* k = coef + (int64_t)y * ksize;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tmp + (j * rows + ymin) * (int64_t)ldt);
  const int ld4 = ldt >> 2;
  float* o = out + (j * Ho + y) * (int64_t)Wo;
  for (int q = threadIdx.x; 4 * q < Wo; q += PF_THREADS) {
    int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
#pragma unroll 4
    for (int i = 0; i < ys; ++i) {
      const uint32_t w = src[(int64_t)i * ld4 + q];
      const int32_t kv = k[i];
      a0 += kv * (int32_t)(w & 255);
      a1 += kv * (int32_t)((w >> 8) & 255);
      a2 += kv * (int32_t)((w >> 16) & 255);
      a3 += kv * (int32_t)(w >> 24);
    }
    const f32x4 v = {tab[pf_clip8(a0)], tab[pf_clip8(a1)], tab[pf_clip8(a2)], tab[pf_clip8(a3)]};
    if ((Wo & 3) == 0) {
      *reinterpret_cast<f32x4*>(o + 4 * q) = v;
    } else {
      for (int c = 0; c < 4 && 4 * q + c < Wo; ++c) o[4 * q + c] = v[c];
    }
  }
}

// ---- vertical pass + table, transposed store (the 88-key configuration's portrait frames) ------------------------------------------
// Block (band, j): output rows y = PF_BAND * band ... of frame j, all Wo columns.  Phase 1: an item is (row yy of the band, 4
// consecutive columns): the sums of piano_resize_v_kernel, whose 4 table values go to the LDS tile [x][yy] (pitch PF_BAND + 1:
// lanes on consecutive column quads land 4 * (PF_BAND + 1) words apart, 4 banks on, so at most 4 lanes of a 32-lane half share a bank;
// at pitch PF_BAND every lane of a row would; the reads of phase 2 hit 32 distinct banks).  Phase 2: an item is
// (column x, 4 consecutive yy): out[j][x][y ...] is contiguous along y, so a lane stores 16 bytes and 8 lanes cover a band's run
// of 128 bytes; rows of Ho floats keep the alignment when Ho % 4 == 0 (PF_BAND % 4 == 0).
constexpr int PF_BAND = 32;

__global__ __launch_bounds__(PF_THREADS) void piano_vpass_transposed_kernel(const uint8_t* __restrict__ tmp, int rows, int ldt, int Ho, int Wo,
                                                                     const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                                     int ksize, const float* __restrict__ lut, float* __restrict__ out) {
  extern __shared__ float pf_tile[];          // Wo rows of PF_BAND + 1 floats
  __shared__ float tab[256];
  tab[threadIdx.x] = lut[threadIdx.x];          // PF_THREADS == 256
  __syncthreads();
  constexpr int P = PF_BAND + 1;
  const int yb = blockIdx.x * PF_BAND;
  const int nb = min(PF_BAND, Ho - yb);
  const int64_t j = blockIdx.y;
  const int Q = (Wo + 3) >> 2;
  const int ld4 = ldt >> 2;
  for (int it = threadIdx.x; it < nb * Q; it += PF_THREADS) {
    const int yy = it / Q, q = it - yy * Q;
    const int y = yb + yy;
    const int ys = min(bounds[2 * y + 1], min(ksize, rows));          // the host checks the tables; the clamps keep a wrong one inside tmp
    const int ymin = max(0, min(bounds[2 * y], rows - ys));
    const int32_t* k = coef + (int64_t)y * ksize;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tmp + (j * rows + ymin) * (int64_t)ldt) + q;          // 4 q < ldt
    int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
#pragma unroll 4
    for (int i = 0; i < ys; ++i) {
      const uint32_t w = src[(int64_t)i * ld4];
      const int32_t kv = k[i];
      a0 += kv * (int32_t)(w & 255);
      a1 += kv * (int32_t)((w >> 8) & 255);
      a2 += kv * (int32_t)((w >> 16) & 255);
      a3 += kv * (int32_t)(w >> 24);
    }
    const float v[4] = {tab[pf_clip8(a0)], tab[pf_clip8(a1)], tab[pf_clip8(a2)], tab[pf_clip8(a3)]};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (4 * q + c < Wo) pf_tile[(4 * q + c) * P + yy] = v[c];
  }
  __syncthreads();
  float* o = out + j * (int64_t)Wo * Ho + yb;
  const int G = PF_BAND / 4;
  for (int it = threadIdx.x; it < Wo * G; it += PF_THREADS) {
    const int x = it / G, y4 = 4 * (it - x * G);
    if (y4 >= nb) continue;
    const float* t = pf_tile + x * P + y4;
    float* dst = o + (int64_t)x * Ho + y4;
    if ((Ho & 3) == 0 && y4 + 4 <= nb) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{t[0], t[1], t[2], t[3]};
    } else {
      for (int c = 0; c < 4 && y4 + c < nb; ++c) dst[c] = t[c];
    }
  }
}

}  // namespace

extern "C" int v2a_piano_resize_h(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const int32_t* sel, int32_t n, uint8_t* tmp,
                                  int32_t ldt, int32_t y0, int32_t rows, int32_t Wo, const int32_t* bounds, const int32_t* coef,
                                  int32_t ksize, v2a_stream_t stream) {
  V2A_REQUIRE(frames && tmp && bounds && coef, "v2a_piano_resize_h: null pointer");
  V2A_REQUIRE(F > 0 && H > 0 && W > 0 && Wo > 0 && ksize > 0 && rows > 0 && y0 >= 0 && y0 + rows <= H,
              "v2a_piano_resize_h: F=%d H=%d W=%d Wo=%d rows [%d, %d) ksize=%d", F, H, W, Wo, y0, y0 + rows, ksize);
  V2A_REQUIRE(n > 0 && n <= 65535 && (sel || n <= F), "v2a_piano_resize_h: n=%d frames per call (1..65535, and <= F=%d without sel)", n, F);
  V2A_REQUIRE(ldt >= Wo && ldt % 4 == 0, "v2a_piano_resize_h: ldt=%d must be a multiple of 4 and >= Wo=%d", ldt, Wo);
  V2A_REQUIRE(((uintptr_t)frames & 3) == 0 && ((uintptr_t)tmp & 3) == 0, "v2a_piano_resize_h: frames and tmp must be 4-byte aligned");
  const size_t lds = (size_t)PF_ROWS * ((W + 3) / 4) * 4;
  V2A_REQUIRE(lds <= 64 * 1024, "v2a_piano_resize_h: W=%d needs %zu bytes of LDS (limit 65536)", W, lds);
  const dim3 grid((unsigned)((rows + PF_ROWS - 1) / PF_ROWS), (unsigned)n);
  hipLaunchKernelGGL(piano_resize_h_kernel, grid, dim3(PF_THREADS), lds, (hipStream_t)stream, frames, (int64_t)F * H * W * 3, H, W, sel, tmp,
                     ldt, y0, rows, Wo, bounds, coef, ksize);
  return v2a_check_launch("v2a_piano_resize_h");
}

extern "C" int v2a_piano_resize_v(const uint8_t* tmp, int32_t n, int32_t rows, int32_t ldt, int32_t Ho, int32_t Wo, const int32_t* bounds,
                                  const int32_t* coef, int32_t ksize, const float* lut, float* out, v2a_stream_t stream) {
  V2A_REQUIRE(tmp && bounds && coef && lut && out, "v2a_piano_resize_v: null pointer");
  V2A_REQUIRE(n > 0 && n <= 65535 && rows > 0 && Ho > 0 && Wo > 0 && ksize > 0, "v2a_piano_resize_v: n=%d rows=%d Ho=%d Wo=%d ksize=%d", n, rows,
              Ho, Wo, ksize);
  V2A_REQUIRE(ldt >= Wo && ldt % 4 == 0, "v2a_piano_resize_v: ldt=%d must be a multiple of 4 and >= Wo=%d", ldt, Wo);
  V2A_REQUIRE(((uintptr_t)tmp & 3) == 0 && ((uintptr_t)out & (Wo % 4 == 0 ? 15 : 3)) == 0,
              "v2a_piano_resize_v: tmp must be 4-byte aligned and out 16-byte aligned (4-byte when Wo %% 4 != 0)");
  hipLaunchKernelGGL(piano_resize_v_kernel, dim3((unsigned)Ho, (unsigned)n), dim3(PF_THREADS), 0, (hipStream_t)stream, tmp, rows, ldt, Ho, Wo,
                     bounds, coef, ksize, lut, out);
  return v2a_check_launch("v2a_piano_resize_v");
}

extern "C" int v2a_piano_resize_vt(const uint8_t* tmp, int32_t n, int32_t rows, int32_t ldt, int32_t Ho, int32_t Wo, const int32_t* bounds,
                                   const int32_t* coef, int32_t ksize, const float* lut, float* out, v2a_stream_t stream) {
  V2A_REQUIRE(tmp && bounds && coef && lut && out, "v2a_piano_resize_vt: null pointer");
  V2A_REQUIRE(n > 0 && n <= 65535 && rows > 0 && Ho > 0 && Wo > 0 && ksize > 0, "v2a_piano_resize_vt: n=%d rows=%d Ho=%d Wo=%d ksize=%d", n, rows,
              Ho, Wo, ksize);
  V2A_REQUIRE(ldt >= Wo && ldt % 4 == 0, "v2a_piano_resize_vt: ldt=%d must be a multiple of 4 and >= Wo=%d", ldt, Wo);
  V2A_REQUIRE(((uintptr_t)tmp & 3) == 0 && ((uintptr_t)out & (Ho % 4 == 0 ? 15 : 3)) == 0,
              "v2a_piano_resize_vt: tmp must be 4-byte aligned and out 16-byte aligned (4-byte when Ho %% 4 != 0)");
  const size_t lds = (size_t)Wo * (PF_BAND + 1) * sizeof(float);
  V2A_REQUIRE(lds + 256 * sizeof(float) <= 64 * 1024, "v2a_piano_resize_vt: Wo=%d needs %zu bytes of LDS (limit 65536 with the table)", Wo, lds);
  const dim3 grid((unsigned)((Ho + PF_BAND - 1) / PF_BAND), (unsigned)n);
  hipLaunchKernelGGL(piano_vpass_transposed_kernel, grid, dim3(PF_THREADS), lds, (hipStream_t)stream, tmp, rows, ldt, Ho, Wo, bounds, coef, ksize,
                     lut, out);
  return v2a_check_launch("v2a_piano_resize_vt");
}
