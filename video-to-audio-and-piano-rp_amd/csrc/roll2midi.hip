// Roll2Midi generator (src/audeo/Roll2MidiNet.py:42-87, `r2m`): the three memory-bound kernels around its conv-as-GEMM path, and the
//   attention gate of its enhanced variant (src/audeo/Roll2MidiNet_enhance.py:41-55, `enh`) as a fourth.
//   The U-Net keeps the roll's size (every convolution is 3x3, stride 1, pad 1), so all maps share one (n, H, W) pixel grid:
//   NHWC fp32, optionally stored with a zero border (the implicit-GEMM layout of v2a_gemm's offset tables) and optionally as a
//   channel slice of a wider map (the skip concatenations r2m:38 are never materialised).  A pixel (n, y, x) of a slice is at
//     base + ((n*(H + 2b) + y + b)*(W + 2b) + x + b) * pitch,   base = map + channel offset, pitch = channels of the whole map.
//   stem: down1 (1 -> co channels, K = 9 does not fill a GEMM K tile); leaky_shadow: the LeakyReLU(0.2) the GEMM epilogue lacks,
//   with the bf16 / hi | lo copy the next convolution reads; head: conv1d (1x1, 80 -> 1) + sigmoid + threshold.
#include "v2a_common.h"

namespace {

constexpr int SH_NONE = 0, SH_BF16 = 1, SH_SPLIT = 2;
constexpr float LEAKY = 0.2f;

__device__ __forceinline__ float leaky_f(float v) { return v > 0.f ? v : v * LEAKY; }

// 8 consecutive channels: fp32 to out + o, their bf16 copy (MODE 1) or hi = bf16(v), lo = bf16(v - hi) lo_off further (MODE 2) to sh + o
template <int MODE>
__device__ __forceinline__ void store8(float* __restrict__ out, bf16_t* __restrict__ sh, int64_t o, int64_t lo_off, float (&v)[8]) {
  *reinterpret_cast<f32x4*>(out + o) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(out + o + 4) = f32x4{v[4], v[5], v[6], v[7]};
  if constexpr (MODE != SH_NONE) {
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // the split of the STORED fp32 value: without the barrier -ffp-contract=fast fuses the leaky scaling into the subtraction
      float a = v[e];
      asm volatile("" : "+v"(a));
      hi[e] = (bf16_t)a;
      if constexpr (MODE == SH_SPLIT) lo[e] = (bf16_t)(a - (float)hi[e]);
    }
    *reinterpret_cast<bf16x8*>(sh + o) = hi;
    if constexpr (MODE == SH_SPLIT) *reinterpret_cast<bf16x8*>(sh + lo_off + o) = lo;
  }
}

__device__ __forceinline__ int64_t pixel_of(int64_t t, int H, int W, int b) {      // t = (n*H + y)*W + x -> bordered pixel index
  const int x = (int)(t % W);
  t /= W;
  const int y = (int)(t % H);
  const int64_t n = t / H;
  return (n * (H + 2 * b) + y + b) * (W + 2 * b) + x + b;
}

// ---- down1: one thread per (pixel, 8 output channels); wt[tap][co], taps in (ky, kx) order, one fma chain from tap 0 up ----------
template <int MODE>
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ x, const float* __restrict__ wt, float* __restrict__ out,
                                                   bf16_t* __restrict__ sh, int64_t total, int H, int W, int co, int64_t pitch,
                                                   int border, int64_t lo_off) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int C8 = co / 8;
  const int c = (int)(gid % C8) * 8;
  const int64_t t = gid / C8;
  const int xo = (int)(t % W);
  const int yo = (int)((t / W) % H);
  const int64_t img = (t / W / H) * H * W;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yi = yo + tap / 3 - 1, xi = xo + tap % 3 - 1;
    const float v = (yi >= 0 && yi < H && xi >= 0 && xi < W) ? x[img + (int64_t)yi * W + xi] : 0.f;
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt + tap * co + c);
    const f32x4 w1 = *reinterpret_cast<const f32x4*>(wt + tap * co + c + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = fmaf(w0[e], v, acc[e]);
      acc[4 + e] = fmaf(w1[e], v, acc[4 + e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = leaky_f(acc[e]);
  store8<MODE>(out, sh, pixel_of(t, H, W, border) * pitch + c, lo_off, acc);
}

// ---- LeakyReLU(0.2) in place + shadow: one thread per (pixel, 8 channels) --------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void leaky_shadow_kernel(float* __restrict__ x, bf16_t* __restrict__ sh, int64_t total, int H, int W,
                                                           int C, int64_t pitch, int border, int64_t lo_off) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int C8 = C / 8;
  const int c = (int)(gid % C8) * 8;
  const int64_t o = pixel_of(gid / C8, H, W, border) * pitch + c;
  const f32x4 a = *reinterpret_cast<const f32x4*>(x + o), b = *reinterpret_cast<const f32x4*>(x + o + 4);
  float v[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = leaky_f(a[e]);
    v[4 + e] = leaky_f(b[e]);
  }
  store8<MODE>(x, sh, o, lo_off, v);
}

// ---- conv1d (1x1 over [u | d]) + sigmoid + threshold: one thread per pixel, one fma chain: bias, u channels up, d channels up -----
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ u, int64_t u_pitch, int nu, const float* __restrict__ d,
                                                   int64_t d_pitch, int nd, const float* __restrict__ w, float bias, float threshold,
                                                   int64_t total, int H, int W, int border, float* __restrict__ logits,
                                                   float* __restrict__ probs, uint8_t* __restrict__ midi) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int64_t px = pixel_of(gid, H, W, border);
  const float* up = u + px * u_pitch;
  const float* dp = d + px * d_pitch;
  float acc = bias;
  for (int c = 0; c < nu; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(up + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(w[c + e], v[e], acc);
  }
  for (int c = 0; c < nd; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(dp + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(w[nu + c + e], v[e], acc);
  }
  if (logits) logits[gid] = acc;
  const float p = 1.0f / (1.0f + expf(-acc));        // libm expf, IEEE division: the parity form (r2m:86)
  if (probs) probs[gid] = p;
  if (midi) midi[gid] = p >= threshold ? 1 : 0;
}

// ---- attention gate of Roll2MidiNet_enhance.py (enh:41-55), folded into one weight vector: one wave per pixel ------------------------
// The pixel's C = C0 + C1 channels are the concatenation of two segments.  Lane l owns the 8 channels [512 j + 8 l, + 8) of chunk j
// (NCH chunks, held in registers between the dot and the scaling: every element is read once).  Per lane one fma chain from 0 over
// its channels in ascending order, then an xor butterfly (32, 16, 8, 4, 2, 1) after which every lane holds the same sum; z = sum +
// bias.  The order depends on (C0, C1) alone.  8 channels per lane, as in leaky_shadow_kernel, so that the shadow goes out 16 bytes
// wide through store8.
constexpr int GATE_MAX_C = 2048;      // 4 chunks x 64 lanes x 8 channels: 32 data registers per lane

template <int MODE, int NCH>
__global__ __launch_bounds__(256) void gate_kernel(float* x0, int64_t pitch0, int C0, bf16_t* sh0, int64_t lo0, float* x1, int64_t pitch1,
                                                   int C1, bf16_t* sh1, int64_t lo1, const float* __restrict__ w, float bias,
                                                   int64_t total, int H, int W, int border, float* __restrict__ logits,
                                                   float* __restrict__ alpha_out) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // one wave per pixel: uniform over the wave
  if (t >= total) return;
  const int lane = threadIdx.x & 63;
  const int C = C0 + C1;
  const int64_t px = pixel_of(t, H, W, border);
  float v[NCH][8];
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = j * 512 + lane * 8;                                    // C0 % 8 == 0: the 8 channels lie in one segment
    if (c < C) {
      const float* p = c < C0 ? x0 + px * pitch0 + c : x1 + px * pitch1 + (c - C0);
      const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
      const f32x4 wa = *reinterpret_cast<const f32x4*>(w + c), wb = *reinterpret_cast<const f32x4*>(w + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[j][e] = a[e];
        v[j][4 + e] = b[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(wa[e], a[e], acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(wb[e], b[e], acc);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  const float z = acc + bias;
  const float al = 1.0f / (1.0f + expf(-z));         // libm expf, IEEE division: the parity form of head_kernel
  if (lane == 0) {
    if (logits) logits[t] = z;
    if (alpha_out) alpha_out[t] = al;
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = j * 512 + lane * 8;
    if (c < C) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] *= al;      // one fp32 multiply of the stored x; store8 splits the STORED product
      if (c < C0)
        store8<MODE>(x0, sh0, px * pitch0 + c, lo0, v[j]);
      else
        store8<MODE>(x1, sh1, px * pitch1 + (c - C0), lo1, v[j]);
    }
  }
}

template <int MODE>
void launch_gate(int nch, dim3 grid, hipStream_t s, float* x0, int64_t pitch0, int C0, bf16_t* sh0, int64_t lo0, float* x1, int64_t pitch1,
                 int C1, bf16_t* sh1, int64_t lo1, const float* w, float bias, int64_t total, int H, int W, int border, float* logits,
                 float* alpha) {
  dim3 block(256);
  if (nch == 1)
    hipLaunchKernelGGL((gate_kernel<MODE, 1>), grid, block, 0, s, x0, pitch0, C0, sh0, lo0, x1, pitch1, C1, sh1, lo1, w, bias, total, H, W,
                       border, logits, alpha);
  else if (nch == 2)
    hipLaunchKernelGGL((gate_kernel<MODE, 2>), grid, block, 0, s, x0, pitch0, C0, sh0, lo0, x1, pitch1, C1, sh1, lo1, w, bias, total, H, W,
                       border, logits, alpha);
  else
    hipLaunchKernelGGL((gate_kernel<MODE, 4>), grid, block, 0, s, x0, pitch0, C0, sh0, lo0, x1, pitch1, C1, sh1, lo1, w, bias, total, H, W,
                       border, logits, alpha);
}

// geometry shared by the entry points; `what` prefixes the message
int check_slice(const char* what, const void* base, const void* shadow, int32_t mode, int64_t lo_offset, int32_t n, int32_t H, int32_t W,
                int32_t C, int64_t pitch, int32_t border) {
  V2A_REQUIRE(base != nullptr && ((uintptr_t)base & 15) == 0, "%s: null or misaligned map pointer", what);
  V2A_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && border >= 0, "%s: bad geometry (n=%d H=%d W=%d C=%d border=%d)", what, n, H, W, C,
              border);
  V2A_REQUIRE(pitch >= C && pitch % 8 == 0, "%s: pitch %lld must be >= C=%d and a multiple of 8", what, (long long)pitch, C);
  V2A_REQUIRE(mode == SH_NONE || mode == SH_BF16 || mode == SH_SPLIT, "%s: shadow mode %d (0 none, 1 bf16, 2 hi | lo planes)", what, mode);
  V2A_REQUIRE((mode == SH_NONE) == (shadow == nullptr) && ((uintptr_t)shadow & 15) == 0, "%s: shadow pointer does not go with shadow mode %d", what,
              mode);
  const int64_t plane = (int64_t)n * (H + 2 * border) * (W + 2 * border) * pitch;
  V2A_REQUIRE(((int64_t)n * H * W * (C / 8) + 255) / 256 < 0x7fffffffLL, "%s: too many pixels for one launch", what);
  if (mode == SH_SPLIT)
    V2A_REQUIRE(lo_offset >= plane - (pitch - C) && lo_offset % 8 == 0, "%s: lo_offset %lld must cover the hi plane (%lld elements) and be a multiple of 8",
                what, (long long)lo_offset, (long long)plane);
  else
    V2A_REQUIRE(lo_offset == 0, "%s: lo_offset goes with shadow mode 2", what);
  return V2A_OK;
}

}  // namespace

extern "C" int v2a_roll2midi_stem(const float* x, const float* wt, int32_t n, int32_t H, int32_t W, int32_t co, float* out, void* shadow,
                                  int32_t shadow_mode, int64_t lo_offset, int64_t pitch, int32_t border, v2a_stream_t stream) {
  V2A_REQUIRE(x && wt && ((uintptr_t)wt & 15) == 0, "v2a_roll2midi_stem: null roll or null / misaligned weight");
  if (int rc = check_slice("v2a_roll2midi_stem", out, shadow, shadow_mode, lo_offset, n, H, W, co, pitch, border)) return rc;
  const int64_t total = (int64_t)n * H * W * (co / 8);
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* sh = (bf16_t*)shadow;
  if (shadow_mode == SH_NONE)
    hipLaunchKernelGGL(stem_kernel<SH_NONE>, grid, block, 0, s, x, wt, out, sh, total, H, W, co, pitch, border, lo_offset);
  else if (shadow_mode == SH_BF16)
    hipLaunchKernelGGL(stem_kernel<SH_BF16>, grid, block, 0, s, x, wt, out, sh, total, H, W, co, pitch, border, lo_offset);
  else
    hipLaunchKernelGGL(stem_kernel<SH_SPLIT>, grid, block, 0, s, x, wt, out, sh, total, H, W, co, pitch, border, lo_offset);
  return v2a_check_launch("v2a_roll2midi_stem");
}

extern "C" int v2a_leaky_shadow(float* x, void* shadow, int32_t shadow_mode, int64_t lo_offset, int32_t n, int32_t H, int32_t W, int32_t C,
                                int64_t pitch, int32_t border, v2a_stream_t stream) {
  if (int rc = check_slice("v2a_leaky_shadow", x, shadow, shadow_mode, lo_offset, n, H, W, C, pitch, border)) return rc;
  const int64_t total = (int64_t)n * H * W * (C / 8);
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* sh = (bf16_t*)shadow;
  if (shadow_mode == SH_NONE)
    hipLaunchKernelGGL(leaky_shadow_kernel<SH_NONE>, grid, block, 0, s, x, sh, total, H, W, C, pitch, border, lo_offset);
  else if (shadow_mode == SH_BF16)
    hipLaunchKernelGGL(leaky_shadow_kernel<SH_BF16>, grid, block, 0, s, x, sh, total, H, W, C, pitch, border, lo_offset);
  else
    hipLaunchKernelGGL(leaky_shadow_kernel<SH_SPLIT>, grid, block, 0, s, x, sh, total, H, W, C, pitch, border, lo_offset);
  return v2a_check_launch("v2a_leaky_shadow");
}

extern "C" int v2a_roll2midi_gate(float* x0, int64_t pitch0, int32_t C0, void* shadow0, int64_t lo_offset0, float* x1, int64_t pitch1,
                                  int32_t C1, void* shadow1, int64_t lo_offset1, const float* w, float bias, int32_t shadow_mode, int32_t n,
                                  int32_t H, int32_t W, int32_t border, float* logits, float* alpha, v2a_stream_t stream) {
  V2A_REQUIRE(w != nullptr && ((uintptr_t)w & 15) == 0, "v2a_roll2midi_gate: null or misaligned weight vector");
  V2A_REQUIRE(C1 >= 0, "v2a_roll2midi_gate: bad geometry (C1=%d)", C1);
  if (int rc = check_slice("v2a_roll2midi_gate", x0, shadow0, shadow_mode, lo_offset0, n, H, W, C0, pitch0, border)) return rc;
  if (C1 > 0) {
    if (int rc = check_slice("v2a_roll2midi_gate (second segment)", x1, shadow1, shadow_mode, lo_offset1, n, H, W, C1, pitch1, border)) return rc;
  } else {
    V2A_REQUIRE(x1 == nullptr && shadow1 == nullptr && lo_offset1 == 0, "v2a_roll2midi_gate: C1 = 0 takes no second segment");
  }
  V2A_REQUIRE((int64_t)C0 + C1 <= GATE_MAX_C, "v2a_roll2midi_gate: C0 + C1 = %lld channels, one wave holds at most %d in registers (4 chunks of 64 lanes x 8)",
              (long long)C0 + C1, GATE_MAX_C);
  V2A_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)alpha & 3) == 0, "v2a_roll2midi_gate: misaligned logits / alpha");
  const int64_t total = (int64_t)n * H * W;
  V2A_REQUIRE((total + 3) / 4 < 0x7fffffffLL, "v2a_roll2midi_gate: too many pixels for one launch");
  const int C = C0 + C1;
  const int nch = C <= 512 ? 1 : (C <= 1024 ? 2 : 4);
  dim3 grid((unsigned)((total + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  bf16_t *s0 = (bf16_t*)shadow0, *s1 = (bf16_t*)shadow1;
  if (shadow_mode == SH_NONE)
    launch_gate<SH_NONE>(nch, grid, s, x0, pitch0, C0, s0, lo_offset0, x1, pitch1, C1, s1, lo_offset1, w, bias, total, H, W, border, logits, alpha);
  else if (shadow_mode == SH_BF16)
    launch_gate<SH_BF16>(nch, grid, s, x0, pitch0, C0, s0, lo_offset0, x1, pitch1, C1, s1, lo_offset1, w, bias, total, H, W, border, logits, alpha);
  else
    launch_gate<SH_SPLIT>(nch, grid, s, x0, pitch0, C0, s0, lo_offset0, x1, pitch1, C1, s1, lo_offset1, w, bias, total, H, W, border, logits, alpha);
  return v2a_check_launch("v2a_roll2midi_gate");
}

extern "C" int v2a_roll2midi_head(const float* u, int64_t u_pitch, int32_t nu, const float* d, int64_t d_pitch, int32_t nd, const float* w,
                                  float bias, float threshold, int32_t n, int32_t H, int32_t W, int32_t border, float* logits, float* probs,
                                  uint8_t* midi, v2a_stream_t stream) {
  V2A_REQUIRE(u && d && w && ((uintptr_t)u & 15) == 0 && ((uintptr_t)d & 15) == 0, "v2a_roll2midi_head: null or misaligned pointer");
  V2A_REQUIRE(n > 0 && H > 0 && W > 0 && border >= 0 && nu > 0 && nd > 0 && nu % 4 == 0 && nd % 4 == 0,
              "v2a_roll2midi_head: bad geometry (n=%d H=%d W=%d border=%d nu=%d nd=%d)", n, H, W, border, nu, nd);
  V2A_REQUIRE(u_pitch >= nu && d_pitch >= nd && u_pitch % 4 == 0 && d_pitch % 4 == 0, "v2a_roll2midi_head: pitches (%lld, %lld) must be >= (nu, nd) and multiples of 4",
              (long long)u_pitch, (long long)d_pitch);
  V2A_REQUIRE(logits || probs || midi, "v2a_roll2midi_head: no output requested");
  const int64_t total = (int64_t)n * H * W;
  V2A_REQUIRE((total + 255) / 256 < 0x7fffffffLL, "v2a_roll2midi_head: too many pixels for one launch");
  hipLaunchKernelGGL(head_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, u_pitch, nu, d, d_pitch, nd, w,
                     bias, threshold, total, H, W, border, logits, probs, midi);
  return v2a_check_launch("v2a_roll2midi_head");
}
