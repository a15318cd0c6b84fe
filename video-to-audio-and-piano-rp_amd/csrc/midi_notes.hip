// Note extraction from a piano key roll: the link of the reference's Audeo chain behind Roll2Midi (src/audeo/Midi_synth.py).
//
//   process_midi / process_roll (Midi_synth.py:33-95)   binarise the roll and mark, per frame j and key, an onset (+1) where the key is
//                                                        on at j and off at j - 1 (or j = 0), an offset (-1) where it was on at j - 1
//                                                        and is off at j -- the reference's two `np.setdiff1d` per frame
//   GetNote (Midi_synth.py:97-118)                       per key, the k-th onset paired with the k-th offset; a key still sounding at
//                                                        the end gets end = T (`np.append(end, tmp.shape)`)
//
// One workgroup per clip, one launch, no atomics.  The roll goes through LDS in tiles of NOTES_TILE frames: every thread reads
// elements in the order in which they lie in memory (keys innermost for a (b, t, K) roll, frames innermost for a (b, K, t) view) and
// stores one byte per (key, frame), key-major.  A wave then takes a key: lane l reads frame 64 w + l of word w, a wave64 ballot makes
// the 64-frame on-mask m, and with p = m shifted up by one frame with the previous frame's bit carried in (across words and tiles)
//   rises = m & ~p,   falls = ~m & p.
// Frames at or beyond the clip's length count as off and the tiles run one frame past it, so a note still sounding at the end falls
// at frame `len`: the reference's appended end, with no special case.  Pass 1 counts the rises per key; one wave scans the counts
// over the keys into offsets; pass 2 walks the tiles again and the lane that holds a rise (fall) bit stores the frame as the start
// (end) of row offset + base + popcount(lower lanes' bits), base being the key's rises (falls) so far.  The k-th rise and the k-th
// fall of a key thus meet in one row: rows ordered by key, then by start.
#include "v2a_common.h"

namespace {

constexpr int NOTES_THREADS = 1024;             // 16 waves: the staging loads of a tile are latency-bound, so many are kept in flight
constexpr int NOTES_WAVES = NOTES_THREADS / V2A_WAVE;
constexpr int NOTES_TILE = V2A_ROLL_NOTES_TILE;              // frames per LDS tile
constexpr int NOTES_WORDS = NOTES_TILE / 64;
constexpr int NOTES_PITCH = NOTES_TILE + 4;                  // bytes per key row: 65 dwords, so the key-innermost staging stores spread over the banks
constexpr int NOTES_MAX_KEYS = V2A_ROLL_NOTES_MAX_KEYS;
constexpr int NOTES_UNROLL = 4;                              // staging loads a thread issues before it stores any

struct RollView {
  const void* base;
  int64_t frame_stride, key_stride;                         // elements
  float threshold;
};

template <bool F32>
__device__ __forceinline__ uint8_t roll_on(const RollView& r, int64_t frame, int32_t key) {
  const int64_t e = frame * r.frame_stride + (int64_t)key * r.key_stride;
  if (F32) return ((const float*)r.base)[e] > r.threshold ? 1 : 0;          // a NaN is off
  return ((const uint8_t*)r.base)[e] != 0 ? 1 : 0;
}

// frames [t0, t0 + NOTES_TILE) of every key -> on[key][frame - t0]; frames at or beyond len are off and are not read
template <bool F32>
__device__ __forceinline__ void stage_tile(const RollView& r, uint8_t* on, int32_t keys, int64_t t0, int64_t len, bool keys_innermost) {
  // element i of the tile = (outer o, inner a) with the inner index running over what lies contiguous in memory; thread t takes
  // i = t, t + NOTES_THREADS, ...: one division per thread, then (o, a) advance by a fixed step with one carry
  const int32_t inner = keys_innermost ? keys : NOTES_TILE, outer = keys_innermost ? NOTES_TILE : keys;
  const int32_t dq = NOTES_THREADS / inner, dr = NOTES_THREADS - dq * inner;
  int32_t o = threadIdx.x / inner, a = threadIdx.x - o * inner;
  while (o < outer) {
    uint8_t v[NOTES_UNROLL];
    int32_t at[NOTES_UNROLL];
#pragma unroll
    for (int u = 0; u < NOTES_UNROLL; ++u) {                // the loads of a round first: independent, all in flight together
      at[u] = -1;
      v[u] = 0;
      if (o < outer) {
        const int32_t k = keys_innermost ? a : o, f = keys_innermost ? o : a;
        const int64_t frame = t0 + f;
        at[u] = k * NOTES_PITCH + f;
        if (frame < len) v[u] = roll_on<F32>(r, frame, k);
      }
      a += dr;
      o += dq;
      if (a >= inner) {
        a -= inner;
        ++o;
      }
    }
#pragma unroll
    for (int u = 0; u < NOTES_UNROLL; ++u)
      if (at[u] >= 0) on[at[u]] = v[u];
  }
}

template <bool F32>
__global__ __launch_bounds__(NOTES_THREADS) void roll_notes_kernel(const void* roll, int64_t batch_stride, int64_t frame_stride, int64_t key_stride,
                                                                   float threshold, int32_t T, int32_t keys, const int32_t* __restrict__ lens,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ totals,
                                                                   int32_t* __restrict__ notes, int32_t cap, int8_t* __restrict__ onset) {
  __shared__ uint8_t s_on[NOTES_MAX_KEYS * NOTES_PITCH];
  __shared__ int32_t s_prev[NOTES_MAX_KEYS];                // the key's bit of the frame in front of the tile
  __shared__ int32_t s_rises[NOTES_MAX_KEYS];               // rises so far (pass 1: the count; pass 2: the running base of the starts)
  __shared__ int32_t s_falls[NOTES_MAX_KEYS];               // pass 2: the running base of the ends
  __shared__ int32_t s_offset[NOTES_MAX_KEYS];              // first row of the key

  const int32_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t len = T;
  if (lens) {
    const int32_t l = lens[b];
    len = l < 0 ? 0 : (l > T ? T : l);
  }
  RollView r;
  r.base = F32 ? (const void*)((const float*)roll + (int64_t)b * batch_stride) : (const void*)((const uint8_t*)roll + (int64_t)b * batch_stride);
  r.frame_stride = frame_stride;
  r.key_stride = key_stride;
  r.threshold = threshold;
  const int64_t akey = key_stride < 0 ? -key_stride : key_stride, aframe = frame_stride < 0 ? -frame_stride : frame_stride;
  const bool keys_innermost = akey <= aframe;
  // one frame past the clip, where a sounding note falls; with an onset matrix every frame of it is written, so the tiles reach T
  const int64_t frames = (onset && (int64_t)T > len + 1) ? (int64_t)T : len + 1;
  const uint64_t below = ((uint64_t)1 << lane) - 1;

  for (int pass = 0; pass < 2; ++pass) {
    for (int32_t k = threadIdx.x; k < NOTES_MAX_KEYS; k += NOTES_THREADS) {
      s_prev[k] = 0;
      s_rises[k] = 0;
      s_falls[k] = 0;
    }
    for (int64_t t0 = 0; t0 < frames; t0 += NOTES_TILE) {
      __syncthreads();                                      // the tile in front has been read; the resets above are visible
      stage_tile<F32>(r, s_on, keys, t0, len, keys_innermost);
      __syncthreads();
      for (int32_t k = wave; k < keys; k += NOTES_WAVES) {  // wave-uniform: all 64 lanes reach every ballot
        uint64_t prev = (uint64_t)s_prev[k];
        int32_t nr = s_rises[k], nf = s_falls[k];
        const int32_t row0 = pass ? s_offset[k] : 0;
#pragma unroll
        for (int w = 0; w < NOTES_WORDS; ++w) {
          if (t0 + 64 * w >= frames) break;                 // wave-uniform
          const uint64_t m = __ballot(s_on[k * NOTES_PITCH + 64 * w + lane] != 0);
          const uint64_t p = (m << 1) | prev;
          const uint64_t rises = m & ~p, falls = ~m & p;
          prev = m >> 63;
          if (pass) {
            const int64_t frame = t0 + 64 * w + lane;
            const bool rise = (rises >> lane) & 1, fall = (falls >> lane) & 1;
            if (rise) {
              const int64_t row = (int64_t)row0 + nr + __popcll(rises & below);
              if (row < cap) {
                int32_t* dst = notes + ((int64_t)b * cap + row) * 3;
                dst[0] = k;
                dst[1] = (int32_t)frame;
              }
            }
            if (fall) {
              const int64_t row = (int64_t)row0 + nf + __popcll(falls & below);
              if (row < cap) notes[((int64_t)b * cap + row) * 3 + 2] = (int32_t)frame;
            }
            if (onset && frame < T) onset[((int64_t)b * keys + k) * T + frame] = rise ? (int8_t)1 : (fall ? (int8_t)-1 : (int8_t)0);
          }
          nr += __popcll(rises);
          nf += __popcll(falls);
        }
        if (lane == 0) {
          s_prev[k] = (int32_t)prev;
          s_rises[k] = nr;
          s_falls[k] = nf;
        }
      }
    }
    if (pass) break;
    __syncthreads();
    if (wave == 0) {                                        // exclusive scan of the counts over the keys: lane l takes keys l and 64 + l
      const int32_t c0 = lane < keys ? s_rises[lane] : 0, c1 = 64 + lane < keys ? s_rises[64 + lane] : 0;
      int32_t s0 = c0, s1 = c1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t u0 = __shfl_up(s0, o, 64), u1 = __shfl_up(s1, o, 64);
        if (lane >= o) {
          s0 += u0;
          s1 += u1;
        }
      }
      const int32_t low = __shfl(s0, 63, 64), high = __shfl(s1, 63, 64);
      s_offset[lane] = s0 - c0;
      s_offset[64 + lane] = low + s1 - c1;
      if (lane < keys) counts[(int64_t)b * keys + lane] = c0;
      if (64 + lane < keys) counts[(int64_t)b * keys + 64 + lane] = c1;
      if (lane == 0) totals[b] = low + high;
    }
    __syncthreads();                                        // offsets before the resets of pass 2 and its reads
  }
}

}  // namespace

extern "C" int v2a_roll_notes(const void* roll, int32_t elem_bytes, int64_t batch_stride, int64_t frame_stride, int64_t key_stride, float threshold,
                              int32_t B, int32_t T, int32_t keys, const int32_t* lens, int32_t* counts, int32_t* totals, int32_t* notes, int32_t cap,
                              int8_t* onset, v2a_stream_t stream) {
  V2A_REQUIRE(roll && counts && totals, "v2a_roll_notes: null pointer");
  V2A_REQUIRE(elem_bytes == 1 || elem_bytes == 4, "v2a_roll_notes: elem_bytes=%d (1: bytes, on iff != 0; 4: fp32, on iff > threshold)", elem_bytes);
  V2A_REQUIRE(B >= 1 && T >= 1 && keys >= 1 && keys <= V2A_ROLL_NOTES_MAX_KEYS, "v2a_roll_notes: B=%d T=%d keys=%d (keys <= %d)", B, T, keys,
              V2A_ROLL_NOTES_MAX_KEYS);
  V2A_REQUIRE(T <= V2A_ROLL_NOTES_MAX_FRAMES, "v2a_roll_notes: T=%d (at most %d frames: the rows of a clip are counted in int32)", T, V2A_ROLL_NOTES_MAX_FRAMES);
  V2A_REQUIRE(cap >= 0 && (cap == 0 || notes), "v2a_roll_notes: cap=%d rows without a notes buffer", cap);
  V2A_REQUIRE(elem_bytes == 1 || ((uintptr_t)roll & 3) == 0, "v2a_roll_notes: alignment (4 bytes for an fp32 roll)");
  V2A_REQUIRE((((uintptr_t)counts | (uintptr_t)totals | (uintptr_t)notes | (uintptr_t)lens) & 3) == 0, "v2a_roll_notes: alignment (4 bytes for the int32 buffers)");
  if (elem_bytes == 4)
    hipLaunchKernelGGL(roll_notes_kernel<true>, dim3(B), dim3(NOTES_THREADS), 0, (hipStream_t)stream, roll, batch_stride, frame_stride, key_stride, threshold, T,
                       keys, lens, counts, totals, notes, cap, onset);
  else
    hipLaunchKernelGGL(roll_notes_kernel<false>, dim3(B), dim3(NOTES_THREADS), 0, (hipStream_t)stream, roll, batch_stride, frame_stride, key_stride, threshold, T,
                       keys, lens, counts, totals, notes, cap, onset);
  return v2a_check_launch("v2a_roll_notes");
}
