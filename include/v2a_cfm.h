/*
 * v2a_cfm.h -- C ABI of the MI355X (gfx950) kernels behind the flow-matching V2A sampler.
 *
 * The reference (acappemin/Video-to-Audio-and-Piano-RP) has no FFI/operator layer: the hot
 * path is a Python class API (E2TTS.sample / transformer_with_pred_head) whose arithmetic
 * runs as stock PyTorch ops.  Each entry point below therefore names the reference
 * *module/function* it replaces (file:line, `x3` = src/e2_tts_pytorch/e2_tts_crossatt3.py;
 * `xt` = third-party x-transformers==1.37.4, requirements.txt:19, call sites given).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name says `host`;
 *   - no allocation and no synchronisation inside: the caller owns every buffer and passes
 *     the stream; all launches are graph-capturable.  The only process-wide state is the
 *     explicit tile-selection override of v2a_set_tuning() (benchmarking aid, defaults =
 *     automatic) and per-kernel "large LDS" attributes set once, thread-safely, at the first
 *     launch of each kernel; nothing is read from the environment;
 *   - return value 0 = ok, negative = error; v2a_last_error() gives the message of the
 *     last failing call on the calling thread;
 *   - "compute dtype" T is V2A_F32 (parity mode, exact-fp32 MFMA) or V2A_BF16 (bf16
 *     operands, fp32 accumulate).  Residual streams are always fp32;
 *   - a "step vector" is a float vector selected per launch by a device-side step counter
 *     and per row by its batch:  v = base + step[0]*step_stride + batch*batch_stride,
 *     batch = row / rows_per_batch.  step may be NULL (= 0).  This is how the per-Euler-step
 *     AdaLN / AdaptiveRMSNorm modulation tables are addressed from ONE captured hipGraph.
 */
#ifndef V2A_CFM_H
#define V2A_CFM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* v2a_stream_t; /* hipStream_t */

enum {
  V2A_F32 = 0,
  V2A_BF16 = 1,
  /* split-bf16 operand layout (the "bf16x3" parity mode): a row of d fp32 values v is stored as 2*d bf16 values
   * [hi_0 .. hi_{d-1} | lo_0 .. lo_{d-1}], hi = bf16(v), lo = bf16(v - hi).  A GEMM on the concatenation
   * [A_hi | A_hi | A_lo] x [W_hi | W_lo | W_hi]^T (three K segments of v2a_gemm) then sums hi*hi + hi*lo + lo*hi in fp32:
   * fp32-grade products (relative error ~2^-16) at three bf16 MFMAs instead of one fp32 MFMA at 1/16 of the rate.
   * Accepted as y_dtype of v2a_rmsnorm and by v2a_split_bf16; never a compute dtype. */
  V2A_BF16_SPLIT = 2
};

enum {
  V2A_OK = 0,
  V2A_ERR_ARG = -1,    /* shape/alignment/enum the kernels do not support */
  V2A_ERR_LAUNCH = -2  /* hipGetLastError() after launch */
};

int v2a_abi_version(void);        /* 9 */
const char* v2a_last_error(void);

/* ---------------------------------------------------------------------------------------
 * GEMM with fused epilogues:  acc[m][n] = sum_k A[m][k] * W[n][k]      (nn.Linear layout)
 * A is the virtual concatenation along K of up to 3 row-major segments (so
 * TextAudioCrossCondition's pack((audio,text,frames)) x3:693-700 and the U-Net skip
 * torch.cat((x, skip)) x3:1116-1117 are never materialised).
 * Replaces: every nn.Linear on the path -- xt Attention.to_q/to_k/to_v/to_out (sites
 * x3:808,813,881,914), xt FeedForward (x3:817,884,917), TextAudioCrossCondition
 * x3:698-700, skip_proj x3:1117, to_pred x3:2083, AdaLNZero.to_gamma x3:550 and
 * AdaptiveRMSNorm.to_gamma (table build).
 * ------------------------------------------------------------------------------------- */
enum {
  V2A_EPI_STORE = 0,      /* out = acc + bias                                    */
  V2A_EPI_SIGMOID = 1,    /* out = sigmoid(acc + bias)            (AdaLNZero table) */
  V2A_EPI_GEGLU = 2,      /* W rows packed [16 value | 16 gate] per 16 outputs:
                             out[m][j] = (acc_v + b_v) * gelu_erf(acc_g + b_g); out has N/2 cols.  fp32 output: erff; bf16 and
                             V2A_BF16_SPLIT (hi | lo plane) output: erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 */
  V2A_EPI_RESID = 3,      /* out = resid + acc + bias             (text/frames streams, cross-condition) */
  V2A_EPI_GATE_RESID = 4, /* out = resid + gate[n] * (acc + bias) (AdaLNZero x3:546-551 + residual x3:1128) */
  V2A_EPI_GEGLU_TANH = 5, /* v2a_gemm_skinny_f32 only (v2a_gemm rejects it): the GEGLU row packing with value = wi_1, gate = wi_0,
                             out[m][j] = (acc_v + b_v) * gelu_new(acc_g + b_g), gelu_new(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) */
  V2A_EPI_GELU = 6,       /* ABI 8, additive: out = gelu_erf(acc + bias), gelu_erf(x) = 0.5 x (1 + erf(x / sqrt(2))) -- CLIPMLP.fc1 + activation_fn
                             of the CLIP image encoder (transformers CLIPEncoderLayer, reached from x3:1714, 1733-1735).  fp32 compute (exact erff,
                             fp32 output) or split operands (the bf16x3 mode; output fp32 with exact erff, or out_dtype V2A_BF16_SPLIT: row m =
                             [hi of the N outputs | lo of them], ldo >= 2N, erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, the fc2 operand
                             written directly).  Plain bf16 compute refuses it. */
  V2A_EPI_SWIGLU = 7,     /* ABI 8, additive: the GEGLU row packing [16 value | 16 gate] per 16 outputs with silu on the gate,
                             out[m][j] = (acc_v + b_v) * silu(acc_g + b_g), silu(x) = x / (1 + exp(-x)); out has N/2 cols -- Dinov2SwiGLUFFN of the
                             DINOv2 image encoder (`video_encoder="dinov2"`, x3:1432-1433, 1714, 1742-1744): gate = rows [0, Hf) of weights_in (x1),
                             value = rows [Hf, 2Hf) (x2).  fp32 compute (exact expf and division, fp32 output) or split operands (the bf16x3 mode;
                             output fp32 with exact expf, or out_dtype V2A_BF16_SPLIT: row m = [hi of the N/2 outputs | lo of them], ldo >= N, silu
                             on v_exp_f32, the weights_out operand written directly).  Plain bf16 compute refuses it. */
  V2A_EPI_CFG_EULER = 8,  /* Additive to ABI 9; v2a_gemm_cfg_euler only (v2a_gemm rejects it): the STORE epilogue on a tile that holds 32 rows of the
                             conditional half and the same 32 rows of the null half of the M rows, followed by the CFG + Euler update of y and the
                             operand planes of the new y -- see v2a_gemm_cfg_euler below */
  V2A_EPI_QUICK_GELU = 9  /* Additive to ABI 9: out = v sigmoid(1.702 v) = v / (1 + exp(-1.702 v)), v = acc + bias (transformers QuickGELUActivation)
                             -- CLIPMLP.fc1 + activation_fn of the ViT-L/14-336 CLIP image encoder (`video_encoder="clip_vit2"`, x3:1426-1428,
                             1714, 1736-1738).  Accepted and refused exactly where V2A_EPI_GELU is, with the same tiles: fp32 compute (v_exp_f32 of
                             -|1.702 v| and a Newton-refined reciprocal of 1 + e, fp32 output) or split operands (output fp32 likewise, or out_dtype V2A_BF16_SPLIT: row m = [hi of the
                             N outputs | lo of them], ldo >= 2N, on v_exp_f32 / v_rcp_f32, rounded to the planes once).  Evaluated in fp32 from the
                             fp32 accumulator and finite for every finite v (v << 0 gives -0).  Plain bf16 compute refuses it. */
};

typedef struct v2a_gemm_args {
  const void* a[3];      /* segment base pointers                                       */
  int64_t lda[3];        /* row stride of each segment, in elements                     */
  int32_t ka[3];         /* K extent of each segment; each a multiple of 64 (bf16) / 16 (f32) */
  int32_t nseg;          /* 1..3                                                        */
  int32_t a_dtype;       /* V2A_F32 or V2A_BF16; f32 A with bf16 compute is converted on load */
  const void* w;         /* [N][K] row-major, compute dtype, K = sum ka                 */
  int64_t ldw;
  const float* bias;     /* [N] or NULL                                                 */
  int32_t M, N;
  int32_t compute_dtype; /* V2A_F32 | V2A_BF16                                          */
  int32_t epilogue;      /* V2A_EPI_*                                                   */
  void* out;             /* [M][N] (GEGLU: [M][N/2])                                    */
  int64_t ldo;
  int32_t out_dtype;     /* V2A_F32 | V2A_BF16 (RESID/GATE_RESID/SIGMOID: f32 only; GEGLU: bf16, or f32 with bf16 compute) */
  void* out_bf16;        /* optional bf16 shadow copy of an f32 output (operand of a later GEMM), or NULL */
  int64_t ld_out_bf16;
  const float* resid;    /* [M][ldr] f32; may alias out                                 */
  int64_t ldr;
  const float* gate;     /* step vector of length N (GATE_RESID)                        */
  const int32_t* step;
  int64_t gate_step_stride, gate_batch_stride;
  int32_t rows_per_batch;
  /* optional fused rotary embedding (bf16 STORE epilogue only): columns [0, rope_cols) are 64-wide heads whose
   * interleaved pairs (2i, 2i+1) are rotated by cs_table[rope_pos_offset + m % rows_per_batch][i] = (cos, sin);
   * replaces a separate v2a_rope_inplace(layout 0) pass over the fused [q|k|v|gate] output */
  const float* rope_table;
  int32_t rope_cols, rope_pos_offset;
  int32_t relu;          /* non-zero: out = max(out, 0) after the epilogue (not GEGLU): the conv + folded-BatchNorm + ReLU
                          * and conv + BN + residual + ReLU blocks of the Video2Roll encoder, Video2RollNet.py:70-88 */
  /* implicit-GEMM convolution (bf16 compute, one bf16 A segment, STORE / RESID epilogue): with a_row_offset the A row m
   * starts at a[0] + a_row_offset[m] and K tile kt (64 elements) adds a_ktile_offset[kt] -- for an NHWC map stored with a
   * zero border, a_row_offset = top-left tap of output pixel m and a_ktile_offset[kt] = (ky*Wp + kx)*C + c0, so the patch
   * matrix of nn.Conv2d (Video2RollNet.py:9-12) is never materialised; lda is ignored.  With out_row_offset, row m of out,
   * resid and out_bf16 starts at base + out_row_offset[m] (the interior of the next layer's bordered map) instead of m * ld.
   * All offsets in elements, multiples of 8; NULL = dense rows.
   * Split operands (a_dtype V2A_BF16_SPLIT, the bf16x3 mode) take the tables too, on the 64-wide K stage shapes only (tile_hint 0 or
   * 1..4): the hi plane of row m / K tile kt starts at a[0] + a_row_offset[m] + a_ktile_offset[kt], its lo plane a_lo_offset[0]
   * elements further (required, > 0, a multiple of 8; lda is not checked).  The CALLER guarantees that every hi-plane read --
   * a_row_offset[m] + a_ktile_offset[kt] + 64 -- stays within a_lo_offset[0] (the zero-bordered NHWC hi map), the library cannot
   * see the device tables.  A split shadow (out_bf16_split) with out_row_offset puts the lo plane of row m at out_bf16 +
   * out_row_offset[m] + out_bf16_lo_offset (required, > 0: the hi map's size). */
  const int32_t* a_row_offset;
  const int32_t* a_ktile_offset;
  const int32_t* out_row_offset;
  /* 0 = the library picks the tile shape for the fastest stand-alone launch.  k + 1 = use LDS-DMA tile configuration k of
   * v2a_tuning.gemm_force_tile for THIS call (bf16 x bf16 only).  The sampler passes 1 (128x256 tiles, one workgroup per CU) for
   * the text / frames streams: their GEMMs run beside the audio stream's, and few fat workgroups that own whole CUs disturb
   * the critical path less than many small ones spread over every CU (+3.5 % end to end, measured).
   * Plain bf16 x bf16 operands, 0 = by shape or 1..16 (any other value is rejected).  The LDS-DMA ring shapes, one row per tile_hint
   * (V2A_RING_TILES in csrc/gemm.hip holds the same rows under k = tile_hint - 1):
   *   plain hint | tile    | waves (rows x columns) | ring depth | K stage | wave tile
   *            1 | 128x256 | 2x4 | 3 | 64 | 64x64
   *            2 | 128x128 | 2x2 | 3 | 64 | 64x64
   *            3 | 128x64  | 2x2 | 3 | 64 | 64x32
   *            4 | 64x64   | 2x2 | 3 | 64 | 32x32
   *            5 | 64x64   | 2x2 | 3 | 64 | 32x32      (another name of 4)
   *            6 | 256x256 | 2x4 | 2 | 64 | 128x64
   *            8 | 64x128  | 2x2 | 6 | 64 | 32x64
   *            9 | 64x64   | 2x2 | 6 | 64 | 32x32
   *           10 | 64x64   | 2x2 | 4 | 64 | 32x32
   *           11 | 64x64   | 2x2 | 5 | 64 | 32x32
   *           12 | 128x128 | 2x2 | 4 | 64 | 64x64
   *           13 | 128x128 | 2x4 | 3 | 64 | 64x32
   *           14 | 64x64   | 2x4 | 3 | 64 | 32x16
   *           15 | 128x64  | 4x2 | 3 | 64 | 32x32
   *           16 | 64x128  | 2x4 | 3 | 64 | 32x32
   *    7 = the 256x256 phase-interleaved (8-phase) kernel: dense rows and 16-byte aligned epilogue operands only
   * 14 has no GEGLU form (value / gate groups of 16 columns need wave tiles of 32) and is refused together with norm_ssq (V2A_ERR_ARG: the
   * partial sums per 32 columns need wave tiles of at least 32 columns); norm_gamma alone, the shadow without sums, runs on it.  The K order
   * of an output element is the same on every ring shape: STORE / RESID / GATE_RESID results of hints 1..6 and 8..16 are equal bit for bit.
   * Split operands (a_dtype V2A_BF16_SPLIT) have tile shapes of their own, 0 = by shape or 1..7 (any other value is rejected).  The LDS-DMA
   * ring shapes (V2A_SPLIT_RING_TILES in csrc/gemm.hip); a stage holds K stage logical k of the four planes:
   *   split hint | tile    | waves (rows x columns) | ring depth | K stage | wave tile
   *            1 | 64x64   | 2x2 | 3 | 64 | 32x32
   *            2 | 128x64  | 2x2 | 3 | 64 | 64x32
   *            3 | 128x128 | 2x4 | 2 | 64 | 64x32
   *            4 | 64x128  | 2x4 | 3 | 64 | 32x32
   *            6 | 128x256 | 2x4 | 3 | 32 | 64x64
   *            7 | 128x128 | 2x4 | 3 | 32 | 64x32
   *   5 = the 256x256 phase-interleaved (8-phase) kernel: a stage = 32 logical k, staged as rows [32 k hi | 32 k lo] of both operands,
   *       three products (A_lo W_hi, A_hi W_lo, A_hi W_hi) from one set of fragments; dense rows only; every ka a multiple of 64.
   * With a_row_offset / out_row_offset only 0 and 1..4 are admitted (a_ktile_offset is laid out for 64-wide K tiles).  Every shape adds the
   * three products of a 32-wide k step -- A_lo W_hi, A_hi W_lo, A_hi W_hi, in that order -- to one accumulator chain, k steps in ascending order,
   * whether a stage holds 64 k (two steps) or 32: the sum order of an output element does not depend on the shape.  STORE (with or without
   * fused RoPE) / RESID / GATE_RESID results, their shadows and norm_ssq are equal bit for bit on the ring shapes 1..4, 6, 7, and the fp32
   * results of shape 5 (the 8-phase kernel forms the same products in the same order per 32 logical k) equal them too
   * (tests/test_gemm_split_ring_gpu.py asserts both).  GEGLU / SWIGLU / GELU / QUICK_GELU results agree to rounding only: their store forms may evaluate the activation differently. */
  int32_t tile_hint;
  /* RMSNorm folded into its neighbours (bf16 x bf16, 16-byte aligned epilogue operands, N % 32 == 0):
   * PRODUCER (RESID / GATE_RESID with out_bf16): with norm_gamma the shadow is out_bf16[m][n] = bf16(out[m][n] * gamma[n]),
   * gamma = norm_gamma + step[0] * norm_step_stride + (m / rows_per_batch) * norm_batch_stride (+ norm_switch_offset for rows
   * m >= norm_switch_row: the rows a later GEMM of the block does not touch carry the NEXT norm's gamma), and with norm_ssq
   * the sums of squares of out[m][32 j .. 32 j + 31] go to norm_ssq[m * ld_norm_ssq + j].
   * CONSUMER (any epilogue): with row_ssq the accumulator row m is multiplied by
   * sqrt(row_norm_dim) / max(sqrt(sum_{j < row_ssq_parts} row_ssq[m * ld_row_ssq + j]), 1e-12) before the bias -- F.normalize
   * of xt RMSNorm / AdaptiveRMSNorm commutes with the product, so norm -> Linear costs no pass of its own.  row_ssq_parts <= 40;
   * rows of row_ssq are read as whole float4: ld_row_ssq a multiple of 4 and the columns past row_ssq_parts zero. */
  const float* norm_gamma;
  int64_t norm_step_stride, norm_batch_stride;
  int32_t norm_switch_row, norm_switch_offset;
  float* norm_ssq;
  int64_t ld_norm_ssq;
  const float* row_ssq;
  int64_t ld_row_ssq;
  int32_t row_ssq_parts, row_norm_dim;
  /* non-zero: the out_bf16 shadow is written in the V2A_BF16_SPLIT layout, row m = [hi_0 .. hi_{N-1} | lo_0 .. lo_{N-1}] of the
   * (gamma-scaled, when norm_gamma is given) fp32 result, ld_out_bf16 >= 2 * N: the operand of a later split-bf16 GEMM without a
   * v2a_split_bf16 pass.  Likewise out_dtype = V2A_BF16_SPLIT (GEGLU, SWIGLU, GELU and QUICK_GELU epilogues only): out row m = [hi | lo] planes of the N/2
   * hidden values, ldo >= N (GELU / QUICK_GELU: of the N values, ldo >= 2N).  A split shadow is written by the LDS-staged epilogue of the ring and 8-phase
   * kernels only: out_bf16_split is refused (V2A_ERR_ARG) with compute_dtype V2A_F32, with fp32 A on bf16 compute, with the SIGMOID epilogue and
   * with epilogue operands that are not 16-byte aligned -- those launches run a scalar epilogue that would write the hi plane alone. */
  int32_t out_bf16_split;
  /* ABI 8, split operands / split shadow only.  a_lo_offset[s]: elements from the hi plane of a row of segment s to its lo plane; 0 = ka[s], the
   * layout [hi k | lo k].  out_bf16_lo_offset: the same for the shadow row; 0 = N.  They let ONE buffer of rows [x_hi | s_hi | x_lo | s_lo] serve
   * as a K = 2d segment (x and the U-Net skip concatenated, lo plane 2d further) AND, half by half, as a K = d segment or as the split shadow
   * two different GEMM epilogues write (lo plane 2d further, not d): the fused cross-condition + skip projection of the bf16x3 mode.
   * Multiples of 8 (a_lo_offset) / 4 (out_bf16_lo_offset); lda[s] >= a_lo_offset[s] + ka[s], ld_out_bf16 >= out_bf16_lo_offset + N. */
  int64_t a_lo_offset[3];
  int64_t out_bf16_lo_offset;
} v2a_gemm_args;

int v2a_gemm(const v2a_gemm_args* args, v2a_stream_t stream);
/* sizeof(v2a_gemm_args) as the library was built: a binding checks its mirror of the struct against this */
int v2a_gemm_args_size(void);

/* ABI 9: what v2a_gemm would launch for these arguments under the current v2a_tuning.  v2a_gemm_choose runs everything v2a_gemm runs up
 * to, but not including, its first HIP call -- the argument checks, the tile selection, the dispatch to the instantiation -- and that
 * instantiation writes *choice from its own constants.  Return codes and v2a_last_error texts are those of v2a_gemm for the same arguments
 * (a refusal leaves *choice zeroed).  No pointer of args is dereferenced and no GPU is needed. */
enum { V2A_GEMM_REGISTER_STAGED = 0, V2A_GEMM_RING = 1, V2A_GEMM_8PHASE = 2 };
typedef struct v2a_gemm_choice {
  int32_t family;            /* V2A_GEMM_*: the register-staged kernel (exact fp32, fp32 A, SIGMOID), the LDS-DMA ring, the 8-phase kernel */
  int32_t split;             /* non-zero: the instantiation for split (hi | lo plane) operands */
  int32_t bm, bn, bk;        /* workgroup tile and the logical K of one stage */
  int32_t waves_m, waves_n;  /* waves of a workgroup, rows x columns */
  int32_t stages;            /* LDS buffers a K stage rotates through */
  int32_t tiles;             /* workgroups of the launch */
  int32_t xcd_gm, xcd_gn;    /* XCD grid over the tile space (used by the ring and 8-phase kernels) */
  int32_t vec_epi;           /* non-zero: the LDS-staged epilogue with 16-byte row pieces */
} v2a_gemm_choice;
int v2a_gemm_choose(const v2a_gemm_args* args, v2a_gemm_choice* choice);

/* Tile-selection overrides of v2a_gemm for A/B measurements (bench.py, scripts/).  Library defaults: force -1, rotation 0,
 * 8-phase kernel on (staggered) from 400 tiles.
 * Process-wide; call it between launches, not concurrently with them.  NULL restores the defaults. */
typedef struct v2a_tuning {
  int32_t gemm_force_tile;        /* -1 = by shape; k = 0..8 without 4: the shape of plain tile_hint k + 1 (v2a_gemm_args) for every bf16 x bf16 GEMM (0 128x256, 1 128x128, 2 128x64, 3 64x64, 5 256x256), 6 = the 256x256 8-phase kernel, 7 / 8 = 64x128 / 64x64 with a 6-deep ring */
  int32_t gemm_k_rotation;        /* ignored since ABI 5 (was: M bands that share a W panel start their K walk at different K tiles; +0.7 %, and it made
                                   * the fp32 summation order depend on M): the K loop now walks running pointers */
  int32_t gemm_8phase;            /* 256x256 phase-interleaved kernel for wide outputs (N >= 2048): 0 off, 1 on (staggered wave rows), 2 on (lock-step) */
  int32_t gemm_8phase_min_tiles;  /* ... when the problem yields at least this many 256x256 tiles (0 = 400) */
  int32_t dwconv_rows_per_wave;   /* v2a_dwconv_silu_residual: output positions per wave pass of the small-launch kernel, 4 or 6 (0 = default 4);
                                   * -1 = never use the streaming kernel that chip-filling launches take (A/B) */
  int32_t gemm_xcd_order_1x8;     /* 1: every XCD walks whole column strips of the tile space (the round-1 order) instead of the
                                   * per-shape gm x gn rectangle grid that minimises operand re-fetch across the 8 L2s */
  int32_t attn_one_group_from;    /* v2a_attention (bf16): launches with at least this many workgroups run one wave group per workgroup
                                   * instead of two that split the key tiles (0 = default 1536) */
  int32_t reserved[1];            /* A/B bits: 128 = GEGLU epilogue with 8-byte (four-column) stores, 256 = split attention with 64 queries per workgroup, 512 = 8-phase kernel multiplies padding row bands too; others: probe builds only */
} v2a_tuning;
int v2a_set_tuning(const v2a_tuning* tuning);

/* ---------------------------------------------------------------------------------------
 * RMSNorm / AdaptiveRMSNorm:  y = x / max(|x|_2, 1e-12) * sqrt(d) * gamma
 * gamma is a step vector: RMSNorm passes g (strides 0); AdaptiveRMSNorm passes the
 * precomputed (to_gamma(c) + 1) table.  Output in the compute dtype (GEMM operand); y_dtype V2A_BF16_SPLIT writes the
 * hi / lo planes of the split layout (ldy >= 2*d).
 * Replaces: xt RMSNorm (x3:880,883,913,916,935), xt AdaptiveRMSNorm (x3:807,812,816).
 * ------------------------------------------------------------------------------------- */
int v2a_rmsnorm(const float* x, int64_t ldx, void* y, int64_t ldy, int32_t y_dtype,
                int64_t rows, int32_t d,
                const float* gamma, const int32_t* step, int64_t gamma_step_stride,
                int64_t gamma_batch_stride, int32_t rows_per_batch, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Position-generating depthwise conv, fused with mask, SiLU and the caller's residual:
 *   out[b,n,:] = x[b,n,:] + m[b,n] * silu(bias + sum_j wt[j,:] * (m*x)[b, n+j-k/2, :])
 * m[b,n] = n < len[b] (len NULL = all valid).  wt is the Conv1d weight transposed to
 * [k][d].  out may alias x only if out == x is NOT used (the kernel reads a halo): pass a
 * different buffer.
 * Replaces: DepthwiseConv x3:495-528 + the `+ x` at x3:1082,1097,1122.
 * ------------------------------------------------------------------------------------- */
int v2a_dwconv_silu_residual(const float* x, float* out, const float* wt, const float* bias,
                             int32_t B, int32_t N, int32_t d, int32_t ksize,
                             const int32_t* len, v2a_stream_t stream);
/* The same with the RMSNorm that follows it folded in (x3:1083,1098,1126): additionally
 *   out_bf16[b,n,c] = bf16(out[b,n,c] * gamma[c]),  gamma = norm_gamma + step[0] * step_stride + b * batch_stride
 *   norm_ssq[(b*N + n) * ld_ssq + j] = sum of out[b,n,32j..32j+31]^2
 * for the GEMM that consumes out_bf16 with row_ssq (v2a_gemm_args).  d % 32 == 0. */
typedef struct v2a_dwconv_norm {
  void* out_bf16;
  int64_t ld_out_bf16;
  const float* norm_gamma;
  const int32_t* step;
  int64_t norm_step_stride, norm_batch_stride;
  float* norm_ssq;
  int64_t ld_norm_ssq;
  int32_t split;          /* non-zero: out_bf16 rows in the V2A_BF16_SPLIT layout [hi d | lo d] (ld_out_bf16 >= 2 * d): bf16x3 mode */
  int32_t reserved;
} v2a_dwconv_norm;
int v2a_dwconv_silu_residual_norm(const float* x, float* out, const float* wt, const float* bias,
                                  int32_t B, int32_t N, int32_t d, int32_t ksize,
                                  const int32_t* len, const v2a_dwconv_norm* norm, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Rotary embedding applied in place to `nheads` consecutive 64-wide heads of every row
 * (the q and k column blocks of the fused QKV GEMM output).
 * position of row r = pos_offset + (r % rows_per_batch); table cs[pos][32][2] = (cos,sin)
 * of pos * 10000^(-2i/64).  layout 0 = interleaved pairs (2i,2i+1), 1 = half split (i,i+32).
 * Replaces: xt RotaryEmbedding.forward_from_seq_len + apply_rotary_pos_emb
 * (x3:779-781,983,988,994 and the rotary_pos_emb argument at x3:1084,1099,1126,1131).
 * ------------------------------------------------------------------------------------- */
int v2a_rope_inplace(void* qk, int32_t dtype, int64_t rows, int64_t row_stride, int32_t nheads,
                     int32_t rows_per_batch, int32_t pos_offset, const float* cs_table,
                     int32_t layout, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Soft-clamped, key-masked, head-gated attention core (dim_head = 64):
 *   s = clamp * tanh(scale * q.k / clamp);  p = softmax_j(s | j < kv_len[b]);
 *   o[b,i,h,:] = sigmoid(gate[b,i,h]) * sum_j p_j v[b,j,h,:];  rows i >= q_len[b] -> 0
 * q/k/v/gate/out are addressed as base + b*batch_stride + token*row_stride + h*64 (+c)
 * (gate: + h), so they can live inside the fused [q|k|v|gate] GEMM output.
 * Replaces: xt Attention forward minus its Linears (attend + to_v_head_gate epilogue +
 * out.masked_fill), sites x3:808,813,881,914,1084,1099,1126,1131.
 * ------------------------------------------------------------------------------------- */
typedef struct v2a_attn_args {
  const void *q, *k, *v, *gate;
  void* out;
  int64_t q_row_stride, k_row_stride, v_row_stride, gate_row_stride, out_row_stride;
  int64_t q_batch_stride, k_batch_stride, v_batch_stride, gate_batch_stride, out_batch_stride;
  int32_t B, H, Nq, Nk;
  const int32_t* kv_len; /* [B] or NULL (= Nk) */
  const int32_t* q_len;  /* [B] or NULL (= Nq) */
  float scale, softclamp;
  int32_t dtype;         /* V2A_F32 / V2A_BF16: dtype of q,k,v,gate,out and of the arithmetic; V2A_BF16_SPLIT: fp32 tensors,
                          * products as three bf16 MFMA passes over hi | lo operand planes (the bf16x3 mode) */
  int32_t out_split;     /* dtype V2A_BF16_SPLIT only, non-zero: out is a bf16 buffer in the V2A_BF16_SPLIT layout -- row =
                          * [hi of the H*64 outputs | lo of them], out_row_stride / out_batch_stride in bf16 elements -- i.e. the
                          * A operand of the out-projection's split GEMM, written directly */
} v2a_attn_args;

int v2a_attention(const v2a_attn_args* args, v2a_stream_t stream);
/* ---------------------------------------------------------------------------------------
 * Cross-attention of the audio stream in ONE launch (ABI 6): the q-projection GEMM of v2a_gemm -- STORE epilogue with the optional
 * row_ssq consumer scale, bias and fused RoPE -- whose 64-token x one-head output tile never leaves the workgroup: it is the Q
 * operand of QK^T over the clip's Nk <= 64 context keys, soft clamp, softmax, PV, per-head sigmoid gate, and only the attention
 * output rows are written.  Equal bit for bit to v2a_gemm(gemm) into a [q | gate] buffer followed by v2a_attention(attn) on it.
 *   gemm: nseg = 1, bf16 A and W, ka[0] a multiple of 512; W rows [0, H*64) = to_q, rows [H*64, H*64 + H) = the per-head gate
 *         rows (N >= H*65), bias likewise; M = attn->B * attn->Nq rows, rows_per_batch = attn->Nq; out / ldo / out_dtype ignored.
 *   attn: dtype V2A_BF16; k, v, out and their strides, B, H, Nq, Nk, kv_len, q_len, scale, softclamp as for v2a_attention;
 *         q, gate and their strides ignored.
 * Replaces: xt Attention.forward with a context -- to_q, rotary_emb on q, attend, to_v_gates -- at call site x3:1126 (audio
 * stream of a layer with text context), for launches small enough to be latency bound (the sampler: <= 2 clips per GPU).
 * ------------------------------------------------------------------------------------- */
int v2a_qproj_xattn(const v2a_gemm_args* gemm, const v2a_attn_args* attn, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Cross-attention with the context absorbed into the weights (bf16x3 mode; additive entry points, ABI 9).  Without rotary in
 * cross-attention and with bias-free to_q / to_k / to_v / to_out, for clip b, layer l, head h and key slot j
 *   logits[n,h,j] = x[n,:] . Wqk[b,l][(h,j),:]      Wqk[(h,j),c] = sum_d K[b,j,l,h,d] * to_q[l][h*64+d, c]
 *   out[n,o] = sum_{h,j} P[n,h,j] * sigmoid(gate[n,h]) * Wvo[b,l][o,(h,j)]      Wvo[o,(h,j)] = sum_d to_out[l][o, h*64+d] * V[b,j,l,h,d]
 * and K, V of the context are constants of a sample() call.  KP = key slots per head: 16 (nc <= 16) or 32 (nc <= 32).
 *
 * v2a_xattn_absorb_prepare (once per sample(), two launches for all clips, layers and heads): from the fp32 context K / V rows
 * (row b*nc + j; K of layer l at columns k_col + l*H*64, V at v_col + l*H*64) and fp32 masters wq [L][H*64 + H][D] (to_q rows, then
 * the to_v_head_gate rows) and wo [L][D][H*64] writes, as V2A_BF16_SPLIT rows [hi | lo] of the fp32 results (fma chains over the 64
 * head dimensions in order),
 *   wqk [B][L][H*KP + H][2 D]   row h*KP + j as above, zero for nc <= j < KP; the last H rows are the planes of the gate rows
 *   wvo [B][L][D][2 H*KP]       columns h*KP + j as above, zero for nc <= j < KP
 * ------------------------------------------------------------------------------------- */
typedef struct v2a_xattn_prepare_args {
  const float* ctx_kv;
  int64_t ctx_ld;        /* floats per context row */
  int32_t k_col, v_col;
  const float* wq;
  const float* wo;
  void* wqk;
  void* wvo;             /* 8-byte aligned */
  int32_t B, L, H, D, nc, KP;
} v2a_xattn_prepare_args;
int v2a_xattn_absorb_prepare(const v2a_xattn_prepare_args* args, v2a_stream_t stream);

/* v2a_xattn_absorbed (per evaluation): rows of `a` (V2A_BF16_SPLIT, [hi K | lo K], K a multiple of 512, <= 2048) times Wqk of the
 * row's clip (row / rows_per_batch; clips w_batch_stride elements apart, rows ldw >= 2 K apart) as the split GEMM computes it (per
 * 32 k: A_lo W_hi + A_hi W_lo + A_hi W_hi), then per row and head: x 1/rms of the row when row_ssq is given (the folded-norm
 * consumer of v2a_gemm_args), soft clamp clamp*tanh(scale*s/clamp) (softclamp > 0), key slots >= min(kv_len[b], KP) masked, softmax
 * over the KP slots, times sigmoid(gate logit (x 1/rms) + gate_bias[h]); rows at or beyond q_len[b] in their clip and rows of a clip
 * with kv_len[b] = 0 are exactly zero.  out: (M, [hi H*KP | lo H*KP]) bf16 rows ldo apart, the A operand of
 * v2a_gemm(V2A_EPI_GATE_RESID) with W = Wvo of the clip, K = H*KP.  H*KP must be a multiple of 64; kv_len is required.
 * Replaces, together with that GEMM: v2a_qproj_xattn (or v2a_gemm + v2a_attention) and the out-projection at call site x3:1126. */
typedef struct v2a_xattn_absorbed_args {
  const void* a;
  int64_t lda;
  int32_t K, M;
  const void* wqk;
  int64_t ldw, w_batch_stride;
  const float* gate_bias;   /* [H] or NULL */
  void* out;
  int64_t ldo;
  int32_t rows_per_batch, B, H, KP;
  const int32_t* kv_len;    /* [B] */
  const int32_t* q_len;     /* [B] or NULL (= rows_per_batch) */
  float scale, softclamp;
  const float* row_ssq;     /* as v2a_gemm_args: row_ssq, ld_row_ssq, row_ssq_parts, row_norm_dim */
  int64_t ld_row_ssq;
  int32_t row_ssq_parts, row_norm_dim;
} v2a_xattn_absorbed_args;
int v2a_xattn_absorbed(const v2a_xattn_absorbed_args* args, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Small fp32 linear with output row scatter (1 <= K <= 2048, VALU; V2A_ERR_ARG beyond):
 *   out[(m / T)*out_batch_stride + (row_off + m % T)*d + n] =
 *        bias[n] + add[(m % T)*d + n] + sum_k a[m*K + k] * wt[k*d + n]
 * and, when `dup_batch_offset` > 0, the same value again at batch (m/T + dup_batch_offset)
 * (cond and null CFG halves share proj_in(x) + abs_pos_emb).
 * Two launch forms, both with the block's A rows in dynamic LDS at 8 * K bytes per row: 8 rows per block when that gives at least
 * 512 blocks (ceil(rows / 8) * (M / T), rows = T plus the register rows), else 2 rows per block.  The 2-row form stays within 32 KB at
 * every K; the 8-row form takes 64 KB at K = 1024 and, for K in (1024, 2048], up to 128 KB, for which it raises the kernel's dynamic
 * LDS limit once per device (V2A_ERR_LAUNCH if the device refuses).  The two forms are not required to agree in the last bits of a sum.
 * Replaces: proj_in x3:2027 + abs_pos_emb x3:957-960 + register pack x3:975-976;
 * proj_frames x3:2069.
 * ------------------------------------------------------------------------------------- */
int v2a_linear_small(const float* a, int64_t M, int32_t K, const float* wt, const float* bias,
                     const float* add, int32_t T, float* out, int64_t out_batch_stride,
                     int32_t row_off, int32_t d, int32_t dup_batch_offset,
                     const float* regs /* NULL, or [row_off][d]: also writes rows [0,row_off) = regs */,
                     void* out_bf16 /* NULL, or bf16 shadow with out's geometry */, v2a_stream_t stream);

/* out[b, r, :] = regs[r, :] for r < R, b < B  (register tokens, x3:975-997) */
int v2a_fill_registers(float* out, int64_t out_batch_stride, const float* regs, int32_t B,
                       int32_t R, int32_t d, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Time conditioning for every grid point at once:
 *   out[s,:] = silu(bias + Wt^T [t_s, sin(2 pi t_s w), cos(2 pi t_s w)])
 * wt = Linear(d+1, d).weight transposed to [d+1][d].
 * Replaces: RandomFourierEmbed x3:555-564 + time_cond_mlp x3:793-797,966-971.
 * ------------------------------------------------------------------------------------- */
int v2a_time_cond(const float* t, int32_t S, const float* fourier_w, const float* wt,
                  const float* bias, float* out, int32_t d, v2a_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CFG combine + explicit Euler update, in place on y (B, T, C):
 *   f = pc + s*(pc - pn);  y += dt[step] * f
 * pc = pred[b, row_off + i, :], pn = pred[B + b, row_off + i, :]  (pred is (2B, Np, C)).
 * With apg != NULL (remove_parallel_component): apg[b] = {sum (pc-pn)*pc, sum pc*pc} in
 * fp64 from v2a_apg_reduce and   upd = orth + keep*par.
 * Replaces: cfg_transformer_with_pred_head x3:2106-2113, project x3:162-173,
 * torchdiffeq Euler step (x3:2255).
 * ------------------------------------------------------------------------------------- */
int v2a_apg_reduce(const float* pred, double* apg, int32_t B, int32_t T, int32_t C,
                   int64_t pred_batch_stride, int32_t row_off,
                   const int32_t* valid_rows /* ABI 7: device int or NULL (= T): only rows [0, valid_rows[0]) of every clip enter the sums --
                                                the frames of the call, when the plan's T is padded to a shape bucket */,
                   v2a_stream_t stream);
int v2a_cfg_euler(float* y, const float* pred, int32_t B, int32_t T, int32_t C,
                  int64_t pred_batch_stride, int32_t row_off, float cfg_strength,
                  const float* dt, const int32_t* step, const double* apg,
                  float keep_parallel_frac, v2a_stream_t stream);
/* Additive to ABI 9: v2a_cfg_euler that also stores the operand planes of the y it has just updated (V2A_BF16_SPLIT, the rounding of
 * v2a_split_bf16, 8-byte vector stores): element (b, i, c) goes to row (k * B + b) * rows_per_seq + row_off + i of `planes` for every
 * copy k < copies, hi plane at column c, lo plane at column lo_offset + c; rows outside [row_off, row_off + T) of a sequence are not
 * touched.  The DiT engine's folded layer-0 GEMMs read these rows as their K = C operand: row_off = registers, rows_per_seq = registers +
 * frames, copies = 2 (the conditional and the null half of the CFG batch both hold y).  y is updated exactly as by v2a_cfg_euler; with
 * planes == NULL (or a NULL struct) the call IS v2a_cfg_euler. */
typedef struct v2a_y_planes {
  void* planes;          /* bf16 rows, 8-byte aligned */
  int64_t ld;            /* row pitch in elements, >= lo_offset + C, % 4 == 0 */
  int64_t lo_offset;     /* elements from the hi plane of a row to its lo plane, >= C, % 4 == 0 */
  int32_t row_off;       /* first row of y inside every sequence */
  int32_t rows_per_seq;  /* >= row_off + T */
  int32_t copies;        /* 1 or 2 stacked batches of B sequences */
  int32_t reserved;
} v2a_y_planes;
int v2a_cfg_euler_planes(float* y, const float* pred, int32_t B, int32_t T, int32_t C,
                         int64_t pred_batch_stride, int32_t row_off, float cfg_strength,
                         const float* dt, const int32_t* step, const double* apg,
                         float keep_parallel_frac, const v2a_y_planes* planes, v2a_stream_t stream);
/* y[r][0:d] = hi, y[r][d:2d] = lo of x[r][0:d] (V2A_BF16_SPLIT layout above), rows x d fp32 in, row strides in elements,
 * d % 4 == 0: the split operand copy of an fp32 buffer (residual streams, attention outputs, GEGLU hidden) for the
 * three-segment bf16 GEMMs of the bf16x3 mode */
int v2a_split_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int32_t d, v2a_stream_t stream);
/* y[i] = bf16(x[i]), n % 4 == 0: bf16 operand copy of an fp32 stream that no GEMM epilogue produced
 * (the embed output x3:2027 feeding the first cross-condition GEMM) */
int v2a_cast_bf16(const float* x, void* y, int64_t n, v2a_stream_t stream);
/* step[0] += 1 (own launch: every block of the step has read step[0] before it runs) */
int v2a_step_advance(int32_t* step, v2a_stream_t stream);
/* Additive to ABI 9: the step seam of the sampler in ONE launch -- the to_pred GEMM, v2a_cfg_euler_planes (without APG) and v2a_step_advance.
 * `g` describes the to_pred GEMM exactly as for v2a_gemm: split operands (a_dtype V2A_BF16_SPLIT, bf16 compute), V2A_EPI_STORE, fp32 out with
 * ldo >= N, optional bias and row_ssq (folded final norm); no shadow, rope, relu or offset tables.  M = 2 * B * rows_per_seq rows: the
 * conditional half, then the null half; N = C, a multiple of 64.  The kernel is the 64x64 split ring of v2a_gemm with another row map -- tile
 * row j of row band i is row 32 i + (j mod 32) of the conditional (j < 32) or the null (j >= 32) half -- and the epilogue V2A_EPI_CFG_EULER:
 *   out[m] = acc * (1 / rms of row m) + bias      for every row m < M (the bits of the v2a_gemm launch: the split ring adds every 32-wide k
 *                                                 step in one order whatever the tile), register rows included;
 *   y[b][t] += dt[step[0]] * (pc + cfg_strength * (pc - pn))    with pc / pn = out of rows b * rows_per_seq + row_off + t of the two halves, the
 *                                                 expression of v2a_cfg_euler; hi | lo planes of the new y[b][t] into those two rows of `planes`
 *                                                 as by v2a_cfg_euler_planes with copies = 2; rows outside [row_off, row_off + T) of a sequence
 *                                                 update nothing and their plane rows are not touched.
 * Step counter: every workgroup reads dt[step[0]] and then adds 1 to arrive[0]; the workgroup that finds all others there stores step[0] + 1 and
 * puts arrive[0] back to 0.  No workgroup waits for another.  arrive[0] must be 0 when the launch starts, and is 0 again when it has ended. */
typedef struct v2a_step_seam {
  float* y;              /* (B, T, C) fp32, 16-byte aligned, updated in place */
  const float* dt;       /* step sizes */
  int32_t* step;         /* device step counter (required) */
  uint32_t* arrive;      /* arrival counter of the launch */
  void* planes;          /* bf16 rows of both halves (M rows), 8-byte aligned */
  int64_t ld;            /* row pitch of planes in elements, >= lo_offset + C, % 4 == 0 */
  int64_t lo_offset;     /* elements from the hi plane of a row to its lo plane, >= C, % 4 == 0 */
  int32_t B, T;          /* clips, latent frames */
  int32_t row_off;       /* first row of y inside every sequence (registers) */
  int32_t rows_per_seq;  /* >= row_off + T */
  float cfg_strength;
  int32_t reserved;
} v2a_step_seam;
int v2a_gemm_cfg_euler(const v2a_gemm_args* g, const v2a_step_seam* s, v2a_stream_t stream);

/* =======================================================================================
 * N2: Video2Roll frame encoder -- `E2TTS.encode_frames` x3:1525-1553 running
 * `Video2RollNet.resnet18` (`v2r` = src/audeo/Video2RollNet.py:127-251).  Activations are NHWC fp32;
 * every convolution is v2a_im2col (patch matrix in the compute dtype) + v2a_gemm with the eval-mode BatchNorm
 * folded into the weights / bias and ReLU / residual in the epilogue.
 * ===================================================================================== */

/* Patch matrix of a 2-D convolution:  col[(n*Ho + yo)*Wo + xo][k],  zero outside the image and for k >= K.
 *   window_t == 0: x is NHWC fp32 (n < B), k = (ky*kw + kx)*C + c, C % 4 == 0
 *                  (replaces the unfold of nn.Conv2d at v2r:9-12,18-19,138,187-188)
 *   window_t  > 0: x is (B / window_t clips, window_t frames, H, W) single-channel fp32 and the C = 5 input channels of
 *                  window n = (clip, i) are frames clamp(i-2 .. i+2, 0, window_t-1) of that clip -- the 5-frame stack
 *                  built at x3:1531-1539 is never materialised; k = (c*kh + ky)*kw + kx (the conv1 weight's own order)
 * ldo = padded K (multiple of 64 for bf16, 16 for f32), out_dtype = V2A_F32 | V2A_BF16. */
int v2a_im2col(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride,
               int32_t pad, int32_t Ho, int32_t Wo, void* col, int64_t ldo, int32_t out_dtype, int32_t window_t,
               int32_t window_first, v2a_stream_t stream);

/* First-layer operand of the implicit GEMM (bf16): one clip's frames (T, H, W) fp32 -> column patches
 *   out[j][xo][y][e],  j < T + 4, xo < Wo, y < H + 2*pad, e < 16   (bf16; (T+4)*Wo*(H+2*pad)*16 elements)
 *   = frame clamp(j - 2, 0, T - 1) at row y - pad, column stride*xo - pad + e; zero outside the image and for e >= kw.
 * The 5-frame window i of x3:1531-1539 is frames j = i .. i+4 of this replicate-padded clip, and the kh x kw taps of output
 * pixel (yo, xo) in channel c are the kh consecutive 16-element rows from out[i + c][xo][stride*yo]: with
 *   a_row_offset[m]    = ((i*Wo + xo)*Hp + stride*yo) * 16
 *   a_ktile_offset[kt] = (kt / g) * Wo*Hp*16 + (kt % g) * 64,   g = ceil(kh / 4) K tiles per channel (weights zero-padded)
 * v2a_gemm computes conv1 (v2r:138, 11x11 / stride 2 / pad 4) without the patch matrix of v2a_im2col. */
int v2a_frames_pack(const float* frames, void* out, int32_t T, int32_t H, int32_t W, int32_t kw, int32_t stride, int32_t pad,
                    int32_t Wo, v2a_stream_t stream);
/* The same column patches in the V2A_BF16_SPLIT planes of the bf16x3 mode (conv1, v2r:138): out[i] = hi = bf16(v) for the
 * (T+4)*Wo*(H+2*pad)*16 elements i of v2a_frames_pack, and out[lo_offset + i] = lo = bf16(v - hi) -- the grey frames are fp32
 * intensities that one bf16 does not hold.  lo_offset >= (T+4)*Wo*(H+2*pad)*16, a multiple of 8; out holds lo_offset + that many.
 * v2a_gemm reads both planes through the same offset tables (a_dtype V2A_BF16_SPLIT, a_lo_offset[0] = lo_offset). */
int v2a_frames_pack_split(const float* frames, void* out, int64_t lo_offset, int32_t T, int32_t H, int32_t W, int32_t kw,
                          int32_t stride, int32_t pad, int32_t Wo, v2a_stream_t stream);

/* NHWC fp32 pooling: mode 0 = max (padding acts as -inf; nn.MaxPool2d(3, 2, 1) v2r:141), mode 1 = average over the full
 * k*k window (nn.AvgPool2d(2, 2) / (3, 1), pad 0, v2r:22-23).  C % 4 == 0.  The input / output maps may be stored with a
 * zero border of in_border / out_border pixels (the implicit-GEMM layout of v2a_gemm's offset tables): only interiors are
 * read / written.  out_bf16 (or NULL) receives a bf16 copy with out's geometry (operand of the next convolution). */
int v2a_pool2d(const float* x, float* out, void* out_bf16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
               int32_t stride, int32_t pad, int32_t mode, int32_t Ho, int32_t Wo, int32_t in_border, int32_t out_border,
               v2a_stream_t stream);
/* v2a_pool2d with its bf16 copy in the V2A_BF16_SPLIT planes of the bf16x3 mode, written by the pooling kernel itself: out_split
 * (required) has out's geometry twice -- hi = bf16(out) at the position of out, lo = bf16(out - hi) lo_offset elements further
 * (>= B*(Ho+2*out_border)*(Wo+2*out_border)*C, a multiple of 4).  Only interiors are written: the caller zeroes the borders once.
 * The maps that feed a convolution: the max pool after conv1 (v2r:141) and FTB2_1's average pool into FTB2_2 (v2r:22-23, 214). */
int v2a_pool2d_split(const float* x, float* out, void* out_split, int64_t lo_offset, int32_t B, int32_t H, int32_t W, int32_t C,
                     int32_t k, int32_t stride, int32_t pad, int32_t mode, int32_t Ho, int32_t Wo, int32_t in_border,
                     int32_t out_border, v2a_stream_t stream);

/* Fused top of the network (v2r:224-249 + the sigmoid of x3:1541), one workgroup per window:
 *   FRB4/3/2 channel gates (global average pool -> fc1 -> ReLU -> fc2 -> sigmoid, v2r:44-57), out1 = p2*p3, softmax over
 *   the P positions per channel, out2 = softmax*p4, conv2 (1x1) + p4, global average pool, fc, optional sigmoid.
 * The 1x1 conv and the pool commute, so only per-channel position sums are formed.  All tensors fp32; x2_, x3_, x4_ are
 * (B, P, 128) and x5 is (B, P, 64) NHWC maps; weights are TRANSPOSED ([in][out]) so lanes read consecutive outputs. */
typedef struct v2a_roll_head_args {
  const float *x2, *x3, *x4, *x5;
  int32_t B, P;
  const float *frb4_w1t, *frb4_b1, *frb4_w2t, *frb4_b2;   /* [192][128], [128], [128][128], [128] */
  const float *frb3_w1t, *frb3_b1, *frb3_w2t, *frb3_b2;   /* [256][128] ...                        */
  const float *frb2_w1t, *frb2_b1, *frb2_w2t, *frb2_b2;   /* [256][128] ...                        */
  const float *conv2_wt, *conv2_b;                        /* [128][128], [128]                     */
  const float *fc_wt, *fc_b;                              /* [128][notes], [notes]                 */
  int32_t notes;                                          /* <= 128 (51: NOTES, x3:1523)           */
  int32_t apply_sigmoid;                                  /* 1: probabilities (encode_frames), 0: logits (ResNet.forward) */
  float* out;                                             /* (B, notes)                            */
} v2a_roll_head_args;
int v2a_roll_head(const v2a_roll_head_args* args, v2a_stream_t stream);

/* roll (B, t, notes) -> out (B, l, notes): every frame row repeated `rep` (3) times, cropped / zero-padded to l rows
 * (x3:1544-1553) */
int v2a_roll_expand(const float* roll, float* out, int32_t B, int32_t t, int32_t notes, int32_t rep, int32_t l,
                    v2a_stream_t stream);

/* The same by a ratio rep / group, the 88-key configuration's 5 / 2 (x3_2 = e2_tts_crossatt3_2.py:1546-1554): every row repeated
 * `rep` times, the repeated rows cut to a whole number of groups and every `group` (1 or 2) consecutive ones averaged:
 *   out[b][r] = (1 / group) * sum_{g < group} roll[b][(r * group + g) / rep]   for r < t * rep / group,   0 for the rows up to l.
 * group = 2 forms (a + b) * 0.5f in fp32, which is what torch's `.mean(2)` of two rows gives bit for bit; group = 1 copies, so
 * (rep, 1) equals v2a_roll_expand.  Replaces the repeat / reshape / mean / crop / zero-pad expression of x3_2:1546-1554. */
int v2a_roll_expand_ratio(const float* roll, float* out, int32_t B, int32_t t, int32_t notes, int32_t rep, int32_t group, int32_t l,
                          v2a_stream_t stream);

/* =======================================================================================
 * N1: Encodec 24 kHz decoder, the vocoder behind `EncodecWrapper.decode` x3:434-437 (predict.py:277-278;
 * arithmetic: transformers EncodecDecoder, requirements.txt:20).  Activations are time-major [T][C] fp32, so every
 * causal Conv1d is a v2a_gemm over overlapping rows (lda = C, K = k*C) and every ConvTranspose1d(k = 2*stride) a v2a_gemm
 * with K = 2C, N = stride*Cout whose output IS the up-sampled [T*stride][Cout] signal.  Two kernels complete the stack:
 * ===================================================================================== */

/* out[(pad + t)][c] = act ? ELU(x[t][c]) : x[t][c] for t < T, preceded by `pad` rows: reflect != 0 -> row (pad - i) mirrors
 * row i (the causal reflect padding of EncodecConv1d: F.pad(x, (k-1, 0), "reflect")), else zeros (the x[q-1] operand of a
 * transposed convolution at q = 0).  out holds (T + pad) rows.  C % 4 == 0.  Replaces nn.ELU + the padding of every conv. */
int v2a_elu_pad(const float* x, float* out, int64_t T, int32_t C, int32_t pad, int32_t reflect, int32_t act,
                v2a_stream_t stream);

/* One nn.LSTM layer's recurrence over T steps (batch 1, hidden H = 512, zero initial state), gates in torch order (i,f,g,o):
 *   g_t = gates_x[t] + W_hh h_{t-1};  c_t = sig(f) c_{t-1} + sig(i) tanh(g);  h_t = sig(o) tanh(c_t)
 * gates_x[t] = W_ih x_t + b_ih + b_hh comes from a v2a_gemm.  h (T, H) receives every h_t; with y != NULL also
 * y[t] = h_t + resid[t] (the skip of EncodecLSTM).  Persistent kernel of H/8 workgroups with W_hh in registers; h_t travels
 * between workgroups as 64-bit {value, step tag} words (device-scope atomic store / polled load), one round trip per step.
 * workspace = 4*H + 2 int32, 8-byte aligned (zeroed by the call; workspace[4*H] != 0 afterwards means a workgroup timed
 * out waiting for its peers and the result is invalid). */
int v2a_lstm_layer(const float* gates_x, const float* w_hh, float* h, const float* resid, float* y, int32_t T, int32_t H,
                   int32_t* workspace, v2a_stream_t stream);

/* Both layers of EncodecLSTM (2-layer nn.LSTM + skip, batch 1, H = 512) in one persistent kernel: pipeline step s runs layer 0
 * at time s and layer 1 at time s - 1, both fed by values published in step s - 1, so the sequence costs T + 1 exchange round
 * trips instead of 2T and layer 1's input projection (w_ih1, bias1 = b_ih1 + b_hh1) is done in the kernel.
 *   y[t] = h1[t] + resid[t]   (resid may be NULL).   gates_x0[t] = W_ih0 x_t + b_ih0 + b_hh0 from a v2a_gemm.
 * workspace = 8*H + 2 int32, 8-byte aligned (zeroed by the call; workspace[8*H] != 0 afterwards = a workgroup timed out). */
int v2a_lstm2(const float* gates_x0, const float* w_hh0, const float* w_ih1, const float* bias1, const float* w_hh1,
              const float* resid, float* y, int32_t T, int32_t H, int32_t* workspace, v2a_stream_t stream);

/* =======================================================================================
 * Encodec 24 kHz encoder, `EncodecWrapper.forward` x3:428-432 (predict.py:222; arithmetic: transformers EncodecEncoder): the
 * decoder's mirror.  A strided Conv1d(k = 2r, stride r) on a time-major [T][C] buffer is ONE v2a_gemm whose A rows overlap with
 * lda = r*C, K = k*C, M = ceil(T / r), over a buffer padded by v2a_elu_pad_lr; the LSTM is v2a_lstm2.  ABI 8, additive.
 * ===================================================================================== */

/* v2a_elu_pad with a pad on both sides: out[pad_left + t][c] = act ? ELU(x[t][c]) : x[t][c] for t < T, preceded by pad_left
 * reflected rows (row pad_left - i mirrors row i) and followed by pad_right reflected rows (row pad_left + T - 1 + i mirrors row
 * T - 1 - i), as F.pad(x, (pad_left, pad_right), "reflect") does: EncodecConv1d pads k - stride samples in front and, where the
 * length is not a multiple of the stride, up to stride - 1 behind.  out holds T + pad_left + pad_right rows.  C % 4 == 0, both
 * pads < T (V2A_ERR_ARG otherwise). */
int v2a_elu_pad_lr(const float* x, float* out, int64_t T, int32_t C, int32_t pad_left, int32_t pad_right, int32_t act,
                   v2a_stream_t stream);

/* Layers 0 and 1 of the encoder in one pass: wave (n samples) -> out [n][32] time-major,
 *   x0 = Conv1d(1->32, k7)(reflect-pad 6 in front);  out = shortcut(x0) + block.3(ELU(block.1(ELU(x0), reflect-pad 2 in front)))
 * with block.1 = Conv1d(32->16, k3), block.3 = Conv1d(16->32, k1), shortcut = Conv1d(32->32, k1).  n >= 8.
 * params: 3376 floats, 16-byte aligned: stem weight [32][7], stem bias [32], shortcut weight [32][32], (shortcut bias + block.3
 * bias) [32], block.1 weight [16][3][32] (out, tap, in), block.1 bias [16], block.3 weight [32][16].
 * One thread per sample (~3.7 k VALU FMAs, weights at lane-uniform addresses), one coalesced write of the result.  Replaces the
 * zero-padded K = 16 stem GEMM and the nine passes of the generic path over [n][16..32] buffers. */
int v2a_encodec_stage0(const float* wave, const float* params, float* out, int64_t n, v2a_stream_t stream);

/* =======================================================================================
 * FLAN-T5 prompt encoder: `E2TTS.encode_text` x3:1648-1657 running transformers `T5EncoderModel` (x3:1413, 1654), fp32.
 * Per block: h += o(Attn(LN1(h))); h += wo(gelu_new(wi_0 LN2(h)) * wi_1 LN2(h)); then final_layer_norm.
 * ===================================================================================== */

/* T5LayerNorm: y[m] = w * x[m] * rsqrt(mean(x[m]^2) + eps), fp32, d % 4 == 0, 16-byte aligned rows.
 * With ids != NULL row m of x is the embedding row ids[m] of the table x (vocab rows, row stride ldx) and is also written to
 * resid[m] (the residual stream): the embedding gather of T5Stack fused into the first LN.  The caller validates the ids.
 * Replaces: transformers T5LayerNorm (LN1, LN2, final_layer_norm) and the embed_tokens lookup, reached from x3:1413,1654. */
int v2a_t5_rmsnorm(const float* x, int64_t ldx, const int32_t* ids, int32_t vocab, float* resid, int64_t ldr, float* y, int64_t ldy,
                   int64_t rows, int32_t d, const float* w, float eps, v2a_stream_t stream);

/* T5Attention core (d_kv = 64, N <= 512), fp32 VALU with an online softmax over 64-key blocks:
 *   s[b,h,i,j] = q[b,i,h,:] . k[b,j,h,:] + bias[h][j - i + N - 1]      (no 1/sqrt(d) scale)
 *   o[b,i,h,:] = softmax_j(s | key_mask[b][j] != 0) v[b,j,h,:]          for every row i, padded rows included
 * q/k/v/out are addressed as base + b*batch_stride + token*row_stride + h*64 (+c), so q, k, v are read in place from the fused
 * [q | k | v] GEMM output.  bias is the relative-position bias gathered per call from the bucket table and the
 * relative_attention_bias embedding (num_buckets x H) of block 0.  A batch row with no valid key is the caller's error (it gets 0).
 * Replaces: transformers T5Attention minus its Linears (T5LayerSelfAttention), reached from x3:1413,1654. */
typedef struct v2a_t5_attn_args {
  const float *q, *k, *v;
  float* out;
  int64_t q_row_stride, k_row_stride, v_row_stride, out_row_stride;
  int64_t q_batch_stride, k_batch_stride, v_batch_stride, out_batch_stride;
  int32_t B, H, N, d_kv;
  const float* bias;        /* [H][2N - 1] */
  const int32_t* key_mask;  /* [B][N], 0 / 1 */
} v2a_t5_attn_args;
int v2a_t5_attention(const v2a_t5_attn_args* args, v2a_stream_t stream);

/* Exact-fp32 GEMM for few rows (the encoder at B*N <= 128 rows streams 51 MB of fp32 weights per block): a subset of
 * v2a_gemm_args -- nseg 1, a_dtype / compute_dtype / out_dtype V2A_F32, K % 32 == 0, 16-byte aligned A / W rows, M <= 8192 --
 * and the epilogues STORE (N % 16 == 0), RESID (resid may alias out) and GEGLU_TANH (N % 32 == 0, out has N/2 columns).  Each
 * workgroup owns 16 output columns (32 packed rows for GEGLU_TANH) and its 8 waves split K; the partial sums are added in a fixed
 * order, so the result is the same bits on every run and for every M.  v2a_gemm's dispatch is unaffected.
 * Replaces: the Linears of transformers T5Attention (fused q|k|v, o) and T5DenseGatedActDense (wi_0 | wi_1, wo) with the
 * residual add of T5LayerSelfAttention / T5LayerFF, reached from x3:1413,1654. */
int v2a_gemm_skinny_f32(const v2a_gemm_args* args, v2a_stream_t stream);

/* =======================================================================================
 * N3: CLIP ViT image encoder, `video_encoder="clip_vit"` of the reference: transformers CLIPImageProcessor() +
 * CLIPVisionModelWithProjection (IP-Adapter sdxl_models/image_encoder = OpenCLIP ViT-bigG/14), x3:1423-1425, 1714, 1733-1735.
 * Per layer: h += out_proj(Attn(LN1(h))); h += fc2(gelu(fc1(LN2(h)))); image_embeds = visual_projection(post_layernorm(h[CLS])).
 * The Linears are v2a_gemm calls (fc1 with V2A_EPI_GELU); the kernels below are the rest.
 * ===================================================================================== */

/* Pillow BICUBIC resize (Image.resize(..., BICUBIC, reducing_gap=None), the 8-bit path of ImagingResample), horizontal pass:
 *   tmp[f][y - y0][x][c] = clip8((2^21 + sum_{i < bounds[2x+1]} frames[f][y][bounds[2x] + i][c] * coef[x * ksize + i]) >> 22)
 * frames (F, H, W, 3) uint8 RGB; tmp (F, rows, S, 3) uint8 for the input rows y0 <= y < y0 + rows and the S output columns of the
 * centre crop.  bounds / coef: Pillow's precompute_coeffs + normalize_coeffs_8bpc for those columns (22 fraction bits), built on
 * the host; the CALLER guarantees bounds[2x] + bounds[2x+1] <= W.
 * Replaces: the resize of CLIPImageProcessor.preprocess (transformers image_transforms.resize -> PIL), reached from x3:1714. */
int v2a_clip_resize_h(const uint8_t* frames, int32_t F, int32_t H, int32_t W, uint8_t* tmp, int32_t y0, int32_t rows, int32_t S,
                      const int32_t* bounds, const int32_t* coef, int32_t ksize, v2a_stream_t stream);
/* Vertical pass of the same resize over tmp, for the S crop rows (bounds relative to row y0 of tmp; the CALLER guarantees
 * bounds[2y] + bounds[2y+1] <= rows), then rescale + normalise through lut[c * 256 + u] (the processor's fp32 value of byte u in
 * channel c, built on the host), written as the patch matrix of the stride-P patch convolution:
 *   patches[f * (1 + (S/P)^2) + 1 + (y/P) * (S/P) + x/P][c * P * P + (y % P) * P + x % P]
 * Row f * (1 + (S/P)^2) (the class-token slot) and columns >= 3 P^2 are never written: the caller zeroes them once.  out_dtype
 * V2A_F32 (ldp floats per row) or V2A_BF16_SPLIT (hi at the column, lo lo_offset bf16 further, ldp bf16 per row).  crop (or NULL)
 * receives the uint8 crop (F, S, S, 3).  Replaces: resize + center_crop + rescale + normalize of CLIPImageProcessor (x3:1423, 1714). */
int v2a_clip_resize_v(const uint8_t* tmp, int32_t F, int32_t rows, int32_t S, int32_t P, const int32_t* bounds, const int32_t* coef,
                      int32_t ksize, const float* lut, void* patches, int64_t ldp, int32_t out_dtype, int64_t lo_offset, uint8_t* crop,
                      v2a_stream_t stream);
/* h[r][c] = pos[r % T][c] + (r % T == 0 ? cls[c] : 0) for rows r < rows: the class / position embedding rows of the residual stream,
 * onto which the patch GEMM (RESID epilogue over the patch matrix above, whose class rows are zero) adds the patch embeddings.
 * Replaces: CLIPVisionEmbeddings (class_embedding, position_embedding) reached from x3:1733-1735. */
int v2a_clip_embed_init(float* h, int64_t ldh, int64_t rows, int32_t T, int32_t d, const float* cls, const float* pos,
                        v2a_stream_t stream);
/* nn.LayerNorm: y[r] = (x[r] - mean) / sqrt(var + eps) * gamma + beta (biased variance, fp32, centred two-pass), d % 4 == 0,
 * d <= 4096.  y_dtype V2A_F32 or V2A_BF16_SPLIT (row = [hi | lo] halves of ldy >= 2d bf16, lo at ldy / 2: columns d .. ldy/2 - 1 of
 * each half are not written, a zero K pad for the GEMM).  ldx is free: ldx = T * d with rows = F
 * normalises the class rows only.  Replaces: CLIPVisionTransformer.pre_layrnorm / post_layernorm and CLIPEncoderLayer
 * layer_norm1 / layer_norm2 (transformers), reached from x3:1733-1735. */
int v2a_clip_layernorm(const float* x, int64_t ldx, void* y, int64_t ldy, int32_t y_dtype, int64_t rows, int32_t d, const float* gamma,
                       const float* beta, float eps, v2a_stream_t stream);
/* Bidirectional, unmasked attention core, fp32 (VALU FMA, online softmax over 32-key blocks) in every compute mode:
 *   o[b,i,h,:] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) v[b,j,h,:]
 * q / k / v (fp32) are addressed as base + b * batch_stride + token * row_stride + h * d_head (+c) -- read in place from the fused
 * [q | k | v] GEMM output; d_head a multiple of 4, <= 112 (104 for ViT-bigG), N <= 4096 (257 at 224 px, 577 at 336 px).
 * out_split = 0: fp32 out; 1: bf16 out row = [hi of the H * d_head outputs | lo of them], the lo plane at out_row_stride / 2 (the
 * out-projection's split operand; columns past H * d_head in each half are not written).
 * Replaces: transformers CLIPAttention minus its Linears (eager path), reached from x3:1733-1735. */
typedef struct v2a_clip_attn_args {
  const float *q, *k, *v;
  void* out;
  int64_t row_stride, batch_stride;          /* q / k / v, in floats          */
  int64_t out_row_stride, out_batch_stride;  /* in elements of out            */
  int32_t B, H, N, d_head;
  float scale;
  int32_t out_split;
} v2a_clip_attn_args;
int v2a_clip_attention(const v2a_clip_attn_args* args, v2a_stream_t stream);

/* =======================================================================================
 * N3: piano-frame preprocessing, the uncached `piano` branch of `E2TTS.encode_video_frames` (x3:1876-1891 with the
 * module-level `transform`, x3:60-63): per decoded frame Image.convert('L'), Image.resize((900, 100)) (BICUBIC), / 255.
 * Two integer passes, equal to Pillow bit for bit; tables from the host as for v2a_clip_resize_h / _v.
 * ===================================================================================== */

/* Grey + horizontal pass.  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow rgb2l) of every tap is formed in registers, then
 *   tmp[j][y - y0][x] = clip8((2^21 + sum_{i < bounds[2x+1]} L(frames[f_j][y][bounds[2x] + i]) * coef[x * ksize + i]) >> 22)
 * for j < n, y0 <= y < y0 + rows, x < Wo, with f_j = sel[j] (device int32, any order, repeats allowed; the CALLER guarantees
 * 0 <= sel[j] < F) or j when sel is NULL (then n <= F).  frames (F, H, W, 3) uint8 RGB, 4-byte aligned; tmp (n, rows, ldt) uint8,
 * ldt >= Wo a multiple of 4 (columns >= Wo of a row hold nothing).  n <= 65535 per call; 4 * ceil(W / 4) * 4 bytes of LDS.  The
 * CALLER guarantees bounds[2x] + bounds[2x+1] <= W and bounds[2x+1] <= ksize.
 * Replaces: Image.convert('L') and the horizontal pass of Image.resize at x3:1883-1886. */
int v2a_piano_resize_h(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const int32_t* sel, int32_t n, uint8_t* tmp, int32_t ldt,
                       int32_t y0, int32_t rows, int32_t Wo, const int32_t* bounds, const int32_t* coef, int32_t ksize,
                       v2a_stream_t stream);
/* Vertical pass over tmp (bounds relative to its row 0; the CALLER guarantees bounds[2y] + bounds[2y+1] <= rows and
 * bounds[2y+1] <= ksize), clipped to a byte u, stored as lut[u] (256 floats, float32(float64(u) / 255.0) built on the host):
 *   out[j][y][x] = lut[clip8((2^21 + sum_i tmp[j][bounds[2y] + i][x] * coef[y * ksize + i]) >> 22)],  out (n, Ho, Wo) fp32 contiguous,
 * 16-byte aligned when Wo % 4 == 0.  Replaces: the vertical pass of Image.resize, the reshape and `x / 255.` of `transform` (x3:60-63)
 * and the float32 cast of x3:1890. */
int v2a_piano_resize_v(const uint8_t* tmp, int32_t n, int32_t rows, int32_t ldt, int32_t Ho, int32_t Wo, const int32_t* bounds,
                       const int32_t* coef, int32_t ksize, const float* lut, float* out, v2a_stream_t stream);
/* The vertical pass with a transposed store, for the 88-key configuration's portrait frames: the same sums, clip and table as
 * v2a_piano_resize_v (same arguments, same caller guarantees), stored as
 *   out[j][x][y],  out (n, Wo, Ho) fp32 contiguous, 16-byte aligned when Ho % 4 == 0.
 * A workgroup forms a band of 32 output rows y in LDS and writes runs along y.  Wo <= 488 (the band and the table in 64 KB of LDS).  Replaces: the
 * vertical pass of `x.resize((100, 900))`, the reshape to (900, 100, 1), the transpose [2, 1, 0] and `x / 255.` of `transform`
 * (x3_2 = e2_tts_crossatt3_2.py:65-68) and the float32 cast of x3_2:1906. */
int v2a_piano_resize_vt(const uint8_t* tmp, int32_t n, int32_t rows, int32_t ldt, int32_t Ho, int32_t Wo, const int32_t* bounds,
                        const int32_t* coef, int32_t ksize, const float* lut, float* out, v2a_stream_t stream);

/* =======================================================================================
 * Encodec residual vector quantizer: the part of `EncodecModel.encode` / `.decode` between the encoder (v2a_encodec_stage0 and the
 * GEMM stack) and the vocoder.  Additive to ABI 8.
 * ===================================================================================== */

/* Latents -> codes, all n_q stages in one launch.  With r_0 = x[frame] (D = 128 floats), for s = 0 .. n_q - 1:
 *   codes[s][frame] = arg-max_j (2 r_s . e^s_j - norms[s][j])      (lowest j among equal scores)
 *   r_{s+1}         = r_s - e^s_{codes[s][frame]}                  (fp32, one rounding per element and stage)
 * The products are exact fp32 (fp32-input MFMA, one rounding per product, accumulated in a fixed order that does not depend on the
 * other frames of the launch).  x is read in place as x[b * batch_stride + t * frame_stride + c * chan_stride] (strides in floats,
 * >= 0), b < B, t < T: both (b, 128, t) and (b, t, 128) tensors.  codebooks (S, Kc, D) fp32 contiguous, 16-byte aligned, of which
 * the first n_q <= S stages are used; norms (S, Kc) = |e^s_j|^2, precomputed by the caller; D == 128, Kc a multiple of 512;
 * codes (n_q, B * T) int64, frame = b * T + t; B * T <= 2^30.
 * Replaces: `EncodecEuclideanCodebook.quantize` (the distance matrix and its arg-max) inside `EncodecResidualVectorQuantizer.encode`
 * (the stage loop with `residual = residual - quantized`), transformers/models/encodec/modeling_encodec.py. */
int v2a_encodec_rvq_encode(const float* x, int64_t batch_stride, int64_t frame_stride, int64_t chan_stride, int32_t B, int32_t T,
                           const float* codebooks, const float* norms, int32_t S, int32_t Kc, int32_t D, int32_t n_q, int64_t* codes,
                           v2a_stream_t stream);
/* Codes -> latents: out[frame] = ((0 + e^0[codes[0][frame]]) + e^1[codes[1][frame]]) + ... in fp32, in stage order, written through
 * the same three strides.  codes (n_q, B * T) int64, n_q <= S; the CALLER guarantees 0 <= codes < Kc (an index outside is clamped
 * into the codebook, never followed).  D == 128.
 * Replaces: `EncodecResidualVectorQuantizer.decode` (`quantized_out = quantized_out + layer.decode(indices)`) with
 * `EncodecEuclideanCodebook.decode` (the embedding lookup), transformers/models/encodec/modeling_encodec.py. */
int v2a_encodec_rvq_decode(const int64_t* codes, int32_t n_q, int32_t B, int32_t T, const float* codebooks, int32_t S, int32_t Kc, int32_t D,
                           float* out, int64_t batch_stride, int64_t frame_stride, int64_t chan_stride, v2a_stream_t stream);

/* =====================================================================================
 * Validation pass of E2TTS.forward(val=True) (e2_tts_crossatt3.py:2307-2588): the interpolation in front of the DiT and the two
 * losses behind it.  Additive: the ABI version does not change.
 * ===================================================================================== */

/* Workgroup partials of v2a_masked_sqerr / v2a_roll_metrics: `scratch` holds V2A_LOSS_MAX_PARTS * 2 (resp. * 6) doubles. */
#define V2A_LOSS_MAX_PARTS 256

/* One pass over the (B, T, C) fp32 latents, t (B) fp32:
 *   w    = (1 - t[b]) * x0 + t[b] * x1     two rounded products and a rounded sum (no FMA): torch's fp32 result bit for bit
 *   flow = x1 - x0
 *   cond = span[b * T + n] ? 0 : x1        only when cond != NULL; span (B * T) bytes, NULL = no frame is in the span
 * C a multiple of 4, the five tensors contiguous and 16-byte aligned.
 * Replaces: `w = (1. - t) * x0 + t * x1`, `flow = x1 - x0` and the `einx.where` of x3:2394-2407. */
int v2a_cfm_interp(const float* x0, const float* x1, const float* t, const uint8_t* span, float* w, float* flow, float* cond, int32_t B,
                   int32_t T, int32_t C, v2a_stream_t stream);
/* out[0] = sum of (double(pred) - double(target))^2 over the elements of the frames with mask[b * T + n] != 0, out[1] = their number.
 * pred, target (B, T, C) fp32 contiguous, 16-byte aligned, C a multiple of 4; mask (B * T) bytes.  The sums are taken in double in
 * an order fixed by the shape (workgroup partials in `scratch`, then one workgroup over them; no atomics): two calls give the same bits.
 * Replaces: `F.mse_loss(pred, flow, reduction = 'none')[rand_span_mask].mean()` (x3:2542-2547) up to the final division. */
int v2a_masked_sqerr(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t T, int32_t C, double* scratch,
                     double* out, v2a_stream_t stream);
/* roll, midis (B, T, notes) fp32 contiguous, mask (B * T) bytes.
 *   out[0] = sum of (roll - midis)^2 * |midis - 0.10| in double over the elements of the masked frames, out[1] = their number
 *   out[2..5] = tp, fp, fn, tn over the (clip, g < T / 3, note) cells whose frames 3g, 3g + 1, 3g + 2 are all masked in, on the fp32
 *               means ((a + b) + c) / 3 of the three frames: roll mean >= 0.4f against midis mean >= 0.5f
 * Same fixed-order reduction as v2a_masked_sqerr.
 * Replaces: the roll loss and the pooled confusion counts of x3:2429-2443. */
int v2a_roll_metrics(const float* roll, const float* midis, const uint8_t* mask, int32_t B, int32_t T, int32_t notes, double* scratch,
                     double* out, v2a_stream_t stream);

/* =====================================================================================
 * Wave front end: the first channel of an audio file at any rate -> the 24 kHz, normalised wave the Encodec encoder reads
 * (trainer_multigpus_alldatas3.py:1047-1050 and 1427-1431, torch_tools.py:53-56).  Additive: the ABI version does not change.
 * ===================================================================================== */

/* Workgroup partials of v2a_wave_resample / v2a_wave_stats: `parts` holds V2A_WAVE_MAX_PARTS records of 16 bytes,
 * { double sum; float min; float max; }, 8-byte aligned; the entry point stores in *n_parts (host) how many it wrote. */
#define V2A_WAVE_MAX_PARTS 256
/* LDS a resampler workgroup may take for its input window and the filter table together; a table that does not fit beside the
 * window is read from global memory (same arithmetic, same bits). */
#define V2A_WAVE_LDS_BYTES (128 * 1024)
/* Largest filter table, n * K entries (16 MiB of fp32); wave.py refuses a rate pair above it before anything is allocated. */
#define V2A_WAVE_TABLE_MAX (1 << 22)

/* Polyphase sinc resampler.  o / n: input / output rate divided by their gcd; table (n, K) fp32, K = 2 * width + o, row p = the
 * taps of output phase p (wave.py: sinc_resample_table).  For j = q * n + p < out_len = ceil(n * L / o):
 *   y[j] = fma(xpad[q o + K - 1], table[p][K - 1], ... fma(xpad[q o + 1], table[p][1], fma(xpad[q o], table[p][0], 0)))
 * with xpad[i] = x[i - width] inside the wave and 0 outside: fp32, one chain from k = 0 up, so a sample does not depend on the
 * tiling of the launch nor on where the table was read from.  x (L) and y (out_len) fp32; nothing past y[out_len - 1] is written.
 * `parts` / *n_parts: the partials of y, see above.  K <= 8192, n * K <= V2A_WAVE_TABLE_MAX.
 * Replaces: `torchaudio.functional.resample(waveform, orig_freq, new_freq)` (trainer_multigpus_alldatas3.py:1048-1049, 1429-1430):
 * `_get_sinc_resample_kernel` is the host table, `_apply_sinc_resample_kernel` (pad, conv1d of stride o, transpose, cut) this launch. */
int v2a_wave_resample(const float* x, int64_t L, const float* table, int32_t o, int32_t n, int32_t K, int32_t width, float* y,
                      int64_t out_len, void* parts, int32_t* n_parts, v2a_stream_t stream);
/* The same partials for a wave x (n) that needs no resampling (orig_freq == new_freq).
 * Replaces: the reductions of `torch.mean(waveform)` and `torch.max(torch.abs(waveform[0, :]))` (torch_tools.py:54-55). */
int v2a_wave_stats(const float* x, int64_t n, void* parts, int32_t* n_parts, v2a_stream_t stream);
/* With (sum, min, max) = the n_parts partials combined in index order (no atomics: two calls give the same bits):
 *   m    = float(sum / n)                               the double sum divided in double, rounded once
 *   peak = max(fl32(max - m), fl32(m - min))            = max_i |fl32(x[i] - m)|, rounding being monotonic
 *   out[i] = ((x[i] - m) / (peak + 1e-8f)) * 0.5f       i < min(n, n_out): three rounded fp32 operations, IEEE division
 *   out[i] = 0                                          n <= i < n_out
 * and stats[0] = m, stats[1] = peak (device).  out is either x itself (in place) or does not overlap it.
 * Replaces: `normalize_wav` (torch_tools.py:53-56) and the cut `waveform[:, :val_length * hop_size]` that follows it in the
 * validation set (trainer_multigpus_alldatas3.py:1129-1134). */
int v2a_wave_normalize(const float* x, int64_t n, const void* parts, int32_t n_parts, float* out, int64_t n_out, float* stats,
                       v2a_stream_t stream);

/* =====================================================================================
 * Roll2Midi generator: the U-Net behind the Video2Roll key roll (`r2m` = src/audeo/Roll2MidiNet.py:42-87, run as in
 * Roll2Midi_inference.py:51-71).  Every convolution is 3x3 / stride 1 / pad 1, so all maps share one (n, H, W) pixel grid and each
 * of them is a v2a_gemm (eval-mode BatchNorm folded in, the transposed convolutions r2m:27 as plain ones with flipped, transposed
 * weights).  The three kernels below do what v2a_gemm cannot.  They address a CHANNEL SLICE of an NHWC fp32 map that may carry a
 * zero border of `border` pixels: pixel (i, y, x) of the slice starts at
 *   base + ((i*(H + 2*border) + y + border)*(W + 2*border) + x + border) * pitch,
 * base = the map + the slice's channel offset, pitch = the channels of the whole map (a multiple of 8; base 16-byte aligned).
 * A shadow is the copy the next convolution's GEMM reads, at the same offsets from `shadow`: shadow_mode 0 = none (shadow NULL),
 * 1 = bf16, 2 = V2A_BF16_SPLIT planes, hi = bf16(v) and, lo_offset elements further (>= the hi map, a multiple of 8), lo =
 * bf16(v - hi).  Only interiors are written: the caller zeroes the borders once.  Additive: the ABI version does not change.
 * ===================================================================================== */

/* down1 (r2m:46, 62): roll x (n, H, W) fp32 -> co channels (co % 8 == 0), 3x3 / pad 1, no bias, LeakyReLU(0.2).  wt is [9][co]
 * fp32, tap = ky*3 + kx.  Per output one chain acc = fma(wt[tap][c], x[y + ky - 1][x + kx - 1], acc) from tap 0 up (zero outside
 * the roll), then acc > 0 ? acc : 0.2f * acc.  K = 9 does not fill a K tile of v2a_gemm. */
int v2a_roll2midi_stem(const float* x, const float* wt, int32_t n, int32_t H, int32_t W, int32_t co, float* out, void* shadow,
                       int32_t shadow_mode, int64_t lo_offset, int64_t pitch, int32_t border, v2a_stream_t stream);
/* x = x > 0 ? x : 0.2f * x in place on the C channels (C % 8 == 0) of a slice, and the shadow of the result: the nn.LeakyReLU(0.2)
 * of down2..down6 (r2m:13), which no epilogue of v2a_gemm has.  leaky(0) = 0: a zero border stays zero without being touched. */
int v2a_leaky_shadow(float* x, void* shadow, int32_t shadow_mode, int64_t lo_offset, int32_t n, int32_t H, int32_t W, int32_t C,
                     int64_t pitch, int32_t border, v2a_stream_t stream);
/* conv1d + sigmoid (r2m:58, 84-86) and the threshold of Roll2Midi_inference.py:65 per pixel of two slices with one geometry, u
 * (nu channels of up5) and d (nd channels of down1), nu and nd multiples of 4, w (nu + nd) fp32:
 *   z = fma(w[nu + nd - 1], d[nd - 1], ... fma(w[nu], d[0], fma(w[nu - 1], u[nu - 1], ... fma(w[0], u[0], bias))))
 *   logits[i] = z,  probs[i] = 1 / (1 + expf(-z)),  midi[i] = probs[i] >= threshold        dense (n, H, W); NULL = not written */
int v2a_roll2midi_head(const float* u, int64_t u_pitch, int32_t nu, const float* d, int64_t d_pitch, int32_t nd, const float* w,
                       float bias, float threshold, int32_t n, int32_t H, int32_t W, int32_t border, float* logits, float* probs,
                       uint8_t* midi, v2a_stream_t stream);
/* Attention gate of Roll2MidiNet_enhance.py (`AttentionGate.forward`, enh:49-55) with theta_x, phi_g and psi folded into one weight
 * vector w (C0 + C1) fp32 and a bias (roll2midi.folded_gate).  Per pixel of the (n, H, W) grid, over the concatenation of segment 0
 * (C0 channels at x0, pitch0) and segment 1 (C1 channels at x1, pitch1; C1 = 0 with x1 = shadow1 = NULL: one segment), both with the
 * geometry above and one border; C0, C1 multiples of 8, C0 + C1 <= 2048 (one wave holds the pixel in registers):
 *   z = sum + bias, sum = xor butterfly over 64 lanes of the lanes' chains fma(w[c], x[c], acc) from 0 over channels
 *       c = 512 j + 8 lane + e (j, e ascending): the order depends on (C0, C1) alone, never on n, the grid or the other pixels
 *   alpha = 1 / (1 + expf(-z));   x[c] = x[c] * alpha in place (one fp32 multiply), and the shadow of the stored value at the same
 *   offsets of shadow0 / shadow1 (shadow_mode as above, lo_offset per segment).  Borders and other channels are not touched.
 *   logits[i] = z, alpha[i] = alpha   dense (n, H, W) fp32; NULL = not written.  Additive: the ABI version does not change. */
int v2a_roll2midi_gate(float* x0, int64_t pitch0, int32_t C0, void* shadow0, int64_t lo_offset0, float* x1, int64_t pitch1, int32_t C1,
                       void* shadow1, int64_t lo_offset1, const float* w, float bias, int32_t shadow_mode, int32_t n, int32_t H, int32_t W,
                       int32_t border, float* logits, float* alpha, v2a_stream_t stream);

/* =====================================================================================
 * Note extraction: the link behind Roll2Midi in the reference's Audeo chain, `process_midi` / `process_roll` and `GetNote` of
 * src/audeo/Midi_synth.py:33-118 -- a binarised key roll -> onsets and offsets -> (key, start, end) rows.
 * Additive: the ABI version does not change.
 * ===================================================================================== */

#define V2A_ROLL_NOTES_MAX_KEYS 128
#define V2A_ROLL_NOTES_TILE 256                 /* frames a workgroup holds in LDS at a time; T itself is not bounded by LDS */
#define V2A_ROLL_NOTES_MAX_FRAMES (1 << 24)     /* keys * ceil(T / 2) rows of a clip stay inside int32 */

/* roll: element (b, j, i) = clip b, frame j < T, key i < keys at roll[b * batch_stride + j * frame_stride + i * key_stride] (strides in
 * ELEMENTS: a (B, T, keys) tensor and a transposed (B, keys, T) view are both read in place).  elem_bytes 1: bytes, on iff != 0;
 * elem_bytes 4: fp32, on iff > threshold (a NaN is off; threshold is ignored for bytes).  lens (B) int32 or NULL: the valid frames of
 * every clip, clamped to [0, T] (NULL: T); frames at or beyond lens[b] count as off and are not read.
 *   onset at (j, i):  on at j and (j == 0 or off at j - 1)          Midi_synth.py:54-61, 85-92
 *   offset at (j, i): j > 0, on at j - 1 and off at j; a key on at frame lens[b] - 1 has its last offset at lens[b]   (:104-105, 115-116)
 *   notes of key i = (k-th onset, k-th offset), k = 0 .. counts[b][i] - 1                                              (:106, 117)
 * counts (B, keys) int32; totals (B) int32 = the sum of a clip's counts; notes (B, cap, 3) int32 rows (key, start, end) of clip b from
 * notes + b * cap * 3 on, ordered by key, then by start.  Rows at or beyond min(totals[b], cap) are NOT written; totals[b] > cap is no
 * error of this call (it returns 0, totals holds the true count: the caller compares).  cap = 0 with notes NULL: counts only.
 * onset (B, keys, T) int8 or NULL: +1 at an onset, -1 at an offset at a frame < T, 0 elsewhere -- every element is written (the
 * reference's `onset.T`).  One launch of B workgroups, no atomics, no host synchronisation; a clip's results do not depend on B or on
 * the other clips.  keys <= V2A_ROLL_NOTES_MAX_KEYS, T <= V2A_ROLL_NOTES_MAX_FRAMES. */
int v2a_roll_notes(const void* roll, int32_t elem_bytes, int64_t batch_stride, int64_t frame_stride, int64_t key_stride, float threshold,
                   int32_t B, int32_t T, int32_t keys, const int32_t* lens, int32_t* counts, int32_t* totals, int32_t* notes, int32_t cap,
                   int8_t* onset, v2a_stream_t stream);

/* =====================================================================================
 * Log-mel front end: the reference's `MelSpec` (x3:375-417) -- torchaudio's MelSpectrogram and log(clamp(mel, 1e-5)) (x3:293-294).
 * v2a_mel_pad, the exact-fp32 v2a_gemm over overlapping rows (lda = hop, K = n_fft, W = the windowed real DFT basis with the rows of
 * bin k at 2k (re) and 2k + 1 (im): mel.py, stft_basis), v2a_mel_from_dft.  The GEMM adds its K products in one fp32 chain, so K is cut
 * into chunks (256 samples in mel.py): one launch per chunk on the same rows, A and W moved by the chunk, each into a partial DFT of its
 * own.  Window, normalisation and mel norm live in the two host tables; the kernels know n_fft, hop, the bins, n_mels and power.
 * Additive: the ABI version does not change.
 * ===================================================================================== */

#define V2A_MEL_MAX_FFT 2048                    /* a workgroup of v2a_mel_from_dft holds n_fft / 2 + 1 bins of 16 frames in LDS */
#define V2A_MEL_MAX_CHUNKS 16                   /* partial DFTs of one frame: mel.py cuts K into chunks of 256 samples */

/* B waves x (row b at x + b * ldx, nw samples) -> out + b * pitch: `pad` reflected samples, the wave, `pad` reflected samples
 * (torch.stft's center = True with pad_mode = "reflect": the edge sample is not repeated; pad < nw), pad = 0: a copy.  Only the
 * nw + 2 pad samples of every clip are written; pitch >= nw + 2 pad.  With pitch a multiple of hop, frame t of clip b is row
 * b * pitch / hop + t of the GEMM behind it. */
int v2a_mel_pad(const float* x, int64_t ldx, int32_t B, int64_t nw, int32_t pad, float* out, int64_t pitch, v2a_stream_t stream);
/* dft: n_chunks partial DFTs, chunk_stride floats apart, each fp32 rows of ld_dft floats with (re, im) of bin k at 2k and 2k + 1,
 * k < n_fft / 2 + 1; frame t < T of clip b < B is row b * rows_per_clip + t (rows_per_clip >= T: the rows between two clips are never
 * read).  re and im of a bin are its partials added in chunk order, ((c0 + c1) + c2) + ...  Per frame and bin
 *   p[k] = fma(im, im, re * re)  (power 2)   or   sqrt of it, correctly rounded  (power 1)
 * and per mel channel m, with (first, count) = bands[2m], bands[2m + 1] and w = weights + m * wpitch,
 *   mel = fma(w[count - 1], p[first + count - 1], ... fma(w[1], p[first + 1], fma(w[0], p[first], 0)))
 * one fp32 chain in ascending bin order, so a value does not depend on the tiling, on B or on T.  Stored at
 * out[b * out_batch_stride + m * out_row_stride + t]: float(log((double)max(mel, eps))), the log taken in double and rounded once,
 * or mel itself when eps < 0.  Nothing else of out is written.  `bands` (device) and `bands_host` (host) hold the same n_mels pairs:
 * the entry point checks the host copy (0 <= first, 0 <= count <= wpitch, first + count <= bins), the kernel clamps what it reads.
 * n_fft even, 4 .. V2A_MEL_MAX_FFT; hop a positive multiple of 4 (the GEMM's lda); power 1 or 2; no atomics. */
int v2a_mel_from_dft(const float* dft, int64_t ld_dft, int64_t rows_per_clip, int32_t n_chunks, int64_t chunk_stride, int32_t B, int32_t T,
                     int32_t n_fft, int32_t hop, int32_t n_mels, const int32_t* bands_host, const int32_t* bands, const float* weights, int32_t wpitch,
                     int32_t power, float eps, float* out, int64_t out_batch_stride, int64_t out_row_stride, v2a_stream_t stream);

/* =====================================================================================
 * Vocos vocoder, mel variant with padding = "center": mel frames -> wave, the `vocos` of a model whose latents are log-mel frames
 * (Vocos.from_pretrained('charactr/vocos-mel-24khz'), e2_tts_crossatt.py:1324, e2_tts_crossatt6.py:1469; `self.vocos.decode`,
 * x3:2275-2287).  vocos.py runs it as: v2a_vocos_stage_in, v2a_gemm (embed conv over overlapping rows), v2a_clip_layernorm, per
 * block v2a_vocos_dwconv_ln + v2a_gemm (pwconv1) + v2a_vocos_gelu + v2a_gemm (pwconv2) + v2a_vocos_scale_residual, v2a_clip_layernorm,
 * v2a_gemm (head), v2a_vocos_spectrum, v2a_gemm against the inverse-DFT basis of vocos.py (window, 1 / n_fft and the factor 2 of the
 * inner bins folded in), v2a_vocos_overlap_add.  Every GEMM runs in K chunks of 256, chunk c added to the sum of the chunks before it by
 * the RESID epilogue: the exact-fp32 GEMM adds its K products in one chain whose error grows with K.  Activations are fp32 rows, frame t of clip b at row
 * b * rows_per_clip + t; vocos.py keeps rows_per_clip = T + 6, the rows between two clips are computed and never read.
 * `lens` (device int32[B] or NULL = T everywhere): clip b has lens[b] frames and is decoded as if it were alone -- every convolution
 * zero padded at its own end, its own envelope.  The kernels clamp lens[b] to 0 .. T.  No atomics.
 * Additive: the ABI version does not change.
 * ===================================================================================== */

#define V2A_VOCOS_MAX_DIM 2048                  /* d of v2a_vocos_dwconv_ln: a tile of 2 frames + 6 halo rows fits 64 KB of LDS */
#define V2A_VOCOS_MAX_FFT 4096
#define V2A_VOCOS_MAX_FRAMES (1 << 24)

/* x (B, C, T) fp32 channel-major (clip b at x + b * x_batch_stride, channel c at + c * x_chan_stride, unit stride along time) ->
 * out: B * (T + 6) rows of c_pad floats, row b * (T + 6) + 3 + t = frame t of clip b; the 3 rows on either side of a clip, the columns
 * C .. c_pad - 1 and the frames t >= lens[b] are zero.  Every element of out is written.  c_pad >= C, a multiple of 16.
 * Replaces: the zero padding of `backbone.embed` (Conv1d(C, dim, 7, padding=3)) -- the convolution itself is v2a_gemm on rows
 * b * (T + 6) + t with lda = c_pad and K = 7 c_pad. */
int v2a_vocos_stage_in(const float* x, int64_t x_batch_stride, int64_t x_chan_stride, int32_t B, int32_t C, int32_t T, const int32_t* lens,
                       float* out, int32_t c_pad, v2a_stream_t stream);
/* Per frame t < lens[b] of clip b (row r = b * rows_per_clip + t) and channel c < d:
 *   a[c] = fma(wt[6 d + c], x[t + 3][c], ... fma(wt[d + c], x[t - 2][c], fma(wt[c], x[t - 3][c], bias[c])))     x[u] = 0 outside [0, lens[b])
 *   y[r][c] = (a[c] - mean) / sqrt(var + eps) * gamma[c] + beta[c]     mean, var over the d channels (biased, centred two-pass, fp32)
 * wt is tap-major, (7, d): wt[j * d + c] = dwconv.weight[c][0][j].  Rows lens[b] <= t < T of y are zeroed, nothing else is written.
 * d a multiple of 16, 16 .. V2A_VOCOS_MAX_DIM; ldx, ldy >= d and multiples of 4; x != y.
 * Replaces: ConvNeXtBlock.dwconv and ConvNeXtBlock.norm of the Vocos backbone. */
int v2a_vocos_dwconv_ln(const float* x, int64_t ldx, const float* wt, const float* bias, const float* gamma, const float* beta, float eps,
                        int32_t B, int32_t T, int64_t rows_per_clip, int32_t d, const int32_t* lens, float* y, int64_t ldy, v2a_stream_t stream);
/* x[r][c] = 0.5 x (1 + erf(x / sqrt 2)) in place, r < rows, c < n; n a multiple of 4, ldx >= n a multiple of 4.
 * Replaces: ConvNeXtBlock.act (nn.GELU) behind pwconv1. */
int v2a_vocos_gelu(float* x, int64_t ldx, int64_t rows, int32_t n, v2a_stream_t stream);
/* out[r][c] = fma(gamma[c], p[r][c], resid[r][c]), r < rows, c < n; n and the row strides multiples of 4; out may be resid, not p.
 * Replaces: ConvNeXtBlock's `residual + self.gamma * x`. */
int v2a_vocos_scale_residual(const float* p, int64_t ldp, const float* gamma, const float* resid, int64_t ldr, float* out, int64_t ldo,
                             int64_t rows, int32_t n, v2a_stream_t stream);
/* logits: `rows` rows of n_fft + 2 floats, log-magnitudes m[k] at k and phases p[k] at n_fft / 2 + 1 + k, k <= n_fft / 2 ->
 * spec[r][2k] = float(min(exp(m), 100) cos p), spec[r][2k + 1] = float(min(exp(m), 100) sin p): exp, cos, sin and the products in double
 * from the fp32 logits, rounded once.  Columns n_fft + 2 .. ld_spec - 1 are zeroed (the K pad of the GEMM behind it); ld_spec even.
 * Replaces: ISTFTHead.forward up to the complex spectrogram. */
int v2a_vocos_spectrum(const float* logits, int64_t ld_logits, int64_t rows, int32_t n_fft, float* spec, int64_t ld_spec, v2a_stream_t stream);
/* torch.istft's overlap-add (center = True) in gather form.  frames: rows of n_fft floats, irfft(S[:, t]) * w of frame t of clip b at
 * row b * rows_per_clip + t; wsq[j] = w[j]^2.  For n < (lens[b] - 1) hop, with p = n + n_fft / 2,
 *   out[b * out_batch_stride + n] = (sum_t frames[t][p - t hop]) / (sum_t wsq[p - t hop])      over t < lens[b] with 0 <= p - t hop < n_fft,
 * both sums fp32 in ascending t, one IEEE division.  Nothing else of out is written.  1 <= hop <= n_fft, T >= 2.
 * Replaces: ISTFT.forward (torch.istft) of the Vocos head. */
int v2a_vocos_overlap_add(const float* frames, int64_t ld_frames, int64_t rows_per_clip, const float* wsq, int32_t B, int32_t T, int32_t n_fft,
                          int32_t hop, const int32_t* lens, float* out, int64_t out_batch_stride, v2a_stream_t stream);

/* =======================================================================================
 * N3: CLIP ConvNeXt image encoder, `video_encoder="clip_convnext"` of the reference (and the third part of "mixed"):
 * open_clip's `image_encoder.encode_image` = TimmModel.forward = head(trunk(x)) around timm's ConvNeXt (x3:1429-1431, 1716-1720,
 * 1739-1741).  convnext.py runs it as: v2a_clip_resize_h / _v (patches of 4), v2a_gemm (stem.0), v2a_clip_layernorm (stem.1), per stage
 * v2a_clip_layernorm + v2a_im2col + v2a_gemm (downsample), per block v2a_convnext_dwconv + v2a_clip_layernorm + v2a_gemm (mlp.fc1,
 * V2A_EPI_GELU) + v2a_gemm (mlp.fc2 with gamma folded in, V2A_EPI_RESID), then v2a_convnext_pool_ln + v2a_gemm (head.proj).  Maps are
 * fp32 NHWC, (F, H, W, C) dense.  No atomics.  Additive: the ABI version does not change.
 * ===================================================================================== */

/* out[f][y][x][c] = bias[c] + sum_{ky, kx < 7} wt[(ky * 7 + kx) * C + c] * x[f][y + ky - 3][x + kx - 3][c], x = 0 outside the map:
 * per output ONE fp32 chain acc = bias, acc = fma(w, x, acc) in ascending (ky, kx) order, so a pixel's bits depend neither on the
 * tiling nor on F nor on the frame's position.  wt is tap-major, (49, C): wt[(ky * 7 + kx) * C + c] = conv_dw.weight[c][0][ky][kx].
 * Any H, W >= 1 (maps smaller than the kernel included); C a multiple of 4; x != out; F <= 65535.
 * Replaces: ConvNeXtBlock.conv_dw (nn.Conv2d(C, C, 7, padding=3, groups=C)) of timm's ConvNeXt. */
int v2a_convnext_dwconv(const float* x, float* out, const float* wt, const float* bias, int32_t F, int32_t H, int32_t W, int32_t C,
                        v2a_stream_t stream);
/* out[f][c] = LayerNorm_c(mean_p x[f * frame_stride + p * C + c]), p < pixels: the pixel sum of a channel is one fp32 chain in ascending
 * p, divided once; the LayerNorm is v2a_clip_layernorm's (biased variance, centred two-pass).  C <= 4096; one fp32 row of ldo >= C per
 * frame.  Replaces: the head of timm's ConvNeXt behind open_clip's TimmModel (global average pool, head.norm), pool = 'avg'. */
int v2a_convnext_pool_ln(const float* x, int64_t frame_stride, int32_t F, int32_t pixels, int32_t C, const float* gamma, const float* beta,
                         float eps, float* out, int64_t ldo, v2a_stream_t stream);

/* =======================================================================================
 * HiFi-GAN vocoder (AudioLDM's 16 kHz / 64-mel generator): mel frames -> wave, the `decode_to_waveform` half of `VaeWrapper.decode`
 * (x3:470-490, self.vocos = 'vae' at x3:1404-1409): `vocoder_infer` (src/audioldm/hifigan/utilities.py:76-86) around `Generator.forward`
 * (src/audioldm/hifigan/models.py:163-180).  hifigan.py runs it as: v2a_hifigan_act_pad + v2a_gemm (conv_pre), per stage
 * v2a_hifigan_act_pad + v2a_gemm (the transposed convolution in polyphase form), per ResBlock round either v2a_hifigan_act_pad + v2a_gemm
 * chains (tap segments, K chunks chained by V2A_EPI_RESID) or two v2a_hifigan_conv launches, v2a_hifigan_act_pad (the MRF mean), and
 * v2a_hifigan_post.  Activations are fp32 rows of C floats, frame t of clip b at row b * rows_per_clip + t.  `lens` (device int32[B] or
 * NULL = T everywhere): clip b has lens[b] frames at this stage and is decoded as if it were alone; the kernels clamp lens[b] to 0 .. T.
 * No atomics.  Additive: the ABI version does not change.
 * ===================================================================================== */

#define V2A_HIFIGAN_TILE 128                    /* frames of a workgroup of v2a_hifigan_conv */
#define V2A_HIFIGAN_MAX_ROWS (1 << 28)
#define V2A_HIFIGAN_POST_MAX_C 512              /* 16 samples + 6 halo rows of C + 1 floats fit 64 KB of LDS */

/* out: B clips of out_rows_per_clip rows of C floats (dense, row stride C); row halo + t of clip b, 0 <= t < lens[b], is
 *   leaky_relu(((s0 + s1) + s2) / divisor, slope)       of row b * src_rows_per_clip + t of the sources (row stride ld_src),
 * s1 and s2 optional (NULL), the sums and the IEEE division in fp32 in that order, the division skipped for divisor == 1,
 * leaky_relu(v) = v > 0 ? v : v * slope (slope 1: a copy).  Every other row of out -- the halo in front, everything behind the clip's own
 * length -- is zero; every element of out is written.  out_rows_per_clip >= T + 2 halo; C a multiple of 4.
 * Replaces: F.leaky_relu(x, LRELU_SLOPE) in front of every convolution (models.py:97-100, 165), `xs / self.num_kernels` (models.py:173),
 * F.leaky_relu(x) in front of conv_post (models.py:174, the default slope 0.01) and the zero padding of the convolutions behind them. */
int v2a_hifigan_act_pad(const float* s0, const float* s1, const float* s2, int64_t src_rows_per_clip, int64_t ld_src, int32_t B, int32_t T,
                        int32_t C, const int32_t* lens, float divisor, float slope, float* out, int64_t out_rows_per_clip, int32_t halo,
                        v2a_stream_t stream);
/* a: activated rows of C floats (dense), frame t of clip b at row b * rows_per_clip + t; frames outside [0, lens[b]) are taken as zero
 * whatever the buffer holds.  For t < lens[b]:
 *   pre = fma(w[6 C + C - 1], a[t + 3][C - 1], ... fma(w[1], a[t - 3][1], fma(w[0], a[t - 3][0], bias[0])))      w tap-major (7, C)
 *   wave[b * out_batch_stride + t] = tanhf(pre);  pcm[...] = (int16) trunc(wave * 32768) saturated to -32768 .. 32767;  pre[...] = pre
 * wave, pcm, pre optional, one of wave and pcm required; nothing else is written.  C <= V2A_HIFIGAN_POST_MAX_C.
 * Replaces: conv_post and torch.tanh (models.py:175-176) and `(wavs.cpu().numpy() * 32768).astype("int16")` (utilities.py:81). */
int v2a_hifigan_post(const float* a, int64_t rows_per_clip, int32_t B, int32_t T, int32_t C, const int32_t* lens, const float* w,
                     const float* bias, float* wave, int16_t* pcm, float* pre, int64_t out_batch_stride, v2a_stream_t stream);
/* Direct dilated Conv1d(C, C, k, dilation d, padding (k - 1) d / 2) with the leaky ReLU in front of it, on v_mfma_f32_16x16x4_f32.
 * For t < lens[b], row r = b * rows_per_clip + t:
 *   out[r][co] = sum_j (sum_ci W[co][ci][j] * leaky_relu(x[t + (j - (k - 1) / 2) d][ci], slope)) + bias[co] (+ resid[r][co])
 * x = 0 outside [0, lens[b]).  Per tap j one fp32 chain from zero over ci ascending, the taps' sums added in ascending j, then the bias,
 * then the residual: the bits of an output depend on (k, C) alone, not on the tile, the batch or the other clips.  wp holds W in
 * fragment order, k C C floats: float 4 i + e of wp, i = ((j * C / 16 + kq) * C / 16 + n) * 64 + lane, is
 * W[16 n + (lane & 15)][16 kq + 4 e + (lane >> 4)][j].  Rows t >= lens[b] of out are not written.  C = 32, 64 or 128; k odd;
 * (V2A_HIFIGAN_TILE + (k - 1) d) rows of C + 4 floats fit 160 KB of LDS; out != x, out may be resid; 16-byte aligned rows.
 * Replaces: one `c(F.leaky_relu(x, LRELU_SLOPE))` of ResBlock.forward, and for convs2 the `xt + x` behind it (models.py:96-102). */
int v2a_hifigan_conv(const float* x, int64_t ldx, int64_t rows_per_clip, int32_t B, int32_t T, int32_t C, const int32_t* lens,
                     const float* wp, const float* bias, int32_t k, int32_t d, float slope, const float* resid, int64_t ldr, float* out,
                     int64_t ldo, v2a_stream_t stream);

/* =======================================================================================
 * AudioLDM VAE decoder: latents -> the 64-bin mel image, the `decode_first_stage` half of `VaeWrapper.decode` (x3:470-490): `z / scale_factor`,
 * `post_quant_conv` and `Decoder.forward` (src/audioldm/variational_autoencoder/modules.py:650-683; ResnetBlock :155-175, AttnBlock :204-230,
 * Upsample :53-57, Normalize :38-41 = GroupNorm(32, eps 1e-6), nonlinearity :33-35 = x sigmoid(x)).  audioldm_vae.py runs it as:
 * v2a_vae_stage_in, then per GroupNorm v2a_vae_gn_stats + v2a_vae_gn_act_pad, per 3x3 convolution a chain of exact-fp32 v2a_gemm launches
 * (one A segment per kernel row over the flat padded grid, K in launches chained by V2A_EPI_RESID), the attention as v2a_gemm launches
 * around v2a_vae_softmax, v2a_vae_upsample_pad in front of an Upsample's convolution, and v2a_vae_conv_out.
 * Activations are channels-last fp32: time on H, frequency bins on W, C floats per pixel; Wp = W + 2.  Pixel (y, x) of clip b lies at row
 *   bordered:  b * rows_per_clip + (y + 1) Wp + (x + 1)      a one-pixel border around the clip, rows_per_clip >= (H + 2) Wp
 *   flat:      b * rows_per_clip + y * src_wp + x            what a GEMM over the bordered grid writes (src_wp = Wp), or dense (src_wp = W);
 *                                                            rows with x >= W or y >= lens[b] are never read
 * `lens` (device int32[B] or NULL = H everywhere): clip b has lens[b] rows of pixels at this stage and is decoded as if it were alone; the
 * kernels clamp lens[b] to 0 .. H.  No atomics; no sum's order depends on the batch.  Additive: the ABI version does not change.
 * ===================================================================================== */

#define V2A_VAE_GROUPS 32                       /* GroupNorm groups (modules.py:38) */
#define V2A_VAE_GN_TILE 512                     /* pixels of one partial sum of v2a_vae_gn_stats */
#define V2A_VAE_MAX_H (1 << 20)
#define V2A_VAE_MAX_W 4096
#define V2A_VAE_MAX_C 4096
#define V2A_VAE_MAX_Z 64
#define V2A_VAE_MAX_ROWS (1 << 28)

/* The latent z[b][c][t][w] is read at src + b * batch_stride + c * chan_stride + t * time_stride + w * bin_stride: emb (b, 16 zc, l) of
 * `VaeWrapper.decode`, whose z[b][c][t][w] = emb[b][16 c + w][t], has strides (16 zc l, 16 l, 1, l); z (b, zc, l, 16) has (16 zc l, 16 l, 16, 1).
 * out: the bordered map of c_pad channels, for t < lens[b]:
 *   out[..][co] = fma(w[co][zc - 1], z[zc - 1], ... fma(w[co][0], z[0], bias[co]))    co < zc, w (zc, zc) row-major;   0 for zc <= co < c_pad
 * The border and the rows at or behind lens[b] are zero; every element of out (B clips of out_rows_per_clip rows) is written.
 * zc <= c_pad <= V2A_VAE_MAX_Z, c_pad a multiple of 16 (the K granule of the GEMM behind it).
 * Replaces: the transposes and the reshape of VaeWrapper.decode (x3:478-481), `z = 1.0 / self.scale_factor * z` and `post_quant_conv` (the
 * host folds 1 / scale_factor into w in float64). */
int v2a_vae_stage_in(const float* src, int64_t batch_stride, int64_t chan_stride, int64_t time_stride, int64_t bin_stride, int32_t B, int32_t H,
                     int32_t W, int32_t zc, const int32_t* lens, const float* w, const float* bias, float* out, int32_t c_pad,
                     int64_t out_rows_per_clip, v2a_stream_t stream);
/* partials[((b * tiles + j) * 32 + g) * 2 + {0, 1}] = the sum and the sum of squares, in double, of group g (channels g C / 32 ..) over the
 * pixels j * V2A_VAE_GN_TILE <= p < (j + 1) * V2A_VAE_GN_TILE of clip b, p = y W + x counted from the clip's own first pixel, p < lens[b] W.
 * Order: thread s of 8 adds pixels p = s, s + 8, ... of the tile, a pixel's channels ascending, in one chain (squares by fma); the 8 chains
 * are added in ascending s.  Every entry of partials (B * tiles * 64 doubles) is written, zero where the tile holds no pixel of the clip.
 * x is a flat map (src_wp >= W).  C a multiple of 32 up to V2A_VAE_MAX_C; tiles >= ceil(H W / V2A_VAE_GN_TILE).
 * Replaces: the statistics of torch.nn.GroupNorm (modules.py:38-41). */
int v2a_vae_gn_stats(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* lens,
                     double* partials, int32_t tiles, v2a_stream_t stream);
/* Per (clip, group): S, SS = the partials of tiles 0 .. ceil(lens[b] W / V2A_VAE_GN_TILE) - 1 added in ascending order; n = lens[b] W C / 32;
 * mean = S / n, var = max(SS / n - mean^2, 0), rstd = 1 / sqrt(var + eps), all in double, mean and rstd then rounded to fp32 once.  Per element
 *   y = ((x - mean) * rstd) * gamma[c] + beta[c]          four separately rounded fp32 operations
 *   out = swish ? y / (1 + expf(-y)) : y                  libm expf, IEEE division
 * border 1: out is the bordered map (the operand of a convolution); border 0: dense rows b * out_rows_per_clip + y W + x (the attention's
 * norm).  Border pixels and rows at or behind lens[b] are zero; every element of out (B clips of out_rows_per_clip rows) is written:
 * this is the zero padding of the next convolution, per clip of a ragged batch.  out != x; 16-byte aligned rows.
 * Replaces: torch.nn.GroupNorm and `nonlinearity` (modules.py:157-158, 164-165, 206, 678-679). */
int v2a_vae_gn_act_pad(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* lens,
                       const double* partials, int32_t tiles, const float* gamma, const float* beta, double eps, int32_t swish, float* out,
                       int64_t out_rows_per_clip, int32_t border, v2a_stream_t stream);
/* out: the bordered map of 2 H x 2 W pixels (pitch 2 W + 2): pixel (Y, X), Y < 2 lens[b], is a bit copy of pixel (Y / 2, X / 2) of the flat
 * map x; the border and everything at or behind row 2 lens[b] are zero; every element of out is written.  C a multiple of 4.
 * Replaces: F.interpolate(scale_factor=2.0, mode="nearest") and the padding of the convolution behind it (modules.py:54-56). */
int v2a_vae_upsample_pad(const float* x, int64_t src_rows_per_clip, int32_t src_wp, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* lens,
                         float* out, int64_t out_rows_per_clip, v2a_stream_t stream);
/* In place over `rows` rows of ld floats: with v[j] = scale * s[j] (one rounded product), m = max_j v[j] over j < n,
 *   e[j] = expf(v[j] - m),   s[j] = e[j] / sum,   s[j] = 0 for n <= j < ld       (a PV GEMM may read K padded to its granule)
 * sum: thread t of 256 adds e[t], e[t + 256], ... in ascending order; a wave adds its 64 lanes by the xor butterfly (32, 16, .. 1); the four
 * waves' sums are added as (w0 + w1) + (w2 + w3).  scale > 0.
 * Replaces: `w_ * c ** -0.5` and softmax(dim=2) of AttnBlock.forward (modules.py:217-218). */
int v2a_vae_softmax(float* s, int64_t ld, int32_t rows, int32_t n, float scale, v2a_stream_t stream);
/* a: an activated bordered map of C channels (v2a_vae_gn_act_pad's).  For y < lens[b]:
 *   out[(b * H + y) * W + x] = fma chain from bias[0] over ky, then kx, then c ascending of w[(ky * 3 + kx) * C + c] * a[(y + ky, x + kx)][c]
 * ((y + ky, x + kx) in bordered coordinates), and 0 for y >= lens[b]: every element of out (B, H, W) is written -- time-major mel rows, the
 * row layout of hifigan.py.  C a multiple of 4.
 * Replaces: conv_out (modules.py:680) for out_ch = 1. */
int v2a_vae_conv_out(const float* a, int64_t rows_per_clip, int32_t B, int32_t H, int32_t W, int32_t C, const int32_t* lens, const float* w,
                     const float* bias, float* out, v2a_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2A_CFM_H */
