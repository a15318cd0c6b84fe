"""ctypes binding of libv2a_cfm.so (the C ABI declared in include/v2a_cfm.h).

The library is built in-tree by csrc/build.sh (hipcc --offload-arch=gfx950) and loaded
AFTER `import torch`, so its libamdhip64.so.7 dependency resolves to the HIP runtime torch
already loaded and torch streams / device pointers are valid in it.  There is no CPU
fallback: if the library is missing, every op raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libv2a_cfm.so")      # in-tree, next to this file; nothing is read from the environment
CSRC = os.path.join(_HERE, "csrc")

F32, BF16, BF16_SPLIT = 0, 1, 2
EPI_STORE, EPI_SIGMOID, EPI_GEGLU, EPI_RESID, EPI_GATE_RESID = 0, 1, 2, 3, 4
EPI_GEGLU_TANH = 5           # v2a_gemm_skinny_f32 only
EPI_GELU = 6                 # fp32 compute or split operands (CLIP's MLP)
EPI_SWIGLU = 7               # fp32 compute or split operands (DINOv2's feed-forward): the GEGLU packing, silu on the gate
EPI_QUICK_GELU = 9           # as EPI_GELU with v sigmoid(1.702 v) (the ViT-L/14-336 CLIP's MLP); 8 is v2a_gemm_cfg_euler's own

_lib = None


class V2AError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("a", C.c_void_p * 3), ("lda", C.c_int64 * 3), ("ka", C.c_int32 * 3),
        ("nseg", C.c_int32), ("a_dtype", C.c_int32),
        ("w", C.c_void_p), ("ldw", C.c_int64), ("bias", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("compute_dtype", C.c_int32), ("epilogue", C.c_int32),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("out_dtype", C.c_int32),
        ("out_bf16", C.c_void_p), ("ld_out_bf16", C.c_int64),
        ("resid", C.c_void_p), ("ldr", C.c_int64),
        ("gate", C.c_void_p), ("step", C.c_void_p),
        ("gate_step_stride", C.c_int64), ("gate_batch_stride", C.c_int64), ("rows_per_batch", C.c_int32),
        ("rope_table", C.c_void_p), ("rope_cols", C.c_int32), ("rope_pos_offset", C.c_int32), ("relu", C.c_int32),
        ("a_row_offset", C.c_void_p), ("a_ktile_offset", C.c_void_p), ("out_row_offset", C.c_void_p),
        ("tile_hint", C.c_int32),
        ("norm_gamma", C.c_void_p), ("norm_step_stride", C.c_int64), ("norm_batch_stride", C.c_int64),
        ("norm_switch_row", C.c_int32), ("norm_switch_offset", C.c_int32),
        ("norm_ssq", C.c_void_p), ("ld_norm_ssq", C.c_int64),
        ("row_ssq", C.c_void_p), ("ld_row_ssq", C.c_int64), ("row_ssq_parts", C.c_int32), ("row_norm_dim", C.c_int32),
        ("out_bf16_split", C.c_int32),
        ("a_lo_offset", C.c_int64 * 3), ("out_bf16_lo_offset", C.c_int64),
    ]


class GemmChoice(C.Structure):
    """Mirror of `v2a_gemm_choice`: what v2a_gemm would launch (v2a_gemm_choose)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "split", "bm", "bn", "bk", "waves_m", "waves_n", "stages", "tiles", "xcd_gm", "xcd_gn",
                                         "vec_epi")]


GEMM_REGISTER_STAGED, GEMM_RING, GEMM_8PHASE = 0, 1, 2       # v2a_gemm_choice.family

# The tile ids the engines ask for by name (the tile_hint tables of include/v2a_cfm.h).  Plain bf16 operands: k of v2a_tuning.gemm_force_tile,
# tile_hint = k + 1, profiler key tile<k>.  Split operands: the tile_hint itself, profiler key tile<hint - 1>.
TILE_128x128, TILE_8PHASE, TILE_128x128_8WAVES, TILE_128x64_8WAVES = 1, 6, 12, 14
SPLIT_TILE_8PHASE, SPLIT_TILE_128x256_K32 = 5, 6


class DwconvNorm(C.Structure):
    """Mirror of `v2a_dwconv_norm`: the RMSNorm after the depthwise convolution, folded into it."""
    _fields_ = [("out_bf16", C.c_void_p), ("ld_out_bf16", C.c_int64), ("norm_gamma", C.c_void_p), ("step", C.c_void_p),
                ("norm_step_stride", C.c_int64), ("norm_batch_stride", C.c_int64), ("norm_ssq", C.c_void_p), ("ld_norm_ssq", C.c_int64),
                ("split", C.c_int32), ("reserved", C.c_int32)]


class Tuning(C.Structure):
    """Mirror of `v2a_tuning` (include/v2a_cfm.h): explicit tile-selection overrides, nothing is read from the environment."""
    _fields_ = [("gemm_force_tile", C.c_int32), ("gemm_k_rotation", C.c_int32), ("gemm_8phase", C.c_int32),
                ("gemm_8phase_min_tiles", C.c_int32), ("dwconv_rows_per_wave", C.c_int32), ("gemm_xcd_order_1x8", C.c_int32),
                ("attn_one_group_from", C.c_int32), ("reserved", C.c_int32 * 1)]


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("gate", C.c_void_p), ("out", C.c_void_p),
        ("q_row_stride", C.c_int64), ("k_row_stride", C.c_int64), ("v_row_stride", C.c_int64),
        ("gate_row_stride", C.c_int64), ("out_row_stride", C.c_int64),
        ("q_batch_stride", C.c_int64), ("k_batch_stride", C.c_int64), ("v_batch_stride", C.c_int64),
        ("gate_batch_stride", C.c_int64), ("out_batch_stride", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("Nq", C.c_int32), ("Nk", C.c_int32),
        ("kv_len", C.c_void_p), ("q_len", C.c_void_p),
        ("scale", C.c_float), ("softclamp", C.c_float), ("dtype", C.c_int32), ("out_split", C.c_int32),
    ]


class XattnPrepareArgs(C.Structure):
    """Mirror of `v2a_xattn_prepare_args`."""
    _fields_ = [("ctx_kv", C.c_void_p), ("ctx_ld", C.c_int64), ("k_col", C.c_int32), ("v_col", C.c_int32),
                ("wq", C.c_void_p), ("wo", C.c_void_p), ("wqk", C.c_void_p), ("wvo", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("B", "L", "H", "D", "nc", "KP")]


class XattnAbsorbedArgs(C.Structure):
    """Mirror of `v2a_xattn_absorbed_args`."""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int64), ("K", C.c_int32), ("M", C.c_int32),
                ("wqk", C.c_void_p), ("ldw", C.c_int64), ("w_batch_stride", C.c_int64), ("gate_bias", C.c_void_p),
                ("out", C.c_void_p), ("ldo", C.c_int64),
                ("rows_per_batch", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("KP", C.c_int32),
                ("kv_len", C.c_void_p), ("q_len", C.c_void_p), ("scale", C.c_float), ("softclamp", C.c_float),
                ("row_ssq", C.c_void_p), ("ld_row_ssq", C.c_int64), ("row_ssq_parts", C.c_int32), ("row_norm_dim", C.c_int32)]


class YPlanes(C.Structure):
    """Mirror of `v2a_y_planes`: where v2a_cfg_euler_planes stores the operand planes of the updated y."""
    _fields_ = [("planes", C.c_void_p), ("ld", C.c_int64), ("lo_offset", C.c_int64), ("row_off", C.c_int32), ("rows_per_seq", C.c_int32),
                ("copies", C.c_int32), ("reserved", C.c_int32)]


class StepSeam(C.Structure):
    """Mirror of `v2a_step_seam`: what v2a_gemm_cfg_euler needs besides the to_pred GEMM's own arguments."""
    _fields_ = [("y", C.c_void_p), ("dt", C.c_void_p), ("step", C.c_void_p), ("arrive", C.c_void_p), ("planes", C.c_void_p), ("ld", C.c_int64),
                ("lo_offset", C.c_int64), ("B", C.c_int32), ("T", C.c_int32), ("row_off", C.c_int32), ("rows_per_seq", C.c_int32),
                ("cfg_strength", C.c_float), ("reserved", C.c_int32)]


class T5AttnArgs(C.Structure):
    """Mirror of `v2a_t5_attn_args`."""
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
        ("q_row_stride", C.c_int64), ("k_row_stride", C.c_int64), ("v_row_stride", C.c_int64), ("out_row_stride", C.c_int64),
        ("q_batch_stride", C.c_int64), ("k_batch_stride", C.c_int64), ("v_batch_stride", C.c_int64), ("out_batch_stride", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("d_kv", C.c_int32),
        ("bias", C.c_void_p), ("key_mask", C.c_void_p),
    ]


class ClipAttnArgs(C.Structure):
    """Mirror of `v2a_clip_attn_args`."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
                ("row_stride", C.c_int64), ("batch_stride", C.c_int64), ("out_row_stride", C.c_int64), ("out_batch_stride", C.c_int64),
                ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("d_head", C.c_int32), ("scale", C.c_float), ("out_split", C.c_int32)]


class RollHeadArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("x2", "x3", "x4", "x5")] + [("B", C.c_int32), ("P", C.c_int32)] +
                [(f"frb{i}_{n}", C.c_void_p) for i in (4, 3, 2) for n in ("w1t", "b1", "w2t", "b2")] +
                [(n, C.c_void_p) for n in ("conv2_wt", "conv2_b", "fc_wt", "fc_b")] +
                [("notes", C.c_int32), ("apply_sigmoid", C.c_int32), ("out", C.c_void_p)])


EXPORTS = [
    "v2a_abi_version", "v2a_last_error", "v2a_gemm", "v2a_gemm_args_size", "v2a_gemm_choose", "v2a_set_tuning", "v2a_rmsnorm", "v2a_dwconv_silu_residual", "v2a_dwconv_silu_residual_norm",
    "v2a_rope_inplace", "v2a_attention", "v2a_qproj_xattn", "v2a_linear_small", "v2a_fill_registers", "v2a_time_cond",
    "v2a_apg_reduce", "v2a_cfg_euler", "v2a_step_advance", "v2a_cast_bf16", "v2a_split_bf16",
    "v2a_im2col", "v2a_frames_pack", "v2a_pool2d", "v2a_roll_head", "v2a_roll_expand", "v2a_frames_pack_split", "v2a_pool2d_split",
    "v2a_elu_pad", "v2a_lstm_layer", "v2a_lstm2", "v2a_t5_rmsnorm", "v2a_t5_attention", "v2a_gemm_skinny_f32",
    "v2a_clip_resize_h", "v2a_clip_resize_v", "v2a_clip_embed_init", "v2a_clip_layernorm", "v2a_clip_attention",
    "v2a_elu_pad_lr", "v2a_encodec_stage0", "v2a_piano_resize_h", "v2a_piano_resize_v",
    "v2a_encodec_rvq_encode", "v2a_encodec_rvq_decode", "v2a_cfm_interp", "v2a_masked_sqerr", "v2a_roll_metrics",
    "v2a_wave_resample", "v2a_wave_stats", "v2a_wave_normalize",
    "v2a_roll2midi_stem", "v2a_leaky_shadow", "v2a_roll2midi_head", "v2a_roll2midi_gate",
    "v2a_xattn_absorb_prepare", "v2a_xattn_absorbed",
    "v2a_roll_expand_ratio", "v2a_piano_resize_vt",
    "v2a_roll_notes",
    "v2a_cfg_euler_planes", "v2a_gemm_cfg_euler",
    "v2a_mel_pad", "v2a_mel_from_dft",
    "v2a_vocos_stage_in", "v2a_vocos_dwconv_ln", "v2a_vocos_gelu", "v2a_vocos_scale_residual", "v2a_vocos_spectrum", "v2a_vocos_overlap_add",
    "v2a_convnext_dwconv", "v2a_convnext_pool_ln",
    "v2a_hifigan_act_pad", "v2a_hifigan_post", "v2a_hifigan_conv",
    "v2a_vae_stage_in", "v2a_vae_gn_stats", "v2a_vae_gn_act_pad", "v2a_vae_upsample_pad", "v2a_vae_softmax", "v2a_vae_conv_out",
]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libv2a_cfm.so (cross-compiles without a GPU)."""
    if force:
        for f in os.listdir(os.path.join(CSRC, "build")) if os.path.isdir(os.path.join(CSRC, "build")) else []:
            os.remove(os.path.join(CSRC, "build", f))
    r = subprocess.run(["bash", os.path.join(CSRC, "build.sh")], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-8000:])
    if r.returncode != 0:
        raise V2AError("hipcc build of libv2a_cfm.so failed")
    return LIB_PATH


ABI_VERSION = 9          # what v2a_abi_version() of this source tree returns (csrc/rowops.hip)


def _declare(lib):
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.v2a_abi_version.restype = C.c_int
    lib.v2a_last_error.restype = C.c_char_p
    lib.v2a_gemm.argtypes = [C.POINTER(GemmArgs), vp]
    lib.v2a_gemm_args_size.restype = C.c_int
    lib.v2a_gemm_choose.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmChoice)]
    lib.v2a_set_tuning.argtypes = [C.POINTER(Tuning)]
    lib.v2a_attention.argtypes = [C.POINTER(AttnArgs), vp]
    lib.v2a_qproj_xattn.argtypes = [C.POINTER(GemmArgs), C.POINTER(AttnArgs), vp]
    lib.v2a_xattn_absorb_prepare.argtypes = [C.POINTER(XattnPrepareArgs), vp]
    lib.v2a_xattn_absorbed.argtypes = [C.POINTER(XattnAbsorbedArgs), vp]
    lib.v2a_rmsnorm.argtypes = [vp, i64, vp, i64, i32, i64, i32, vp, vp, i64, i64, i32, vp]
    lib.v2a_dwconv_silu_residual.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.v2a_dwconv_silu_residual_norm.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, C.POINTER(DwconvNorm), vp]
    lib.v2a_rope_inplace.argtypes = [vp, i32, i64, i64, i32, i32, i32, vp, i32, vp]
    lib.v2a_linear_small.argtypes = [vp, i64, i32, vp, vp, vp, i32, vp, i64, i32, i32, i32, vp, vp, vp]
    lib.v2a_fill_registers.argtypes = [vp, i64, vp, i32, i32, i32, vp]
    lib.v2a_time_cond.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp]
    lib.v2a_apg_reduce.argtypes = [vp, vp, i32, i32, i32, i64, i32, vp, vp]
    lib.v2a_cfg_euler.argtypes = [vp, vp, i32, i32, i32, i64, i32, f32, vp, vp, vp, f32, vp]
    lib.v2a_cfg_euler_planes.argtypes = [vp, vp, i32, i32, i32, i64, i32, f32, vp, vp, vp, f32, C.POINTER(YPlanes), vp]
    lib.v2a_step_advance.argtypes = [vp, vp]
    lib.v2a_gemm_cfg_euler.argtypes = [C.POINTER(GemmArgs), C.POINTER(StepSeam), vp]
    lib.v2a_cast_bf16.argtypes = [vp, vp, i64, vp]
    lib.v2a_split_bf16.argtypes = [vp, i64, vp, i64, i64, i32, vp]
    lib.v2a_im2col.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i64, i32, i32, i32, vp]
    lib.v2a_frames_pack.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.v2a_pool2d.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.v2a_frames_pack_split.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.v2a_pool2d_split.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.v2a_roll_head.argtypes = [C.POINTER(RollHeadArgs), vp]
    lib.v2a_roll_expand.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.v2a_roll_expand_ratio.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.v2a_elu_pad.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp]
    lib.v2a_lstm_layer.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.v2a_lstm2.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.v2a_t5_rmsnorm.argtypes = [vp, i64, vp, i32, vp, i64, vp, i64, i64, i32, vp, f32, vp]
    lib.v2a_t5_attention.argtypes = [C.POINTER(T5AttnArgs), vp]
    lib.v2a_gemm_skinny_f32.argtypes = [C.POINTER(GemmArgs), vp]
    lib.v2a_clip_resize_h.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, i32, vp]
    lib.v2a_clip_resize_v.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, i32, i64, vp, vp]
    lib.v2a_clip_embed_init.argtypes = [vp, i64, i64, i32, i32, vp, vp, vp]
    lib.v2a_clip_layernorm.argtypes = [vp, i64, vp, i64, i32, i64, i32, vp, vp, f32, vp]
    lib.v2a_clip_attention.argtypes = [C.POINTER(ClipAttnArgs), vp]
    lib.v2a_elu_pad_lr.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp]
    lib.v2a_encodec_stage0.argtypes = [vp, vp, vp, i64, vp]
    lib.v2a_piano_resize_h.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.v2a_piano_resize_v.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp]
    lib.v2a_piano_resize_vt.argtypes = lib.v2a_piano_resize_v.argtypes
    lib.v2a_encodec_rvq_encode.argtypes = [vp, i64, i64, i64, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.v2a_encodec_rvq_decode.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, i64, i64, i64, vp]
    lib.v2a_cfm_interp.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.v2a_masked_sqerr.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.v2a_roll_metrics.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.v2a_wave_resample.argtypes = [vp, i64, vp, i32, i32, i32, i32, vp, i64, vp, C.POINTER(i32), vp]
    lib.v2a_wave_stats.argtypes = [vp, i64, vp, C.POINTER(i32), vp]
    lib.v2a_wave_normalize.argtypes = [vp, i64, vp, i32, vp, i64, vp, vp]
    lib.v2a_roll2midi_stem.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, i64, i64, i32, vp]
    lib.v2a_leaky_shadow.argtypes = [vp, vp, i32, i64, i32, i32, i32, i32, i64, i32, vp]
    lib.v2a_roll2midi_head.argtypes = [vp, i64, i32, vp, i64, i32, vp, f32, f32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.v2a_roll2midi_gate.argtypes = [vp, i64, i32, vp, i64, vp, i64, i32, vp, i64, vp, f32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.v2a_roll_notes.argtypes = [vp, i32, i64, i64, i64, f32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.v2a_mel_pad.argtypes = [vp, i64, i32, i64, i32, vp, i64, vp]
    lib.v2a_mel_from_dft.argtypes = [vp, i64, i64, i32, i64, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, f32, vp, i64, i64, vp]
    lib.v2a_vocos_stage_in.argtypes = [vp, i64, i64, i32, i32, i32, vp, vp, i32, vp]
    lib.v2a_vocos_dwconv_ln.argtypes = [vp, i64, vp, vp, vp, vp, f32, i32, i32, i64, i32, vp, vp, i64, vp]
    lib.v2a_vocos_gelu.argtypes = [vp, i64, i64, i32, vp]
    lib.v2a_vocos_scale_residual.argtypes = [vp, i64, vp, vp, i64, vp, i64, i64, i32, vp]
    lib.v2a_vocos_spectrum.argtypes = [vp, i64, i64, i32, vp, i64, vp]
    lib.v2a_vocos_overlap_add.argtypes = [vp, i64, i64, vp, i32, i32, i32, i32, vp, vp, i64, vp]
    lib.v2a_convnext_dwconv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.v2a_convnext_pool_ln.argtypes = [vp, i64, i32, i32, i32, vp, vp, f32, vp, i64, vp]
    lib.v2a_hifigan_act_pad.argtypes = [vp, vp, vp, i64, i64, i32, i32, i32, vp, f32, f32, vp, i64, i32, vp]
    lib.v2a_hifigan_post.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.v2a_hifigan_conv.argtypes = [vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, i32, f32, vp, i64, vp, i64, vp]
    lib.v2a_vae_stage_in.argtypes = [vp, i64, i64, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, i32, i64, vp]
    lib.v2a_vae_gn_stats.argtypes = [vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.v2a_vae_gn_act_pad.argtypes = [vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, C.c_double, i32, vp, i64, i32, vp]
    lib.v2a_vae_upsample_pad.argtypes = [vp, i64, i32, i32, i32, i32, i32, vp, vp, i64, vp]
    lib.v2a_vae_softmax.argtypes = [vp, i64, i32, i32, f32, vp]
    lib.v2a_vae_conv_out.argtypes = [vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    for name in EXPORTS:
        if name not in ("v2a_abi_version", "v2a_last_error", "v2a_gemm_args_size"):
            getattr(lib, name).restype = C.c_int


def lib():
    """The loaded library; raises loudly if it was never built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise V2AError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the sampler.")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
        if _lib.v2a_abi_version() != ABI_VERSION:
            raise V2AError("libv2a_cfm.so reports ABI version %d, this binding was written for %d: rebuild (csrc/build.sh)"
                           % (_lib.v2a_abi_version(), ABI_VERSION))
        if _lib.v2a_gemm_args_size() != C.sizeof(GemmArgs):
            raise V2AError("libv2a_cfm.so was built with sizeof(v2a_gemm_args) = %d, this binding mirrors %d bytes: rebuild "
                           "(csrc/build.sh)" % (_lib.v2a_gemm_args_size(), C.sizeof(GemmArgs)))
    return _lib


def set_tuning(force_tile: int = -1, k_rotation: bool = False, eight_phase: int | None = None, eight_phase_min_tiles: int = 0,
               dwconv_rows_per_wave: int = 0, xcd_order_1x8: bool = False, attn_one_group_from: int = 0, reserved: int = 0):
    """Tile-selection overrides (A/B measurements); `set_tuning()` restores the library defaults.  `reserved`: probe builds only."""
    if (force_tile == -1 and not k_rotation and eight_phase is None and eight_phase_min_tiles == 0 and dwconv_rows_per_wave == 0
            and not xcd_order_1x8 and attn_one_group_from == 0 and not reserved):
        check(lib().v2a_set_tuning(None))
        return
    t = Tuning(force_tile, 1 if k_rotation else 0, 1 if eight_phase is None else eight_phase, eight_phase_min_tiles, dwconv_rows_per_wave,
               1 if xcd_order_1x8 else 0, attn_one_group_from, (C.c_int32 * 1)(reserved))
    check(lib().v2a_set_tuning(C.byref(t)))


def check(rc: int):
    if rc != 0:
        raise V2AError(f"v2a_cfm call failed ({rc}): {lib().v2a_last_error().decode()}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def dt_code(t: torch.dtype) -> int:
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise V2AError(f"unsupported dtype {t}")


def _p(t):
    return 0 if t is None else t.data_ptr()


class Operand(NamedTuple):
    """A GEMM A segment, or the destination of a bf16 shadow: `t` is the view at the hi plane of row 0, `ld` the row stride in
    elements, `k` the logical K (columns), `lo` the distance from a row's hi plane to its lo plane in the split layout (0: k,
    as in the C ABI).  gemm() takes these wherever it takes (t, lda, k[, lo]) tuples."""
    t: torch.Tensor
    ld: int
    k: int
    lo: int = 0


def split_planes(w):
    """fp32 rows -> [hi | lo] bf16 rows (V2A_BF16_SPLIT): hi = bf16(w), lo = bf16(w - hi)."""
    w = w.float()
    hi = w.bfloat16()
    return torch.cat([hi, (w - hi.float()).bfloat16()], 1)


# ---- optional per-launch timing (bench.py roofline leg): HIP events on the launch stream ----
_prof = None


class KernelProfiler:
    """Per-launch timing of the C-ABI calls with HIP events on the stream the kernel is launched on (torch's current
    stream), aggregated by kernel instantiation.

    external=False : eager -- every launch sits between its own pair of events (`inner` back-to-back launches per pair for
                     GEMMs amortise the ~5 us dispatch gap an eager pair includes, at the price of warm caches).
    external=True  : for use under hipGraph capture -- ONE external event is recorded in front of every launch (an event
                     record node of the graph) and one after the last; after each replay `collect()` adds the interval to
                     the next mark to the launch's total.  Intervals are kernel time + the launch boundary behind it, with
                     every kernel launched exactly once per evaluation in its real cache state."""

    def __init__(self, shapes: bool = False, inner: int = 1, external: bool = False):
        self.recs = []
        self.shapes = shapes      # key GEMM launches by MxNxK as well
        self.inner = inner
        self.external = external
        self.marks, self.end, self.tot = [], None, {}

    def launch(self, key, flops, nbytes, call):
        if self.external:
            e = torch.cuda.Event(enable_timing=True, external=True)
            e.record()
            self.marks.append((key, flops, nbytes, e))
            call()
            return
        n = self.inner if key.startswith("gemm") else 1
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            call()
        e.record()
        self.recs.append((key, flops, nbytes, s, e, n))

    def close(self):
        """external mode: the mark behind the last launch (call inside the capture)."""
        self.end = torch.cuda.Event(enable_timing=True, external=True)
        self.end.record()

    def collect(self):
        """external mode: after a replay has completed, add this replay's intervals."""
        for i, (key, flops, nbytes, e) in enumerate(self.marks):
            nxt = self.marks[i + 1][3] if i + 1 < len(self.marks) else self.end
            a = self.tot.setdefault(key, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            a["launches"] += 1
            a["ms"] += e.elapsed_time(nxt)
            a["flops"] += flops
            a["bytes"] += nbytes

    def summary(self):
        torch.cuda.synchronize()
        if self.external:
            return self.tot
        agg = {}
        for key, flops, nbytes, s, e, n in self.recs:
            a = agg.setdefault(key, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            a["launches"] += 1
            a["ms"] += s.elapsed_time(e) / n
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


def set_profiler(p):
    global _prof
    _prof = p


def _launch(key, flops, nbytes, call):
    if _prof is None:
        check(call())
    else:
        _prof.launch(key, flops, nbytes, lambda: check(call()))


_EPI_NAMES = {0: "store", 1: "sigmoid", 2: "geglu", 3: "resid", 4: "gate_resid", 5: "geglu_tanh", 6: "gelu", 7: "swiglu", 9: "quick_gelu"}


# ------------------------------------------------------------------------------------------
# thin typed wrappers (torch tensors are only carriers of device pointers here)
# ------------------------------------------------------------------------------------------

def gemm(a_segs, w, out, **kw):
    """One v2a_gemm launch; arguments as for gemm_args."""
    g, key, flops, nbytes = gemm_args(a_segs, w, out, **kw)
    _launch(key, flops, nbytes, lambda: lib().v2a_gemm(C.byref(g), stream_ptr()))


def gemm_choice(a_segs, w, out, **kw) -> GemmChoice:
    """What gemm() with the same arguments would launch under the current tuning (v2a_gemm_choose): nothing is launched or read, so
    tensors on any device do; a refusal raises as gemm() would."""
    c = GemmChoice()
    check(lib().v2a_gemm_choose(C.byref(gemm_args(a_segs, w, out, **kw)[0]), C.byref(c)))
    return c


def gemm_args(a_segs, w, out, *, M, N, compute, epilogue=EPI_STORE, bias=None, resid=None, gate=None,
         step=None, gate_step_stride=0, gate_batch_stride=0, rows_per_batch=0, ldo=None, ldr=None,
         out_bf16=None, ld_out_bf16=None, rope_table=None, rope_cols=0, rope_pos_offset=0, relu=False,
         a_row_offset=None, a_ktile_offset=None, out_row_offset=None, tile_hint=0,
         norm_gamma=None, norm_step_stride=0, norm_batch_stride=0, norm_switch_row=0, norm_switch_offset=0, norm_ssq=None,
         row_ssq=None, row_norm_dim=0, out_bf16_split=False, a_split=False, out_split=False, out_bf16_lo_offset=0):
    """a_segs: list of Operand records or (tensor, lda, k[, lo]) tuples.  w: [N][K] tensor in the compute dtype.
    a_split: the segments are V2A_BF16_SPLIT rows ([hi k | lo k], lda >= 2k, or the lo plane `lo` elements after the hi one:
    v2a_gemm_args.a_lo_offset) and w is [N][2K] = [W_hi | W_lo] (the bf16x3 mode's native
    GEMM: three MFMA products per fp32 product); out_split: GEGLU output as hi | lo planes; out_bf16_split: the shadow likewise.
    Folded RMSNorm (v2a_gemm_args): producer -- norm_gamma (+ strides / switch) scales the out_bf16 shadow, norm_ssq (rows, N/32)
    receives the sums of squares; consumer -- row_ssq (rows, parts) of its A rows and row_norm_dim = their width."""
    g = GemmArgs()
    a_segs = [Operand(*seg) for seg in a_segs]
    for i, s in enumerate(a_segs):
        g.a[i], g.lda[i], g.ka[i], g.a_lo_offset[i] = s.t.data_ptr(), s.ld, s.k, s.lo
    g.nseg = len(a_segs)
    g.a_dtype = BF16_SPLIT if a_split else dt_code(a_segs[0].t.dtype)
    g.w = w.data_ptr()
    g.ldw = w.stride(0)
    g.bias = _p(bias)
    g.M, g.N = M, N
    g.compute_dtype = compute
    g.epilogue = epilogue
    g.out = out.data_ptr()
    g.ldo = ldo if ldo is not None else out.stride(-2)
    g.out_dtype = BF16_SPLIT if out_split else dt_code(out.dtype)
    g.out_bf16 = _p(out_bf16)
    g.ld_out_bf16 = (ld_out_bf16 if ld_out_bf16 is not None else g.ldo) if out_bf16 is not None else 0
    g.resid = _p(resid)
    g.ldr = (ldr if ldr is not None else (resid.stride(-2) if resid is not None else 0))
    g.gate = _p(gate)
    g.step = _p(step)
    g.gate_step_stride = gate_step_stride
    g.gate_batch_stride = gate_batch_stride
    g.rows_per_batch = rows_per_batch
    g.rope_table = _p(rope_table)
    g.rope_cols, g.rope_pos_offset = rope_cols, rope_pos_offset
    g.relu = 1 if relu else 0
    g.a_row_offset, g.a_ktile_offset, g.out_row_offset = _p(a_row_offset), _p(a_ktile_offset), _p(out_row_offset)
    g.tile_hint = tile_hint if compute == BF16 and g.a_dtype in (BF16, BF16_SPLIT) and epilogue != EPI_SIGMOID else 0
    g.norm_gamma = _p(norm_gamma)
    g.norm_step_stride, g.norm_batch_stride = norm_step_stride, norm_batch_stride
    g.norm_switch_row, g.norm_switch_offset = norm_switch_row, norm_switch_offset
    g.norm_ssq = _p(norm_ssq)
    g.ld_norm_ssq = norm_ssq.stride(-2) if norm_ssq is not None else 0
    g.row_ssq = _p(row_ssq)
    g.ld_row_ssq = row_ssq.stride(-2) if row_ssq is not None else 0
    g.row_ssq_parts = row_norm_dim // 32 if row_ssq is not None else 0
    g.row_norm_dim = row_norm_dim
    g.out_bf16_split = 1 if out_bf16_split else 0
    g.out_bf16_lo_offset = out_bf16_lo_offset
    K = sum(s.k for s in a_segs)
    key = "gemm<%s,%s,%s,%s>" % ("bf16" if compute == BF16 else "f32", "a_f32" if g.a_dtype == F32 else ("a_split" if a_split else "a_bf16"),
                                 _EPI_NAMES[epilogue], "f32" if g.out_dtype == F32 else "bf16")
    esz = 2 if compute == BF16 else 4
    nbytes = M * K * (4 if g.a_dtype == F32 else 2) + N * K * esz + M * (N // 2 if epilogue in (EPI_GEGLU, EPI_SWIGLU) else N) * out.element_size()
    nbytes += (M * N * 4 if resid is not None else 0) + (M * N * 2 if out_bf16 is not None else 0)      # residual rows read, bf16 shadow written
    if g.tile_hint:
        key = key[:-1] + ",tile%d>" % (g.tile_hint - 1)        # side-stream launches: tile shape chosen for running beside others
    if _prof is not None and _prof.shapes:
        key += " %dx%dx%d" % (M, N, K)
    return g, key, (6.0 if a_split else 2.0) * M * N * K, nbytes * (2 if a_split else 1)


def rmsnorm(x, y, *, rows, d, gamma, step=None, gamma_step_stride=0, gamma_batch_stride=0, rows_per_batch=0,
            ldx=None, ldy=None, split=False):
    """split=True: y is a (rows, 2*d) bf16 buffer that receives the hi | lo planes (BF16_SPLIT)."""
    ydt = BF16_SPLIT if split else dt_code(y.dtype)
    if split:
        ldy = ldy or 2 * d
    _launch("rmsnorm<%s>" % ("f32" if y.dtype == torch.float32 else ("bf16x2" if split else "bf16")), 0.0,
            rows * d * (4 + y.element_size() * (2 if split else 1)),
            lambda: lib().v2a_rmsnorm(x.data_ptr(), ldx or d, y.data_ptr(), ldy or d, ydt, rows, d,
                                      gamma.data_ptr(), _p(step), gamma_step_stride, gamma_batch_stride, rows_per_batch,
                                      stream_ptr()))


def _dwconv_norm(norm, d):
    n = DwconvNorm()
    n.out_bf16, n.ld_out_bf16 = norm["out_bf16"].data_ptr(), norm.get("ld_out_bf16", d)
    n.norm_gamma, n.step = norm["gamma"].data_ptr(), _p(norm.get("step"))
    n.norm_step_stride, n.norm_batch_stride = norm.get("step_stride", 0), norm.get("batch_stride", 0)
    n.norm_ssq, n.ld_norm_ssq = norm["ssq"].data_ptr(), norm["ssq"].stride(-2)
    n.split = 1 if norm.get("split") else 0
    if n.split:
        n.ld_out_bf16 = norm.get("ld_out_bf16", 2 * d)
    return n


def dwconv(x, out, wt, bias, *, B, N, d, ksize, lens=None, norm=None):
    """norm = dict(out_bf16, gamma, ssq, step=None, step_stride=0, batch_stride=0): the RMSNorm after the conv folded in."""
    if norm is None:
        _launch("dwconv", 2.0 * B * N * d * ksize, B * N * d * 8,
                lambda: lib().v2a_dwconv_silu_residual(x.data_ptr(), out.data_ptr(), wt.data_ptr(), bias.data_ptr(),
                                                       B, N, d, ksize, _p(lens), stream_ptr()))
        return
    n = _dwconv_norm(norm, d)
    # x read + out written (fp32) + the normalised bf16 copy: one plane, or hi | lo planes in the split mode
    _launch("dwconv+norm", 2.0 * B * N * d * ksize, B * N * d * (12 if n.split else 10),
            lambda: lib().v2a_dwconv_silu_residual_norm(x.data_ptr(), out.data_ptr(), wt.data_ptr(), bias.data_ptr(),
                                                        B, N, d, ksize, _p(lens), C.byref(n), stream_ptr()))


def rope(qk, *, rows, row_stride, nheads, rows_per_batch, pos_offset, table, layout):
    _launch("rope<%s>" % ("f32" if qk.dtype == torch.float32 else "bf16"), 0.0, rows * nheads * 64 * 2 * qk.element_size(),
            lambda: lib().v2a_rope_inplace(qk.data_ptr(), dt_code(qk.dtype), rows, row_stride, nheads, rows_per_batch,
                                           pos_offset, table.data_ptr(), layout, stream_ptr()))


def attention(q, k, v, gate, out, **kw):
    """q,k,v,gate,out: integer device addresses (views into fused buffers); one v2a_attention launch."""
    a, key, flops, nbytes = attention_args(q, k, v, gate, out, **kw)
    _launch(key, flops, nbytes, lambda: lib().v2a_attention(C.byref(a), stream_ptr()))


def attention_args(q, k, v, gate, out, *, strides, B, H, Nq, Nk, kv_len=None, q_len=None, scale, softclamp, dtype, out_split=False):
    a = AttnArgs()
    a.q, a.k, a.v, a.gate, a.out = q, k, v, gate, out
    (a.q_row_stride, a.k_row_stride, a.v_row_stride, a.gate_row_stride, a.out_row_stride,
     a.q_batch_stride, a.k_batch_stride, a.v_batch_stride, a.gate_batch_stride, a.out_batch_stride) = strides
    a.B, a.H, a.Nq, a.Nk = B, H, Nq, Nk
    a.kv_len, a.q_len = _p(kv_len), _p(q_len)
    a.scale, a.softclamp, a.dtype = scale, softclamp, dtype
    a.out_split = 1 if out_split else 0
    esz = 2 if dtype == BF16 else 4
    return a, "attention<%s>" % {BF16: "bf16", F32: "f32", BF16_SPLIT: "bf16x3"}[dtype], 4.0 * B * H * Nq * Nk * 64, B * H * 64 * (2 * Nq + 2 * Nk) * esz


def qproj_xattn(a, lda, K, w, *, bias, M, N, rows_per_batch, k, v, out, kv_strides, out_strides, B, H, Nk, kv_len=None, q_len=None,
                scale, softclamp, rope_table=None, rope_cols=0, rope_pos_offset=0, row_ssq=None, row_norm_dim=0, split=False):
    """q-projection + cross-attention in one launch (v2a_qproj_xattn).  a: (M, K) bf16 rows; w: [N >= H*65][K] = to_q rows then the
    gate rows; k, v, out: integer device addresses; kv_strides = (k_row, v_row, k_batch, v_batch), out_strides = (row, batch).
    split=True (bf16x3 mode): a rows = [hi K | lo K], w rows = [W_hi | W_lo], k / v fp32, out rows = hi | lo planes (2 * H * 64 bf16)."""
    g = GemmArgs()
    g.a[0], g.lda[0], g.ka[0], g.nseg = a.data_ptr(), lda, K, 1
    g.compute_dtype = BF16
    g.a_dtype = BF16_SPLIT if split else BF16
    g.w, g.ldw = w.data_ptr(), w.stride(0)
    g.bias = _p(bias)
    g.M, g.N = M, N
    g.epilogue = EPI_STORE
    g.out_dtype = F32 if split else BF16
    g.rows_per_batch = rows_per_batch
    g.rope_table = _p(rope_table)
    g.rope_cols, g.rope_pos_offset = rope_cols, rope_pos_offset
    g.row_ssq = _p(row_ssq)
    g.ld_row_ssq = row_ssq.stride(-2) if row_ssq is not None else 0
    g.row_ssq_parts = row_norm_dim // 32 if row_ssq is not None else 0
    g.row_norm_dim = row_norm_dim
    t = AttnArgs()
    t.k, t.v, t.out = k, v, out
    t.k_row_stride, t.v_row_stride, t.k_batch_stride, t.v_batch_stride = kv_strides
    t.out_row_stride, t.out_batch_stride = out_strides
    t.B, t.H, t.Nq, t.Nk = B, H, rows_per_batch, Nk
    t.kv_len, t.q_len = _p(kv_len), _p(q_len)
    t.scale, t.softclamp, t.dtype = scale, softclamp, (BF16_SPLIT if split else BF16)
    t.out_split = 1 if split else 0
    _launch("qproj_xattn<%s>" % ("bf16x3" if split else "bf16"), (3.0 if split else 1.0) * (2.0 * M * (H * 65) * K + 4.0 * B * H * rows_per_batch * Nk * 64),
            M * K * 2 + H * 65 * K * 2 + M * H * 64 * 2 + 2 * B * Nk * H * 64 * 2,
            lambda: lib().v2a_qproj_xattn(C.byref(g), C.byref(t), stream_ptr()))


def xattn_kp(nc):
    """Key slots per head of the absorbed cross-attention: 16 up to 16 context tokens, 32 up to 32."""
    return 16 if nc <= 16 else 32


def xattn_absorb_prepare(ctx_kv, wq, wo, wqk, wvo, *, B, L, H, D, nc, KP, k_col, v_col):
    """Absorbed cross-attention operands of every (clip, layer), once per sample() (v2a_xattn_absorb_prepare).  ctx_kv: fp32 (B*nc, ld)
    context K / V rows, K of layer l at columns k_col + l*H*64, V at v_col + l*H*64; wq: fp32 [L][H*64 + H][D] (to_q rows, gate rows);
    wo: fp32 [L][D][H*64]; wqk: bf16 [B][L][H*KP + H][2 D]; wvo: bf16 [B][L][D][2 H*KP] (hi | lo planes)."""
    a = XattnPrepareArgs()
    a.ctx_kv, a.ctx_ld, a.k_col, a.v_col = ctx_kv.data_ptr(), ctx_kv.stride(-2), k_col, v_col
    a.wq, a.wo, a.wqk, a.wvo = wq.data_ptr(), wo.data_ptr(), wqk.data_ptr(), wvo.data_ptr()
    a.B, a.L, a.H, a.D, a.nc, a.KP = B, L, H, D, nc, KP
    _launch("xattn_absorb_prepare", 4.0 * B * L * H * KP * 64 * D,
            L * (2 * H * 64 + H) * D * 4 + B * L * ((H * KP + H) * D + D * H * KP) * 4 + 2 * B * nc * L * H * 64 * 4,
            lambda: lib().v2a_xattn_absorb_prepare(C.byref(a), stream_ptr()))


def xattn_absorbed(a, lda, K, wqk, out, *, ldw, w_batch_stride, ldo, M, rows_per_batch, B, H, KP, kv_len, q_len=None, gate_bias=None,
                   scale, softclamp, row_ssq=None, row_norm_dim=0):
    """Logits, softmax and head gate of the absorbed cross-attention in one launch (v2a_xattn_absorbed).  a: (M, [hi K | lo K]) bf16
    rows; wqk: bf16 [B][H*KP + H][2 K] of the clips (w_batch_stride elements apart); out: (M, [hi H*KP | lo H*KP]) bf16 rows."""
    g = XattnAbsorbedArgs()
    g.a, g.lda, g.K, g.M = a.data_ptr(), lda, K, M
    g.wqk, g.ldw, g.w_batch_stride, g.gate_bias = wqk.data_ptr(), ldw, w_batch_stride, _p(gate_bias)
    g.out, g.ldo = out.data_ptr(), ldo
    g.rows_per_batch, g.B, g.H, g.KP = rows_per_batch, B, H, KP
    g.kv_len, g.q_len = _p(kv_len), _p(q_len)
    g.scale, g.softclamp = scale, softclamp
    g.row_ssq = _p(row_ssq)
    g.ld_row_ssq = row_ssq.stride(-2) if row_ssq is not None else 0
    g.row_ssq_parts = row_norm_dim // 32 if row_ssq is not None else 0
    g.row_norm_dim = row_norm_dim
    n = H * KP + H
    _launch("xattn_absorbed<bf16x3>", 6.0 * M * n * K, (M * K + B * n * K + M * H * KP) * 4,
            lambda: lib().v2a_xattn_absorbed(C.byref(g), stream_ptr()))


def linear_small(a, wt, bias, add, out, *, M, K, T, out_batch_stride, row_off, d, dup=0, regs=None, out_bf16=None):
    _launch("linear_small", 2.0 * M * K * d, M * (K + d) * 4,
            lambda: lib().v2a_linear_small(a.data_ptr(), M, K, wt.data_ptr(), _p(bias), _p(add), T, out.data_ptr(),
                                           out_batch_stride, row_off, d, dup, _p(regs), _p(out_bf16), stream_ptr()))


def fill_registers(out, regs, *, B, R, d, out_batch_stride):
    check(lib().v2a_fill_registers(out.data_ptr(), out_batch_stride, regs.data_ptr(), B, R, d, stream_ptr()))


def time_cond(t, fourier_w, wt, bias, out, *, S, d):
    check(lib().v2a_time_cond(t.data_ptr(), S, fourier_w.data_ptr(), wt.data_ptr(), bias.data_ptr(),
                              out.data_ptr(), d, stream_ptr()))


def apg_reduce(pred, apg, *, B, T, C_, pred_batch_stride, row_off, valid_rows=None):
    """valid_rows: device int32[1] or None: the rows of every clip that enter the sums (a bucketed plan pads T behind them)."""
    check(lib().v2a_apg_reduce(pred.data_ptr(), apg.data_ptr(), B, T, C_, pred_batch_stride, row_off, _p(valid_rows), stream_ptr()))


def cfg_euler(y, pred, *, B, T, C_, pred_batch_stride, row_off, cfg_strength, dt, step=None, apg=None, keep=0.0, planes=None):
    """planes = dict(out, ld, lo_offset, row_off, rows_per_seq, copies) or None: the hi | lo bf16 planes of the updated y as well, into
    rows [row_off, row_off + T) of every one of copies * B sequences of rows_per_seq rows of `out` (v2a_cfg_euler_planes)."""
    if planes is None:
        _launch("cfg_euler", 0.0, 16.0 * B * T * C_,
                lambda: lib().v2a_cfg_euler(y.data_ptr(), pred.data_ptr(), B, T, C_, pred_batch_stride, row_off,
                                            float(cfg_strength), dt.data_ptr(), _p(step), _p(apg), float(keep), stream_ptr()))
        return
    pl = YPlanes(planes["out"].data_ptr(), planes["ld"], planes["lo_offset"], planes["row_off"], planes["rows_per_seq"], planes["copies"], 0)
    _launch("cfg_euler", 0.0, (16.0 + 4.0 * planes["copies"]) * B * T * C_,
            lambda: lib().v2a_cfg_euler_planes(y.data_ptr(), pred.data_ptr(), B, T, C_, pred_batch_stride, row_off, float(cfg_strength),
                                               dt.data_ptr(), _p(step), _p(apg), float(keep), C.byref(pl), stream_ptr()))


def step_advance(step):
    check(lib().v2a_step_advance(step.data_ptr(), stream_ptr()))


def gemm_cfg_euler(a_segs, w, out, *, y, dt, step, arrive, planes, B, T, row_off, rows_per_seq, cfg_strength, **kw):
    """The step seam in one launch (v2a_gemm_cfg_euler): the to_pred GEMM (a_segs, w, out and kw as for gemm(); split operands, STORE), the
    CFG + Euler update of y (B, T, C) from the two halves of its rows, the hi | lo planes of the new y into both halves of planes =
    dict(out, ld, lo_offset), and the step counter advanced by the workgroup that arrives last at `arrive` (uint32 [1], zero between launches)."""
    g, key, flops, nbytes = gemm_args(a_segs, w, out, **kw)
    s = StepSeam(y.data_ptr(), dt.data_ptr(), step.data_ptr(), arrive.data_ptr(), planes["out"].data_ptr(), planes["ld"], planes["lo_offset"],
                 B, T, row_off, rows_per_seq, float(cfg_strength), 0)
    _launch(key.replace("store", "cfg_euler"), flops, nbytes + (8.0 + 8.0) * B * T * kw["N"],
            lambda: lib().v2a_gemm_cfg_euler(C.byref(g), C.byref(s), stream_ptr()))


def split_bf16(x, y, *, rows, d, ldx=None, ldy=None):
    """fp32 (rows, d) -> bf16 (rows, 2*d) hi | lo planes."""
    _launch("split_bf16", 0.0, rows * d * 8, lambda: lib().v2a_split_bf16(x.data_ptr(), ldx or d, y.data_ptr(), ldy or 2 * d, rows, d, stream_ptr()))


def cast_bf16(x, y):
    _launch("cast_bf16", 0.0, x.numel() * 6, lambda: lib().v2a_cast_bf16(x.data_ptr(), y.data_ptr(), x.numel(), stream_ptr()))


# ---- N2: Video2Roll frame encoder ----------------------------------------------------------------
def im2col(x, col, *, B, H, W, C_, kh, kw, stride, pad, Ho, Wo, ldo, window_t=0, window_first=0):
    K = kh * kw * C_
    _launch("im2col<%s>" % ("f32" if col.dtype == torch.float32 else "bf16"), 0.0, B * Ho * Wo * (4.0 * K + col.element_size() * ldo),
            lambda: lib().v2a_im2col(x.data_ptr(), B, H, W, C_, kh, kw, stride, pad, Ho, Wo, col.data_ptr(), ldo,
                                     dt_code(col.dtype), window_t, window_first, stream_ptr()))


def frames_pack(frames, out, *, T, H, W, kw, stride, pad, Wo):
    _launch("frames_pack", 0.0, 4.0 * T * H * W + 32.0 * (T + 4) * Wo * (H + 2 * pad),
            lambda: lib().v2a_frames_pack(frames.data_ptr(), out.data_ptr(), T, H, W, kw, stride, pad, Wo, stream_ptr()))


def frames_pack_split(frames, out, *, lo_offset, T, H, W, kw, stride, pad, Wo):
    """bf16x3 mode: the column patches of frames_pack as hi | lo planes, the lo plane lo_offset elements after the hi one."""
    _launch("frames_pack_split", 0.0, 4.0 * T * H * W + 64.0 * (T + 4) * Wo * (H + 2 * pad),
            lambda: lib().v2a_frames_pack_split(frames.data_ptr(), out.data_ptr(), lo_offset, T, H, W, kw, stride, pad, Wo, stream_ptr()))


def pool2d(x, out, *, B, H, W, C_, k, stride, pad, mode, Ho, Wo, out_bf16=None, in_border=0, out_border=0):
    _launch("pool2d", 0.0, 4.0 * B * C_ * (H * W + Ho * Wo),
            lambda: lib().v2a_pool2d(x.data_ptr(), out.data_ptr(), _p(out_bf16), B, H, W, C_, k, stride, pad, mode, Ho, Wo,
                                     in_border, out_border, stream_ptr()))


def pool2d_split(x, out, out_split, *, lo_offset, B, H, W, C_, k, stride, pad, mode, Ho, Wo, in_border=0, out_border=0):
    """bf16x3 mode: pool2d whose bf16 copy is written as hi | lo planes (out_split, the lo plane lo_offset elements further)."""
    _launch("pool2d_split", 0.0, 4.0 * B * C_ * (H * W + 2 * Ho * Wo),
            lambda: lib().v2a_pool2d_split(x.data_ptr(), out.data_ptr(), out_split.data_ptr(), lo_offset, B, H, W, C_, k, stride, pad,
                                           mode, Ho, Wo, in_border, out_border, stream_ptr()))


def roll_head(args: "RollHeadArgs"):
    _launch("roll_head", 0.0, 4.0 * args.B * args.P * (3 * 128 + 64), lambda: lib().v2a_roll_head(C.byref(args), stream_ptr()))


def roll_expand(roll, out, *, B, t, notes, rep, l):
    check(lib().v2a_roll_expand(roll.data_ptr(), out.data_ptr(), B, t, notes, rep, l, stream_ptr()))


def roll_expand_ratio(roll, out, *, B, t, notes, rep, group, l):
    """out (B, l, notes) <- rows of roll (B, t, notes) repeated `rep` times, every `group` (1 | 2) of them averaged, zero behind."""
    check(lib().v2a_roll_expand_ratio(roll.data_ptr(), out.data_ptr(), B, t, notes, rep, group, l, stream_ptr()))


# ---- Roll2Midi generator (roll2midi.py) ----------------------------------------------------------
SH_NONE, SH_BF16, SH_SPLIT = 0, 1, 2      # shadow modes of v2a_roll2midi_stem / v2a_leaky_shadow


def roll2midi_stem(x, wt, out, shadow, *, n, H, W, co, shadow_mode, lo_offset, pitch, border):
    """x (n, H, W) fp32 roll -> the co channels of down1 in the slice that starts at `out` (and its shadow at `shadow`)."""
    _launch("roll2midi_stem", 18.0 * n * H * W * co, n * H * W * (4.0 + co * (4 + 2 * shadow_mode)),
            lambda: lib().v2a_roll2midi_stem(x.data_ptr(), wt.data_ptr(), n, H, W, co, out.data_ptr(), _p(shadow), shadow_mode, lo_offset,
                                             pitch, border, stream_ptr()))


def leaky_shadow(x, shadow, *, n, H, W, C_, shadow_mode, lo_offset, pitch, border):
    """LeakyReLU(0.2) in place on the slice that starts at `x`, and the shadow of the result."""
    _launch("leaky_shadow", 0.0, n * H * W * C_ * (8.0 + 2 * shadow_mode),
            lambda: lib().v2a_leaky_shadow(x.data_ptr(), _p(shadow), shadow_mode, lo_offset, n, H, W, C_, pitch, border, stream_ptr()))


def roll2midi_head(u, d, w, *, u_pitch, nu, d_pitch, nd, bias, threshold, n, H, W, border, logits=None, probs=None, midi=None):
    _launch("roll2midi_head", 2.0 * n * H * W * (nu + nd), n * H * W * (4.0 * (nu + nd) + 9),
            lambda: lib().v2a_roll2midi_head(u.data_ptr(), u_pitch, nu, d.data_ptr(), d_pitch, nd, w.data_ptr(), float(bias), float(threshold),
                                             n, H, W, border, _p(logits), _p(probs), _p(midi), stream_ptr()))


def roll2midi_gate(seg0, seg1, w, *, bias, shadow_mode, n, H, W, border, logits=None, alpha=None):
    """The folded attention gate in place on one or two segments (x, pitch, C, shadow, lo_offset); seg1 None: one segment.  x and
    shadow start at the segment's first channel."""
    x0, p0, c0, s0, l0 = seg0
    x1, p1, c1, s1, l1 = seg1 if seg1 is not None else (None, 0, 0, None, 0)
    _launch("roll2midi_gate", 2.0 * n * H * W * (c0 + c1), n * H * W * (c0 + c1) * (8.0 + 2 * shadow_mode) + 4.0 * (c0 + c1),
            lambda: lib().v2a_roll2midi_gate(x0.data_ptr(), p0, c0, _p(s0), l0, _p(x1), p1, c1, _p(s1), l1, w.data_ptr(), float(bias),
                                             shadow_mode, n, H, W, border, _p(logits), _p(alpha), stream_ptr()))


# ---- note extraction behind Roll2Midi (midi.py) --------------------------------------------------
ROLL_NOTES_MAX_KEYS, ROLL_NOTES_TILE, ROLL_NOTES_MAX_FRAMES = 128, 256, 1 << 24      # V2A_ROLL_NOTES_* of include/v2a_cfm.h


def roll_notes(roll, counts, totals, notes, *, strides, B, T, keys, cap, threshold=0.0, lens=None, onset=None):
    """One v2a_roll_notes launch.  roll: uint8 or fp32 tensor read at b * strides[0] + frame * strides[1] + key * strides[2] elements;
    counts (B, keys), totals (B), notes (B, cap, 3) int32 (None with cap = 0), lens (B) int32 or None, onset (B, keys, T) int8 or None."""
    _launch("roll_notes<%s>" % ("f32" if roll.dtype == torch.float32 else "u8"), 0.0, 2.0 * B * T * keys * roll.element_size(),
            lambda: lib().v2a_roll_notes(roll.data_ptr(), roll.element_size(), strides[0], strides[1], strides[2], float(threshold), B, T, keys,
                                         _p(lens), counts.data_ptr(), totals.data_ptr(), _p(notes), cap, _p(onset), stream_ptr()))


# ---- N1: Encodec decoder (vocoder) ---------------------------------------------------------------
def elu_pad(x, out, *, T, C_, pad, reflect, act=True):
    _launch("elu_pad", 0.0, 4.0 * C_ * (2 * T + pad),
            lambda: lib().v2a_elu_pad(x.data_ptr(), out.data_ptr(), T, C_, pad, 1 if reflect else 0, 1 if act else 0, stream_ptr()))


def elu_pad_lr(x, out, *, T, C_, pad_left, pad_right, act=True):
    _launch("elu_pad_lr", 0.0, 4.0 * C_ * (2 * T + pad_left + pad_right),
            lambda: lib().v2a_elu_pad_lr(x.data_ptr(), out.data_ptr(), T, C_, pad_left, pad_right, 1 if act else 0, stream_ptr()))


ENCODEC_STAGE0_PARAMS = 3376     # floats of the parameter block of v2a_encodec_stage0 (include/v2a_cfm.h)


def encodec_stage0(wave, params, out, *, n):
    _launch("encodec_stage0", 2.0 * n * 3744, 4.0 * n * 33,
            lambda: lib().v2a_encodec_stage0(wave.data_ptr(), params.data_ptr(), out.data_ptr(), n, stream_ptr()))


def encodec_rvq_encode(x, strides, codebooks, norms, codes, *, B, T, n_q):
    """x: fp32 tensor read as x[b * strides[0] + t * strides[1] + c * strides[2]]; codebooks (S, Kc, D), norms (S, Kc); codes (n_q, B * T) int64."""
    S, Kc, D = codebooks.shape
    _launch("encodec_rvq_encode", 2.0 * B * T * n_q * Kc * D, 4.0 * (B * T * D + n_q * Kc * D * -(-B * T // 16)) + 8.0 * n_q * B * T,
            lambda: lib().v2a_encodec_rvq_encode(x.data_ptr(), strides[0], strides[1], strides[2], B, T, codebooks.data_ptr(), norms.data_ptr(),
                                                 S, Kc, D, n_q, codes.data_ptr(), stream_ptr()))


def encodec_rvq_decode(codes, codebooks, out, strides, *, B, T, n_q):
    """codes (n_q, B * T) int64 -> out written as out[b * strides[0] + t * strides[1] + c * strides[2]]."""
    S, Kc, D = codebooks.shape
    _launch("encodec_rvq_decode", 1.0 * B * T * n_q * D, B * T * (4.0 * D * (n_q + 1) + 8.0 * n_q),
            lambda: lib().v2a_encodec_rvq_decode(codes.data_ptr(), n_q, B, T, codebooks.data_ptr(), S, Kc, D, out.data_ptr(),
                                                 strides[0], strides[1], strides[2], stream_ptr()))


# ---- validation pass (E2TTS.forward(val=True)) ---------------------------------------------------
LOSS_MAX_PARTS = 256             # V2A_LOSS_MAX_PARTS: workgroup partials of the two loss reductions


def cfm_interp(x0, x1, t, span, w, flow, cond=None):
    """w = (1 - t) x0 + t x1, flow = x1 - x0, cond = span ? 0 : x1 (cond None: not written; span None: no frame in the span).
    x0, x1, w, flow, cond (B, T, C) fp32 contiguous, t (B,) fp32, span (B, T) uint8."""
    B, T, C_ = x1.shape
    _launch("cfm_interp", 4.0 * B * T * C_, 4.0 * B * T * C_ * (4 if cond is None else 5),
            lambda: lib().v2a_cfm_interp(x0.data_ptr(), x1.data_ptr(), t.data_ptr(), _p(span), w.data_ptr(), flow.data_ptr(), _p(cond),
                                         B, T, C_, stream_ptr()))


def masked_sqerr(pred, target, mask, out):
    """out (2,) float64 <- (sum of (pred - target)^2 in double over the frames of mask (B, T) uint8, number of elements)."""
    B, T, C_ = pred.shape
    scratch = torch.empty(LOSS_MAX_PARTS * 2, dtype=torch.float64, device=pred.device)
    _launch("masked_sqerr", 3.0 * B * T * C_, 8.0 * B * T * C_,
            lambda: lib().v2a_masked_sqerr(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, T, C_, scratch.data_ptr(), out.data_ptr(),
                                           stream_ptr()))


def roll_metrics(roll, midis, mask, out):
    """out (6,) float64 <- (sum of (roll - midis)^2 |midis - 0.10|, number of elements, tp, fp, fn, tn); roll, midis (B, T, notes)."""
    B, T, notes = roll.shape
    scratch = torch.empty(LOSS_MAX_PARTS * 6, dtype=torch.float64, device=roll.device)
    _launch("roll_metrics", 5.0 * B * T * notes, 16.0 * B * T * notes,
            lambda: lib().v2a_roll_metrics(roll.data_ptr(), midis.data_ptr(), mask.data_ptr(), B, T, notes, scratch.data_ptr(), out.data_ptr(),
                                           stream_ptr()))


def lstm_layer(gates_x, w_hh, h, workspace, *, T, H, resid=None, y=None):
    _launch("lstm_layer", 2.0 * T * 4 * H * H, 4.0 * T * 6 * H,
            lambda: lib().v2a_lstm_layer(gates_x.data_ptr(), w_hh.data_ptr(), h.data_ptr(), _p(resid), _p(y), T, H,
                                         workspace.data_ptr(), stream_ptr()))


def lstm2(gates_x0, w_hh0, w_ih1, bias1, w_hh1, y, workspace, *, T, H, resid=None):
    _launch("lstm2", 2.0 * T * 4 * H * H * 3, 4.0 * T * 6 * H,
            lambda: lib().v2a_lstm2(gates_x0.data_ptr(), w_hh0.data_ptr(), w_ih1.data_ptr(), bias1.data_ptr(), w_hh1.data_ptr(),
                                    _p(resid), y.data_ptr(), T, H, workspace.data_ptr(), stream_ptr()))


# ---- FLAN-T5 prompt encoder (t5.py) ------------------------------------------------------------
def t5_rmsnorm(x, y, w, *, rows, d, eps, ids=None, vocab=0, resid=None, ldx=None, ldy=None):
    """T5LayerNorm of `rows` rows; with ids, x is the embedding table and the gathered rows also go to resid."""
    _launch("t5_rmsnorm%s" % ("+gather" if ids is not None else ""), 0.0, rows * d * (12 if ids is not None else 8),
            lambda: lib().v2a_t5_rmsnorm(x.data_ptr(), ldx or d, _p(ids), vocab, _p(resid), d, y.data_ptr(), ldy or d, rows, d,
                                         w.data_ptr(), float(eps), stream_ptr()))


def t5_attention(qkv, out, bias, key_mask, *, B, H, N, inner):
    """q | k | v read in place from the fused (B*N, 3*inner) GEMM output; out (B*N, inner)."""
    a = T5AttnArgs()
    base, ld = qkv.data_ptr(), qkv.stride(0)
    a.q, a.k, a.v, a.out = base, base + 4 * inner, base + 8 * inner, out.data_ptr()
    a.q_row_stride = a.k_row_stride = a.v_row_stride = ld
    a.out_row_stride = out.stride(0)
    a.q_batch_stride = a.k_batch_stride = a.v_batch_stride = N * ld
    a.out_batch_stride = N * out.stride(0)
    a.B, a.H, a.N, a.d_kv = B, H, N, 64
    a.bias, a.key_mask = bias.data_ptr(), key_mask.data_ptr()
    _launch("t5_attention", 4.0 * B * H * N * N * 64, 4.0 * B * N * (4 * inner),
            lambda: lib().v2a_t5_attention(C.byref(a), stream_ptr()))


def gemm_skinny(a, w, out, *, M, N, K, epilogue=EPI_STORE, resid=None, bias=None):
    """One v2a_gemm_skinny_f32 launch: a (M, K) fp32 rows, w [N][K] fp32, out (M, N) (GEGLU_TANH: (M, N/2))."""
    g = GemmArgs()
    g.a[0], g.lda[0], g.ka[0], g.nseg = a.data_ptr(), a.stride(0), K, 1
    g.a_dtype = g.compute_dtype = g.out_dtype = F32
    g.w, g.ldw = w.data_ptr(), w.stride(0)
    g.bias = _p(bias)
    g.M, g.N, g.epilogue = M, N, epilogue
    g.out, g.ldo = out.data_ptr(), out.stride(0)
    g.resid, g.ldr = _p(resid), (resid.stride(0) if resid is not None else 0)
    key = "gemm_skinny<f32,%s>" % _EPI_NAMES[epilogue]
    if _prof is not None and _prof.shapes:
        key += " %dx%dx%d" % (M, N, K)
    nbytes = 4.0 * (M * K + N * K + M * (N // 2 if epilogue == EPI_GEGLU_TANH else N) * (2 if resid is not None else 1))
    _launch(key, 2.0 * M * N * K, nbytes, lambda: lib().v2a_gemm_skinny_f32(C.byref(g), stream_ptr()))
