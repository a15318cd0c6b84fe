"""CLIP ViT image encoder on the HIP kernels of include/v2a_cfm.h: the `video_encoder="clip_vit"` model of the reference
(x3:1423-1425) -- transformers `CLIPImageProcessor()` followed by `CLIPVisionModelWithProjection` loaded from IP-Adapter
`sdxl_models/image_encoder` (OpenCLIP ViT-bigG/14) -- which turns every decoded video frame into one `image_embeds` row
(x3:1714, 1733-1735).

Preprocessing runs on the GPU and equals the processor's Pillow path bit for bit: the shortest edge is resized to the image
size with Pillow's BICUBIC (two separable passes of 22-bit fixed-point integer sums, the intermediate clipped to uint8, the
filter widened by the downscale factor), the centre is cropped, and every byte is mapped through a host table of the
processor's fp32 rescale / normalise (resample.py).

Compute modes: `"fp32"` -- exact-fp32 MFMA GEMMs; `"bf16x3"` -- every GEMM operand as hi | lo bf16 planes (three bf16 MFMA
products per fp32 product, fp32 accumulate).  LayerNorm, attention and the residual stream are fp32 in both.  Every layer is
computed on all tokens (no CLS-only shortcut in the last layer).

The engine is vit.py's; here are the key mapping, the shape checks, the K padding of the weights (104-wide heads make the hidden
width no multiple of 64) and the head: post-LayerNorm of the class rows, then the bias-free projection.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .resample import (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, PRECISION_BITS, ResizePlan, normalize_table, resample_coeffs,  # noqa: F401
                       resize_output_size)
from .vit import ViTImageEncoder
from .weights import strip_keys  # noqa: F401

_PREFIXES = ("image_encoder.",)


def infer_config(sd: dict[str, torch.Tensor]) -> dict:
    """Shapes -> config (heads cannot be read off the shapes: 104-wide heads, ViT-bigG's, are assumed unless given)."""
    pe = sd["vision_model.embeddings.patch_embedding.weight"]
    d, P = pe.shape[0], pe.shape[-1]
    T = sd["vision_model.embeddings.position_embedding.weight"].shape[0]
    g = int(round(math.sqrt(T - 1)))
    layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("vision_model.encoder.layers."))
    return dict(hidden_size=d, intermediate_size=sd["vision_model.encoder.layers.0.mlp.fc1.weight"].shape[0], num_hidden_layers=layers,
                num_attention_heads=max(1, d // 104), image_size=g * P, patch_size=P,
                projection_dim=sd["visual_projection.weight"].shape[0], layer_norm_eps=1e-5, hidden_act="gelu", num_channels=pe.shape[1])


class CLIPImageEncoder(ViTImageEncoder):
    """`CLIPImageProcessor()` + `CLIPVisionModelWithProjection` (image_embeds) on the HIP kernels.

    `CLIPImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32)`: plain CLIPVisionModelWithProjection keys or a
    reference checkpoint's `image_encoder.*`; config = a dict of CLIPVisionConfig fields (inferred from the shapes when absent).
    `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, projection_dim) float32 on the device, `chunk` frames per pass (a frame's
    result does not depend on its chunk).  `from_pretrained`: a local HF directory (IP-Adapter sdxl_models/image_encoder)."""

    _CFG_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                 "projection_dim", "layer_norm_eps", "hidden_act", "num_channels")

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32):
        sd = strip_keys(state_dict, _PREFIXES)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        if cfg.get("hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"CLIPImageEncoder: hidden_act {cfg['hidden_act']!r} (only the exact-erf 'gelu' is supported)")
        d, H, P, S, dff = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["image_size"], cfg["intermediate_size"]
        if d % H or (d // H) % 4 or d // H > 112 or d % 4 or dff % 64 or S % P:
            raise ValueError(f"CLIPImageEncoder: hidden {d} / heads {H} / mlp {dff} / image {S} / patch {P} "
                             "(head dim a multiple of 4 up to 112, mlp width a multiple of 64)")
        # K of the hidden-width GEMM operands zero-padded to a multiple of 64; the processor resizes to the crop size
        super().__init__(cfg, device, compute, chunk, S=S, resize=S, kin=3 * P * P, dp=(d + 63) // 64 * 64, dff=dff, ffn=(L.EPI_GELU, dff),
                         out_dim=cfg["projection_dim"])
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        dev, wmat = self._dev, self._wmat
        padk = lambda t: torch.nn.functional.pad(t, (0, self.dp - t.shape[1]))    # zero K columns up to dp
        E = "vision_model.embeddings."
        self.patch_w = self._patch_weight(f32(E + "patch_embedding.weight"))
        self.cls = dev(f32(E + "class_embedding"))
        self.pos = dev(f32(E + "position_embedding.weight"))
        self.pre_ln = (dev(f32("vision_model.pre_layrnorm.weight")), dev(f32("vision_model.pre_layrnorm.bias")))
        self.post_ln = (dev(f32("vision_model.post_layernorm.weight")), dev(f32("vision_model.post_layernorm.bias")))
        self.proj = wmat(padk(f32("visual_projection.weight")))
        self.layers = []
        for i in range(cfg["num_hidden_layers"]):
            p = f"vision_model.encoder.layers.{i}."
            a = p + "self_attn."
            self.layers.append(dict(
                ln1=(dev(f32(p + "layer_norm1.weight")), dev(f32(p + "layer_norm1.bias"))),
                qkv=wmat(padk(torch.cat([f32(a + "q_proj.weight"), f32(a + "k_proj.weight"), f32(a + "v_proj.weight")], 0))),
                qkv_b=dev(torch.cat([f32(a + "q_proj.bias"), f32(a + "k_proj.bias"), f32(a + "v_proj.bias")], 0)),
                o=wmat(padk(f32(a + "out_proj.weight"))), o_b=dev(f32(a + "out_proj.bias")),
                ln2=(dev(f32(p + "layer_norm2.weight")), dev(f32(p + "layer_norm2.bias"))),
                fc1=wmat(padk(f32(p + "mlp.fc1.weight"))), fc1_b=dev(f32(p + "mlp.fc1.bias")),
                fc2=wmat(f32(p + "mlp.fc2.weight")), fc2_b=dev(f32(p + "mlp.fc2.bias"))))
        self.lut = dev(torch.from_numpy(normalize_table()))

    def _head_buffers(self, F: int) -> dict:
        return dict(pooled=torch.zeros(F, self.w * self.dp, dtype=self.adt, device=self.device))     # K pad columns stay zero

    def head(self, bf: dict, F: int) -> torch.Tensor:
        """image_embeds: post_layernorm on the class rows (row stride T * d), visual_projection (no bias)."""
        self.layernorm(bf["h"], bf["pooled"], self.post_ln, rows=F, ldx=self.T * self.d)
        self._gemm(bf["pooled"], self.w * self.dp, self.dp, self.proj, bf["out"], M=F, N=self.out_dim)
        return bf["out"]
