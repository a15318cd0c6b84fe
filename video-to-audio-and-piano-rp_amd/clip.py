"""CLIP ViT image encoders on the HIP kernels of include/v2a_cfm.h.  `CLIPImageEncoder`: the `video_encoder="clip_vit"` model of the reference
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

`CLIPViT2ImageEncoder`: the `video_encoder="clip_vit2"` model (x3:1426-1428) -- `AutoProcessor` + `CLIPVisionModelWithProjection` of
openai/clip-vit-large-patch14-336 (ViT-L/14 at 336 px: d = 1024, 24 layers, 16 heads of 64, MLP 4096 with `quick_gelu`, 577 tokens,
projection to 768), one `image_embeds` row per frame (x3:1714, 1736-1738).  The same class with other defaults: the feed-forward's first
GEMM carries the QUICK_GELU epilogue, and the 64-wide heads run on the MFMA kernels of v2a_attention (the engine's `mfma_attention`).
"""
from __future__ import annotations

import json
import math
import os

import torch

from . import _lib as L
from .resample import (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, PRECISION_BITS, ResizePlan, normalize_table, resample_coeffs,  # noqa: F401
                       resize_output_size)
from .vit import ViTImageEncoder
from .weights import strip_keys  # noqa: F401

_PREFIXES = ("image_encoder.",)
PIL_BICUBIC = 3
_FFN_EPILOGUES = {"gelu": L.EPI_GELU, "quick_gelu": L.EPI_QUICK_GELU}


def infer_config(sd: dict[str, torch.Tensor], head_dim: int = 104, hidden_act: str = "gelu") -> dict:
    """Shapes -> config (neither the heads nor the activation can be read off the shapes: `head_dim`-wide heads -- 104, ViT-bigG's -- and
    `hidden_act` are assumed unless given)."""
    pe = sd["vision_model.embeddings.patch_embedding.weight"]
    d, P = pe.shape[0], pe.shape[-1]
    T = sd["vision_model.embeddings.position_embedding.weight"].shape[0]
    g = int(round(math.sqrt(T - 1)))
    layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("vision_model.encoder.layers."))
    return dict(hidden_size=d, intermediate_size=sd["vision_model.encoder.layers.0.mlp.fc1.weight"].shape[0], num_hidden_layers=layers,
                num_attention_heads=max(1, d // head_dim), image_size=g * P, patch_size=P,
                projection_dim=sd["visual_projection.weight"].shape[0], layer_norm_eps=1e-5, hidden_act=hidden_act, num_channels=pe.shape[1])


class CLIPImageEncoder(ViTImageEncoder):
    """`CLIPImageProcessor()` + `CLIPVisionModelWithProjection` (image_embeds) on the HIP kernels.

    `CLIPImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32, resize=None, image_mean=OPENAI, image_std=OPENAI)`:
    plain CLIPVisionModelWithProjection keys or a reference checkpoint's `image_encoder.*`; config = a dict of CLIPVisionConfig fields
    (inferred from the shapes when absent; `hidden_act`: "gelu", this model's; `CLIPViT2ImageEncoder` also takes "quick_gelu"); resize = the processor's shortest-edge target (the
    image size when absent; the crop is always the image size, the position table has no other).
    `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, projection_dim) float32 on the device, `chunk` frames per pass (a frame's
    result does not depend on its chunk).  `from_pretrained`: a local HF directory (IP-Adapter sdxl_models/image_encoder)."""

    _CFG_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                 "projection_dim", "layer_norm_eps", "hidden_act", "num_channels")
    _HEAD_DIM = 104                      # what a state dict cannot reveal: the head width and the activation assumed unless given
    _HIDDEN_ACT = "gelu"
    _HIDDEN_ACTS = ("gelu",)             # the activations the class runs: the exact-erf GELU of ViT-bigG only, as ever

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32, resize: int | None = None,
                 image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD):
        name = type(self).__name__
        sd = strip_keys(state_dict, _PREFIXES)
        cfg = infer_config(sd, self._HEAD_DIM, self._HIDDEN_ACT)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        if cfg["hidden_act"] not in self._HIDDEN_ACTS:
            raise NotImplementedError(f"{name}: hidden_act {cfg['hidden_act']!r} (built here: {', '.join(map(repr, self._HIDDEN_ACTS))}; "
                                      "'quick_gelu' is CLIPViT2ImageEncoder's)")
        d, H, P, S, dff = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["image_size"], cfg["intermediate_size"]
        if d % H or (d // H) % 4 or d // H > 112 or d % 4 or dff % 64 or S % P:
            raise ValueError(f"{name}: hidden {d} / heads {H} / mlp {dff} / image {S} / patch {P} "
                             "(head dim a multiple of 4 up to 112, mlp width a multiple of 64)")
        resize = S if resize is None else int(resize)
        if resize < S:
            raise ValueError(f"{name}: resize {resize} must be >= the image size {S}")
        self.mfma_attention = d // H == 64       # 64-wide heads: v2a_attention, as DINOv2; any other width: the VALU kernel
        # K of the hidden-width GEMM operands zero-padded to a multiple of 64; the default processor resizes to the crop size
        super().__init__(cfg, device, compute, chunk, S=S, resize=resize, kin=3 * P * P, dp=(d + 63) // 64 * 64, dff=dff,
                         ffn=(_FFN_EPILOGUES[cfg["hidden_act"]], dff), out_dim=cfg["projection_dim"])
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
        self.lut = dev(torch.from_numpy(normalize_table(image_mean, image_std)))

    def _head_buffers(self, F: int) -> dict:
        return dict(pooled=torch.zeros(F, self.w * self.dp, dtype=self.adt, device=self.device))     # K pad columns stay zero

    def head(self, bf: dict, F: int) -> torch.Tensor:
        """image_embeds: post_layernorm on the class rows (row stride T * d), visual_projection (no bias)."""
        self.layernorm(bf["h"], bf["pooled"], self.post_ln, rows=F, ldx=self.T * self.d)
        self._gemm(bf["pooled"], self.w * self.dp, self.dp, self.proj, bf["out"], M=F, N=self.out_dim)
        return bf["out"]


class CLIPViT2ImageEncoder(CLIPImageEncoder):
    """`AutoProcessor` + `CLIPVisionModelWithProjection` (image_embeds) of openai/clip-vit-large-patch14-336 on the HIP kernels: a
    `CLIPImageEncoder` whose defaults are that model's -- `quick_gelu` and 64-wide heads (16 of them at hidden 1024), which a state dict
    cannot reveal -- and the only class that takes `hidden_act="quick_gelu"` (a config may still say "gelu").  `from_pretrained`: a local HF directory with config.json, optionally preprocessor_config.json, and the weights."""

    _HEAD_DIM = 64
    _HIDDEN_ACT = "quick_gelu"
    _HIDDEN_ACTS = ("quick_gelu", "gelu")

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """config.json (`vision_config` when nested) and, when present, preprocessor_config.json: `size` (shortest_edge, or the legacy
        integer), `crop_size` (an integer or height / width; square, and the model's image size), `image_mean` / `image_std`.  A
        resample other than BICUBIC and do_resize / do_center_crop / do_normalize = false are refused: those paths are not built."""
        name = cls.__name__
        pp = os.path.join(path, "preprocessor_config.json")
        crop = None
        if os.path.exists(pp):
            with open(pp) as f:
                pc = json.load(f)
            if pc.get("resample", PIL_BICUBIC) != PIL_BICUBIC:
                raise NotImplementedError(f"{name}: resample {pc['resample']} (only PIL BICUBIC = {PIL_BICUBIC} is built)")
            for k in ("do_resize", "do_center_crop", "do_normalize"):
                if not pc.get(k, True):
                    raise NotImplementedError(f"{name}: {k} = false in preprocessor_config.json (that path is not built)")
            size, cs = pc.get("size"), pc.get("crop_size")
            if isinstance(size, dict):
                if "shortest_edge" not in size:
                    raise NotImplementedError(f"{name}: size {size} (only shortest_edge is built)")
                size = size["shortest_edge"]
            if size is not None:
                kw.setdefault("resize", int(size))
            if isinstance(cs, dict):
                if cs["height"] != cs.get("width", cs["height"]):
                    raise NotImplementedError(f"{name}: crop_size {cs} (square crops only)")
                cs = cs["height"]
            crop = None if cs is None else int(cs)
            if "image_mean" in pc:
                kw.setdefault("image_mean", tuple(pc["image_mean"]))
            if "image_std" in pc:
                kw.setdefault("image_std", tuple(pc["image_std"]))
        enc = super().from_pretrained(path, device, **kw)
        if crop is not None and crop != enc.S:
            raise NotImplementedError(f"{name}: crop_size {crop} differs from the model's image size {enc.S} (CLIP's position table has no other)")
        return enc
