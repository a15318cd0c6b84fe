"""DINOv2 image encoder on the HIP kernels of include/v2a_cfm.h: the `video_encoder="dinov2"` model of the reference
(x3:1432-1433) -- transformers `AutoImageProcessor` (a `BitImageProcessor`: shortest edge to 256, centre crop 224, ImageNet
mean / std, BICUBIC) followed by `AutoModel` of dinov2-giant (`Dinov2Model`, ViT-g/14: 40 layers, d = 1536, 24 heads of 64, SwiGLU
feed-forward with 4096 hidden values, LayerScale) -- which turns every decoded video frame into one `pooler_output` row
(x3:1714, 1742-1744).

The engine is vit.py's (preprocessing, layer loop, compute modes), here with a resize target that differs from the crop, operands
without K padding (64-wide heads), no pre-LayerNorm, and the final LayerNorm of the class rows as the head.

Prepared on the host at load time: the position table interpolated to the crop's grid with the library's own call
(`Dinov2Embeddings.interpolate_pos_encoding`: F.interpolate, bicubic, align_corners=False, float32), the patch bias folded into its
patch rows, LayerScale folded into the `dense` / `weights_out` (`fc2`) weights and biases in float64 before rounding or
splitting, and `weights_in` regrouped [16 value | 16 gate] for the SWIGLU epilogue of v2a_gemm (gate = x1, value = x2).

Attention runs on the MFMA kernels of v2a_attention (the engine's `mfma_attention`: 64-wide heads, no gate, no clamp; in `"bf16x3"`
its products are on hi | lo bf16 planes as well), reading the fused qkv buffer in place.
"""
from __future__ import annotations

import json
import math
import os

import torch

from . import _lib as L
from .resample import normalize_table
from .vit import ViTImageEncoder
from .weights import strip_keys

_PREFIXES = ("image_encoder.",)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PIL_BICUBIC = 3


def infer_config(sd: dict[str, torch.Tensor]) -> dict:
    """Shapes -> config (heads cannot be read off the shapes: 64-wide heads, every DINOv2 size's, are assumed unless given)."""
    pw = sd["embeddings.patch_embeddings.projection.weight"]
    d, P = pw.shape[0], pw.shape[-1]
    g = int(round(math.sqrt(sd["embeddings.position_embeddings"].shape[1] - 1)))
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    return dict(hidden_size=d, num_hidden_layers=layers, num_attention_heads=max(1, d // 64), image_size=g * P, patch_size=P,
                layer_norm_eps=1e-6, use_swiglu_ffn="encoder.layer.0.mlp.weights_in.weight" in sd, num_channels=pw.shape[1])


def pack_swiglu(w_in: torch.Tensor) -> torch.Tensor:
    """[16 value | 16 gate] row packing of V2A_EPI_SWIGLU from `Dinov2SwiGLUFFN.weights_in` rows (or its bias): the module computes
    silu(x1) * x2 with x1 = rows [0, Hf), x2 = rows [Hf, 2 Hf), so gate = x1 and value = x2, per group of 16 outputs."""
    hf = w_in.shape[0] // 2
    gate, value = w_in[:hf], w_in[hf:]
    tail = w_in.shape[1:]
    return torch.cat([value.reshape(hf // 16, 16, *tail), gate.reshape(hf // 16, 16, *tail)], 1).reshape(2 * hf, *tail).contiguous()


def fold_layerscale(lam: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """LayerScale after a Linear, lam * (x W^T + b), as that Linear's own weight and bias: products in float64, rounded once."""
    l64 = lam.double()
    return (l64[:, None] * w.double()).float(), (l64 * b.double()).float()


def interpolate_positions(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """(1, 1 + g0 * g0, d) stored position table -> (1 + grid * grid, d) float32 at the run's patch grid, by the very call of
    `Dinov2Embeddings.interpolate_pos_encoding` (which also skips the interpolation when the grids are equal)."""
    pos = pos.float()
    n0 = pos.shape[1] - 1
    if n0 == grid * grid:
        return pos[0].contiguous()
    g0, d = int(n0 ** 0.5), pos.shape[-1]
    patch = pos[:, 1:].reshape(1, g0, g0, d).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch.to(torch.float32), size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat((pos[:, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, d)), dim=1)[0].contiguous()


class DINOv2ImageEncoder(ViTImageEncoder):
    """`BitImageProcessor` + `Dinov2Model` (pooler_output) on the HIP kernels.

    `DINOv2ImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32, resize=256, crop=224, image_mean=IMAGENET,
    image_std=IMAGENET)`: plain Dinov2Model keys or a reference checkpoint's `image_encoder.*`; config = a dict of Dinov2Config fields
    (inferred from the shapes when absent).  `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, hidden_size) float32 on the device,
    `chunk` frames per pass (a frame's result does not depend on its chunk)."""

    _CFG_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size", "layer_norm_eps", "use_swiglu_ffn",
                 "num_channels")
    mfma_attention = True                # 64-wide heads: v2a_attention and the engine's workgroup floor (vit.py)

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32, resize: int = 256,
                 crop: int = 224, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD):
        sd = strip_keys(state_dict, _PREFIXES)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        d, H, P = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
        if d % H or d // H != 64:
            raise ValueError(f"DINOv2ImageEncoder: hidden {d} / heads {H}: the attention kernels take 64-wide heads only")
        if int(crop) % P or int(resize) < int(crop):
            raise ValueError(f"DINOv2ImageEncoder: crop {crop} must be a multiple of the patch size {P} and resize {resize} >= crop")
        self.swiglu = bool(cfg["use_swiglu_ffn"])
        # hidden values of the feed-forward (K of its second Linear)
        dff = sd["encoder.layer.0.mlp." + ("weights_out" if self.swiglu else "fc2") + ".weight"].shape[1]
        if dff % 64:
            raise ValueError(f"DINOv2ImageEncoder: feed-forward width {dff} must be a multiple of 64")
        super().__init__(cfg, device, compute, chunk, S=crop, resize=resize, kin=cfg["num_channels"] * P * P, dp=d, dff=dff,
                         ffn=(L.EPI_SWIGLU, 2 * dff) if self.swiglu else (L.EPI_GELU, dff), out_dim=d)
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        dev, wmat = self._dev, self._wmat
        E = "embeddings."
        self.patch_w = self._patch_weight(f32(E + "patch_embeddings.projection.weight"))
        # rows v2a_clip_embed_init writes: class row = cls_token + pos[0], patch rows = pos[t] + the patch projection's bias
        pos = interpolate_positions(f32(E + "position_embeddings"), self.g).double()
        pos[1:] += f32(E + "patch_embeddings.projection.bias").double()
        self.pos = dev(pos.float())
        self.cls = dev(f32(E + "cls_token").reshape(d))
        self.final_ln = (dev(f32("layernorm.weight")), dev(f32("layernorm.bias")))
        self.layers = []
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layer.{i}."
            a = p + "attention.attention."
            o_w, o_b = fold_layerscale(f32(p + "layer_scale1.lambda1"), f32(p + "attention.output.dense.weight"), f32(p + "attention.output.dense.bias"))
            if self.swiglu:
                w1, b1 = pack_swiglu(f32(p + "mlp.weights_in.weight")), pack_swiglu(f32(p + "mlp.weights_in.bias"))
                w2, b2 = f32(p + "mlp.weights_out.weight"), f32(p + "mlp.weights_out.bias")
            else:
                w1, b1, w2, b2 = f32(p + "mlp.fc1.weight"), f32(p + "mlp.fc1.bias"), f32(p + "mlp.fc2.weight"), f32(p + "mlp.fc2.bias")
            w2, b2 = fold_layerscale(f32(p + "layer_scale2.lambda1"), w2, b2)
            self.layers.append(dict(
                ln1=(dev(f32(p + "norm1.weight")), dev(f32(p + "norm1.bias"))),
                qkv=wmat(torch.cat([f32(a + "query.weight"), f32(a + "key.weight"), f32(a + "value.weight")], 0)),
                qkv_b=dev(torch.cat([f32(a + "query.bias"), f32(a + "key.bias"), f32(a + "value.bias")], 0)),
                o=wmat(o_w), o_b=dev(o_b),                       # LayerScale 1 folded
                ln2=(dev(f32(p + "norm2.weight")), dev(f32(p + "norm2.bias"))),
                fc1=wmat(w1), fc1_b=dev(b1), fc2=wmat(w2), fc2_b=dev(b2)))       # LayerScale 2 folded
        self.lut = dev(torch.from_numpy(normalize_table(image_mean, image_std)))

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A local HF directory (facebook/dinov2-giant): config.json, preprocessor_config.json (size.shortest_edge, crop_size,
        image_mean / image_std; a resample other than BICUBIC is refused), model.safetensors or pytorch_model.bin."""
        pp = os.path.join(path, "preprocessor_config.json")
        if os.path.exists(pp):
            with open(pp) as f:
                pc = json.load(f)
            if pc.get("resample", PIL_BICUBIC) != PIL_BICUBIC:
                raise NotImplementedError(f"DINOv2ImageEncoder: resample {pc['resample']} (only PIL BICUBIC = {PIL_BICUBIC} is built)")
            size, cs = pc.get("size", {}), pc.get("crop_size", {})
            if isinstance(size, dict) and "shortest_edge" in size:
                kw.setdefault("resize", int(size["shortest_edge"]))
            if isinstance(cs, dict) and "height" in cs:
                if cs["height"] != cs.get("width", cs["height"]):
                    raise NotImplementedError(f"DINOv2ImageEncoder: crop_size {cs} (square crops only)")
                kw.setdefault("crop", int(cs["height"]))
            elif isinstance(cs, int):
                kw.setdefault("crop", cs)
            if "image_mean" in pc:
                kw.setdefault("image_mean", tuple(pc["image_mean"]))
            if "image_std" in pc:
                kw.setdefault("image_std", tuple(pc["image_std"]))
        return super().from_pretrained(path, device, **kw)

    def head(self, bf: dict, F: int) -> torch.Tensor:
        """pooler_output: the final layernorm on the class rows (row stride T * d), fp32; no projection."""
        self.layernorm(bf["h"], bf["out"], self.final_ln, rows=F, ldx=self.T * self.d, y_dtype=L.F32)
        return bf["out"]
