"""CLIP ConvNeXt image encoder on the HIP kernels of include/v2a_cfm.h: the `video_encoder="clip_convnext"` model of the reference
(x3:1429-1431) -- open_clip's `CLIP-convnext_xxlarge-laion2B-s34B-b82K-augreg-soup`, whose `encode_image` is `TimmModel.forward` =
`head(trunk(x))` around timm's `convnext_xxlarge` (depths 3 / 4 / 30 / 3, widths 384 / 768 / 1536 / 3072, LayerNorm eps 1e-5, layer
scale) behind open_clip's `image_transform` (Resize(256, BICUBIC) on the PIL image, CenterCrop(256), ToTensor, Normalize) -- which
turns every decoded video frame into one embedding row (x3:1716-1720, 1739-1741).  `MixedImageEncoder` is the reference's "mixed":
the rows of four encoders side by side (x3:1745-1788).

Neither timm nor open_clip is installed here: the network is restated from their published layout (tests/convnext_ref.py in float64,
pinned where transformers' `ConvNextModel` can express it), the preprocessing from Pillow plus torchvision's size and crop arithmetic.

The engine is vit.py's for everything the two share (the Pillow-exact resize into a patch matrix, compute modes, the pinned split
tile, LayerNorm and GEMM helpers, the chunked `__call__`); the network walk is its own:
  stem        patches of 4 -> v2a_gemm (stem.0) -> v2a_clip_layernorm per pixel (stem.1), once per frame (the patch matrix keeps a
              class-token slot per frame that the map does not)
  downsample  v2a_clip_layernorm -> v2a_im2col (2 x 2, stride 2) [-> v2a_split_bf16] -> v2a_gemm
  block       v2a_convnext_dwconv -> v2a_clip_layernorm (into the mode's operand layout) -> v2a_gemm (fc1, GELU epilogue, plane output
              in bf16x3) -> v2a_gemm (fc2 with gamma folded in float64, RESID epilogue onto the fp32 map)
  head        v2a_convnext_pool_ln [-> v2a_split_bf16] -> v2a_gemm (head.proj)
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib as L
from .conv2d import gemm_weight
from .dinov2 import fold_layerscale
from .resample import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, normalize_table
from .vit import ViTImageEncoder

_PREFIXES = ("image_encoder.visual.", "image_encoder.", "visual.")
MIXED_ORDER = ("clip_vit", "clip_vit2", "clip_convnext", "dinov2")          # x3:1788
CONVNEXT_XXLARGE = dict(depths=(3, 4, 30, 3), dims=(384, 768, 1536, 3072), embed_dim=1024, image_size=256, layer_norm_eps=1e-5)


def is_convnext_state_dict(sd) -> bool:
    """Whether a state dict (under any of the accepted prefixes) holds this network: its stem convolution names it."""
    return isinstance(sd, dict) and "trunk.stem.0.weight" in strip_prefixes(sd)


def strip_prefixes(state_dict) -> dict[str, torch.Tensor]:
    """open_clip's `visual.trunk.` / `visual.head.`, a reference checkpoint's `image_encoder.` in front of either (optionally under
    `model_state_dict`), or the bare `trunk.` / `head.` -> the bare keys; other towers' keys are dropped."""
    sd = state_dict.get("model_state_dict", state_dict)
    out = {}
    for k, v in sd.items():
        for p in _PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        if k.startswith(("trunk.", "head.")):
            out[k] = v
    return out


def infer_config(sd: dict[str, torch.Tensor]) -> dict:
    """Shapes -> depths, dims, embed_dim (bare keys).  Variants outside the reference's model are refused by their keys."""
    if "trunk.stem.0.weight" not in sd:
        raise KeyError("CLIPConvNeXtImageEncoder: the state dict holds no trunk.stem.0.weight (open_clip's visual.trunk.* keys)")
    other = sorted(k for k in sd if k.startswith("head.") and k not in ("head.proj.weight", "head.proj.bias"))
    if other or "head.proj.weight" not in sd:
        raise NotImplementedError(f"CLIPConvNeXtImageEncoder: only open_clip's linear projection head (head.proj.weight) is built, got {other[:4]} "
                                  "(attention pooling and the MLP projection are not)")
    if any(".attn" in k or "attn_pool" in k for k in sd):
        raise NotImplementedError("CLIPConvNeXtImageEncoder: attention pooling is not built")
    stages = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("trunk.stages."))
    depths, dims = [], []
    for s in range(stages):
        p = f"trunk.stages.{s}.blocks."
        depths.append(1 + max(int(k[len(p):].split(".")[0]) for k in sd if k.startswith(p)))
        w1 = sd[p + "0.mlp.fc1.weight"]
        if w1.ndim != 2:
            raise NotImplementedError("CLIPConvNeXtImageEncoder: conv_mlp=True blocks (4-D mlp.fc1.weight) are not built")
        dims.append(w1.shape[1])
        if p + "0.gamma" not in sd:
            raise KeyError(f"CLIPConvNeXtImageEncoder: {p}0.gamma is missing (the model has layer scale)")
    st = sd["trunk.stem.0.weight"]
    if tuple(st.shape) != (dims[0], 3, 4, 4):
        raise ValueError(f"CLIPConvNeXtImageEncoder: stem.0.weight {tuple(st.shape)}, expected ({dims[0]}, 3, 4, 4)")
    return dict(depths=tuple(depths), dims=tuple(dims), embed_dim=sd["head.proj.weight"].shape[0], layer_norm_eps=1e-5)


class CLIPConvNeXtImageEncoder(ViTImageEncoder):
    """open_clip `image_transform` + `TimmModel` (ConvNeXt trunk, pooled, normed, projected) on the HIP kernels.

    `CLIPConvNeXtImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32, resize=256, crop=256, image_mean=OPENAI,
    image_std=OPENAI)`: open_clip keys (`visual.trunk.*`, `visual.head.proj.*`), a reference checkpoint's `image_encoder.*`, or bare
    `trunk.*` / `head.*`; depths, widths and embed_dim come from the shapes, `config["layer_norm_eps"]` defaults to 1e-5
    (convnext_xxlarge; timm's smaller ConvNeXts use 1e-6).  `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, embed_dim) float32 on the
    device, `chunk` frames per pass (a frame's result does not depend on its chunk)."""

    crop_offset = "torchvision"          # CenterCrop's int(round((h - S) / 2.0)), not the transformers processors' floor

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32, resize: int = 256,
                 crop: int = 256, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD):
        name = type(self).__name__
        sd = strip_prefixes(state_dict)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k == "layer_norm_eps"})
        self.depths, self.dims, E = cfg["depths"], cfg["dims"], cfg["embed_dim"]
        ns = len(self.dims)
        if any(c % 64 for c in self.dims) or E % 16:
            raise ValueError(f"{name}: widths {self.dims} must be multiples of 64 and embed_dim {E} of 16")
        if max(self.dims) > 4096:
            raise ValueError(f"{name}: widths {self.dims}: the LayerNorm kernels take up to 4096 channels")
        down = 4 * 2 ** (ns - 1)
        if int(crop) % down or int(resize) < int(crop):
            raise ValueError(f"{name}: crop {crop} must be a multiple of {down} (the stem's 4 and {ns - 1} halvings) and resize {resize} >= crop")
        super().__init__(dict(cfg, hidden_size=self.dims[0], num_attention_heads=1, patch_size=4), device, compute, chunk, S=crop, resize=resize,
                         kin=48, dp=self.dims[0], dff=4 * self.dims[0], ffn=(L.EPI_GELU, 4 * self.dims[0]), out_dim=E)
        self.sizes = tuple(self.g >> s for s in range(ns))                  # map edge per stage
        want = {"trunk.stem.0.bias": (self.dims[0],), "trunk.stem.1.weight": (self.dims[0],), "trunk.stem.1.bias": (self.dims[0],),
                "trunk.head.norm.weight": (self.dims[-1],), "trunk.head.norm.bias": (self.dims[-1],), "head.proj.weight": (E, self.dims[-1])}
        for s, (n, C) in enumerate(zip(self.depths, self.dims)):
            p = f"trunk.stages.{s}."
            if s:
                want.update({p + "downsample.0.weight": (self.dims[s - 1],), p + "downsample.0.bias": (self.dims[s - 1],),
                             p + "downsample.1.weight": (C, self.dims[s - 1], 2, 2), p + "downsample.1.bias": (C,)})
            for j in range(n):
                b = p + f"blocks.{j}."
                want.update({b + "conv_dw.weight": (C, 1, 7, 7), b + "conv_dw.bias": (C,), b + "norm.weight": (C,), b + "norm.bias": (C,),
                             b + "mlp.fc1.weight": (4 * C, C), b + "mlp.fc1.bias": (4 * C,), b + "mlp.fc2.weight": (C, 4 * C),
                             b + "mlp.fc2.bias": (C,), b + "gamma": (C,)})
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"{name}: state dict lacks {len(missing)} keys, e.g. {missing[:4]}")
        bad = [k for k, shp in want.items() if tuple(sd[k].shape) != shp]
        if bad:
            raise ValueError(f"{name}: shape mismatch for {bad[:4]}")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        dev, wmat = self._dev, self._wmat
        pair = lambda k: (dev(f32(k + ".weight")), dev(f32(k + ".bias")))
        self.patch_w, self.patch_b = self._patch_weight(f32("trunk.stem.0.weight")), dev(f32("trunk.stem.0.bias"))
        self.stem_ln = pair("trunk.stem.1")
        self.stages = []
        for s, (n, C) in enumerate(zip(self.depths, self.dims)):
            p = f"trunk.stages.{s}."
            st = dict(blocks=[])
            if s:
                # (ky, kx, c) rows: v2a_im2col's column order over the NHWC map
                st.update(ds_ln=pair(p + "downsample.0"), ds_w=wmat(gemm_weight(f32(p + "downsample.1.weight"))), ds_b=dev(f32(p + "downsample.1.bias")))
            for j in range(n):
                b = p + f"blocks.{j}."
                w2, b2 = fold_layerscale(f32(b + "gamma"), f32(b + "mlp.fc2.weight"), f32(b + "mlp.fc2.bias"))
                st["blocks"].append(dict(dw_w=dev(f32(b + "conv_dw.weight").reshape(C, 49).t()), dw_b=dev(f32(b + "conv_dw.bias")),
                                         ln=pair(b + "norm"), fc1=wmat(f32(b + "mlp.fc1.weight")), fc1_b=dev(f32(b + "mlp.fc1.bias")),
                                         fc2=wmat(w2), fc2_b=dev(b2)))                   # gamma folded
            self.stages.append(st)
        self.head_ln = pair("trunk.head.norm")
        self.proj = wmat(f32("head.proj.weight"))
        self.proj_b = dev(f32("head.proj.bias")) if "head.proj.bias" in sd else None
        self.lut = dev(torch.from_numpy(normalize_table(image_mean, image_std, formula="torchvision")))

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A local open_clip directory: open_clip_config.json (`model_cfg.vision_cfg`: `timm_model_name` gives the LayerNorm eps --
        1e-5 for convnext_xxlarge, timm's 1e-6 otherwise -- and `image_size` the resize and crop; `preprocess_cfg` mean / std when
        there) and open_clip_model.safetensors or open_clip_pytorch_model.bin.  Nothing is fetched."""
        cp = os.path.join(path, "open_clip_config.json")
        config = dict(kw.pop("config", None) or {})
        if os.path.exists(cp):
            with open(cp) as f:
                oc = json.load(f)
            vc = oc.get("model_cfg", oc).get("vision_cfg", {})
            tm = vc.get("timm_model_name", "")
            if tm and not tm.startswith("convnext"):
                raise NotImplementedError(f"{cls.__name__}: timm_model_name {tm!r} (only ConvNeXt trunks are built)")
            if vc.get("timm_pool", "") not in ("", "avg") or vc.get("timm_proj", "linear") != "linear":
                raise NotImplementedError(f"{cls.__name__}: timm_pool {vc.get('timm_pool')!r} / timm_proj {vc.get('timm_proj')!r} "
                                          "(only average pooling and the linear projection are built)")
            if tm:
                config.setdefault("layer_norm_eps", 1e-5 if "xxlarge" in tm else 1e-6)
            if "image_size" in vc:
                kw.setdefault("resize", int(vc["image_size"]))
                kw.setdefault("crop", int(vc["image_size"]))
            pc = oc.get("preprocess_cfg", {})
            if pc.get("interpolation", "bicubic") != "bicubic" or pc.get("resize_mode", "shortest") != "shortest":
                raise NotImplementedError(f"{cls.__name__}: preprocess_cfg {pc} (only the shortest-edge BICUBIC resize is built)")
            if "mean" in pc:
                kw.setdefault("image_mean", tuple(pc["mean"]))
            if "std" in pc:
                kw.setdefault("image_std", tuple(pc["std"]))
        st = os.path.join(path, "open_clip_model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "open_clip_pytorch_model.bin"), map_location="cpu")
        return cls(sd, device, config=config or None, **kw)

    # ---- device pieces -----------------------------------------------------------------------------
    def _buffers(self, F: int) -> dict:
        bf = self._bufs.get(F)
        if bf is None:
            w, dims = self.w, self.dims
            rows = [F * g * g for g in self.sizes]
            act = max(m * c for m, c in zip(rows, dims))
            col = max([rows[s] * 4 * dims[s - 1] for s in range(1, len(dims))] + [1])
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
            # zeroed: the class-token rows and pad columns of the patch matrix (the resize kernel never writes them)
            bf = dict(patches=torch.zeros(F * self.T, w * self.kp, dtype=self.adt, device=self.device), stem=e(F * self.T, dims[0]),
                      h=[e(m, c) for m, c in zip(rows, dims)], y=e(act), x=e(w * act, dt=self.adt), ff=e(w * max(4 * act, col), dt=self.adt),
                      col=e(col), pooled=e(F, dims[-1]), pooled_op=e(F, w * dims[-1], dt=self.adt), out=e(F, self.out_dim))
            self._bufs = {F: bf}           # one live chunk size
        return bf

    def _ln(self, x, y, ln, *, rows, d, ldy, f32=False):
        """LayerNorm over the d channels of `rows` pixels into fp32 rows, or (default) a GEMM operand in the mode's layout."""
        out_bytes = 4 if f32 or not self.split else 2 * 2
        L._launch("clip_layernorm<%s>" % ("f32" if f32 or not self.split else "split"), 0.0, rows * d * (4.0 + out_bytes),
                  lambda: L.lib().v2a_clip_layernorm(x.data_ptr(), d, y.data_ptr(), ldy, L.F32 if f32 else self.ydt, rows, d, ln[0].data_ptr(),
                                                     ln[1].data_ptr(), self.eps, L.stream_ptr()))

    def dwconv(self, x, out, blk, *, F, H, W, C):
        """conv_dw: the 7 x 7 depthwise convolution + bias of the fp32 NHWC map x into out."""
        L._launch("convnext_dwconv", 98.0 * F * H * W * C, 8.0 * F * H * W * C,
                  lambda: L.lib().v2a_convnext_dwconv(x.data_ptr(), out.data_ptr(), blk["dw_w"].data_ptr(), blk["dw_b"].data_ptr(), F, H, W, C,
                                                      L.stream_ptr()))

    def _operand(self, x32, buf, *, rows, d):
        """fp32 rows as a GEMM A operand: themselves, or their hi | lo planes in `buf`."""
        if not self.split:
            return x32
        L.split_bf16(x32, buf, rows=rows, d=d)
        return buf

    @torch.no_grad()
    def encode_chunk(self, frames: torch.Tensor, *, taps: dict | None = None, crop: torch.Tensor | None = None) -> torch.Tensor:
        """One chunk: frames (F, H, W, 3) uint8 on the device -> (F, embed_dim) float32 (a view of a reused buffer).
        `taps`: dict whose keys are "stem" or (stage, block), both from 0; each receives a device copy of the fp32 map (F, h, w, C)
        behind the stem's LayerNorm or behind that block.  `crop`: optional (F, S, S, 3) uint8 buffer for the preprocessed crop."""
        F = frames.shape[0]
        w, T, dims = self.w, self.T, self.dims
        bf = self._buffers(F)
        self.preprocess(frames, bf["patches"], crop)
        g, C = self.sizes[0], dims[0]
        self._gemm(bf["patches"], w * self.kp, self.kp, self.patch_w, bf["stem"], M=F * T, N=C, bias=self.patch_b)
        h = bf["h"][0]
        for f in range(F):                 # the rows behind a frame's class-token slot -> the dense map
            self._ln(bf["stem"][f * T + 1:], h[f * g * g:], self.stem_ln, rows=g * g, d=C, ldy=C, f32=True)
        if taps is not None and "stem" in taps:
            taps["stem"] = h.view(F, g, g, C).clone()
        for s, st in enumerate(self.stages):
            g, C = self.sizes[s], dims[s]
            M = F * g * g
            if s:
                Cp, Mp = dims[s - 1], 4 * M
                lnf = bf["y"][:Mp * Cp]
                self._ln(h, lnf, st["ds_ln"], rows=Mp, d=Cp, ldy=Cp, f32=True)
                col = bf["col"][:M * 4 * Cp]
                L.im2col(lnf, col, B=F, H=2 * g, W=2 * g, C_=Cp, kh=2, kw=2, stride=2, pad=0, Ho=g, Wo=g, ldo=4 * Cp)
                a = self._operand(col, bf["ff"][:w * M * 4 * Cp], rows=M, d=4 * Cp)
                h = bf["h"][s]
                self._gemm(a, w * 4 * Cp, 4 * Cp, st["ds_w"], h, M=M, N=C, bias=st["ds_b"])
            y, x, ff = bf["y"][:M * C], bf["x"][:w * M * C].view(M, w * C), bf["ff"][:w * M * 4 * C].view(M, w * 4 * C)
            for j, blk in enumerate(st["blocks"]):
                self.dwconv(h, y, blk, F=F, H=g, W=g, C=C)
                self._ln(y, x, blk["ln"], rows=M, d=C, ldy=w * C)
                self._gemm(x, w * C, C, blk["fc1"], ff, M=M, N=4 * C, epilogue=L.EPI_GELU, bias=blk["fc1_b"], out_split=self.split, ldo=w * 4 * C)
                self._gemm(ff, w * 4 * C, 4 * C, blk["fc2"], h, M=M, N=C, epilogue=L.EPI_RESID, bias=blk["fc2_b"], resid=h)
                if taps is not None and (s, j) in taps:
                    taps[(s, j)] = h.view(F, g, g, C).clone()
        # head: mean over the last map's pixels, head.norm, head.proj
        L._launch("convnext_pool_ln", 0.0, 4.0 * F * (g * g + 1) * C,
                  lambda: L.lib().v2a_convnext_pool_ln(h.data_ptr(), g * g * C, F, g * g, C, self.head_ln[0].data_ptr(), self.head_ln[1].data_ptr(),
                                                       self.eps, bf["pooled"].data_ptr(), C, L.stream_ptr()))
        a = self._operand(bf["pooled"], bf["pooled_op"], rows=F, d=C)
        self._gemm(a, w * C, C, self.proj, bf["out"], M=F, N=self.out_dim, bias=self.proj_b)
        return bf["out"]


class MixedImageEncoder:
    """The reference's `video_encoder="mixed"` (x3:1745-1788): the rows of `clip_vit`, `clip_vit2`, `clip_convnext` and `dinov2`, in
    that order, side by side per frame (1280 + 768 + 1024 + 1536 = 4608 wide for the real models), cut to the shortest part.
    `encoders`: a dict with exactly those keys; each value maps uint8 frames (F, H, W, 3) to (F, dim) rows."""

    def __init__(self, encoders: dict):
        if set(encoders) != set(MIXED_ORDER):
            raise ValueError(f"MixedImageEncoder: encoders for {sorted(encoders)}, needs exactly {list(MIXED_ORDER)}")
        self.encoders = {k: encoders[k] for k in MIXED_ORDER}
        self.out_dim = sum(int(e.out_dim) for e in self.encoders.values())

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A directory with one subdirectory per choice (`clip_vit`, `clip_vit2`, `clip_convnext`, `dinov2`), each its model's own."""
        from .e2tts import IMAGE_ENCODERS
        return cls({k: IMAGE_ENCODERS[k].from_pretrained(os.path.join(path, k), device, **kw) for k in MIXED_ORDER})

    def parts(self, frames) -> dict:
        """{choice: (F, dim) rows}, each encoder run on the same frames."""
        return {k: e(frames) for k, e in self.encoders.items()}

    @staticmethod
    def concat(parts: dict) -> torch.Tensor:
        n = min(p.shape[0] for p in parts.values())
        return torch.cat([parts[k][:n].float() for k in MIXED_ORDER], 1)

    def __call__(self, frames) -> torch.Tensor:
        return self.concat(self.parts(frames))
