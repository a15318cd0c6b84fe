"""CLIP ViT image encoder on the HIP kernels of include/v2a_cfm.h: the `video_encoder="clip_vit"` model of the reference
(x3:1423-1425) -- transformers `CLIPImageProcessor()` followed by `CLIPVisionModelWithProjection` loaded from IP-Adapter
`sdxl_models/image_encoder` (OpenCLIP ViT-bigG/14) -- which turns every decoded video frame into one `image_embeds` row
(x3:1714, 1733-1735).

Preprocessing runs on the GPU and equals the processor's Pillow path bit for bit: the shortest edge is resized to the image
size with Pillow's BICUBIC (two separable passes of 22-bit fixed-point integer sums, the intermediate clipped to uint8, the
filter widened by the downscale factor), the centre is cropped, and every byte is mapped through a host table of the
processor's fp32 rescale / normalise.  The integer coefficient tables are built here in double precision with the expressions
of Pillow's `precompute_coeffs` / `normalize_coeffs_8bpc`.

Compute modes: `"fp32"` -- exact-fp32 MFMA GEMMs; `"bf16x3"` -- every GEMM operand as hi | lo bf16 planes (three bf16 MFMA
products per fp32 product, fp32 accumulate).  LayerNorm, attention and the residual stream are fp32 in both.  Every layer is
computed on all tokens (no CLS-only shortcut in the last layer).
"""
from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib as L

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit resample
_PREFIXES = ("image_encoder.",)
# bf16x3 tile of every GEMM pinned (the 256x256 8-phase kernel, three products per 32-wide K stage): the summation order of a split GEMM depends on
# the kernel, and a by-shape choice would make a frame's result depend on how many frames share its chunk
_SPLIT_TILE = 5


# ---- Pillow BICUBIC coefficients (host, double precision) ---------------------------------------
def _bicubic(x: float) -> float:
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_coeffs(in_size: int, out_size: int) -> tuple[np.ndarray, np.ndarray]:
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for BICUBIC over the box (0, in_size):
    bounds (out_size, 2) int32 = (first input pixel, taps), coef (out_size, ksize) int32 with 22 fraction bits."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            coef[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coef


def resize_output_size(h: int, w: int, size: int) -> tuple[int, int]:
    """transformers get_resize_output_image_size(default_to_square=False): shortest edge -> size, long edge int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


class ResizePlan:
    """Host tables of one input size: the crop columns of the horizontal pass, the input rows it covers and the crop rows of the
    vertical pass (bounds relative to the first covered row).  `resize`: the shortest-edge target when it differs from the crop S
    (DINOv2's processor resizes to 256 and crops 224; CLIP's resizes to the crop size, the default)."""

    def __init__(self, H: int, W: int, S: int, resize: int | None = None):
        self.H, self.W, self.S = H, W, S
        self.resize = S if resize is None else int(resize)
        if self.resize < S:
            raise ValueError(f"ResizePlan: resize {self.resize} below the crop {S} (the processor would pad)")
        oh, ow = resize_output_size(H, W, self.resize)
        self.out_hw = (oh, ow)
        self.top, self.left = (oh - S) // 2, (ow - S) // 2
        hb, hk = resample_coeffs(W, ow)
        vb, vk = resample_coeffs(H, oh)
        self.hb, self.hk = hb[self.left:self.left + S].copy(), hk[self.left:self.left + S].copy()
        vb, vk = vb[self.top:self.top + S].copy(), vk[self.top:self.top + S].copy()
        self.y0 = int(vb[:, 0].min())
        self.rows = int((vb[:, 0] + vb[:, 1]).max()) - self.y0
        vb[:, 0] -= self.y0
        self.vb, self.vk = vb, vk
        # the kernels read what the tables say: every tap must lie inside the image (checked here, the device cannot)
        assert (self.hb[:, 0] >= 0).all() and (self.hb[:, 0] + self.hb[:, 1] <= W).all()
        assert (self.vb[:, 0] >= 0).all() and (self.vb[:, 0] + self.vb[:, 1] <= self.rows).all() and self.y0 + self.rows <= H

    def resize_numpy(self, img: np.ndarray) -> np.ndarray:
        """The two integer passes on the host, (H, W, 3) uint8 -> the (S, S, 3) uint8 crop: the restatement the kernels follow."""
        x = img.astype(np.int64)
        rows = x[self.y0:self.y0 + self.rows]
        tmp = np.empty((self.rows, self.S, 3), np.int64)
        for j in range(self.S):
            x0, n = self.hb[j]
            tmp[:, j] = ((rows[:, x0:x0 + n] * self.hk[j, :n, None]).sum(1) + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
        tmp = np.clip(tmp, 0, 255)
        out = np.empty((self.S, self.S, 3), np.int64)
        for i in range(self.S):
            y0, n = self.vb[i]
            out[i] = ((tmp[y0:y0 + n] * self.vk[i, :n, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
        return np.clip(out, 0, 255).astype(np.uint8)


def normalize_table(mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD) -> np.ndarray:
    """(3, 256) float32: the processor's value of byte u in channel c -- rescale in float64 then cast (transformers `rescale`),
    normalise in float32 (`normalize`)."""
    u = np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1)
    x = (u.astype(np.float64) * (1 / 255)).astype(np.float32)
    y = (x - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32)
    return np.ascontiguousarray(y.T.astype(np.float32))


# ---- weights ---------------------------------------------------------------------------------------------
def strip_keys(state_dict) -> dict[str, torch.Tensor]:
    """Plain CLIPVisionModelWithProjection keys from such a state dict or a reference checkpoint's `image_encoder.*`."""
    sd = state_dict.get("model_state_dict", state_dict) if isinstance(state_dict, dict) else state_dict
    if any(k.startswith(_PREFIXES) for k in sd):
        return {k[len(p):]: v for k, v in sd.items() for p in _PREFIXES if k.startswith(p)}
    return dict(sd)


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


class CLIPImageEncoder:
    """`CLIPImageProcessor()` + `CLIPVisionModelWithProjection` (image_embeds) on the HIP kernels.

    `CLIPImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32)`: plain CLIPVisionModelWithProjection keys or a
    reference checkpoint's `image_encoder.*`; config = a dict of CLIPVisionConfig fields (inferred from the shapes when absent).
    `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, projection_dim) float32 on the device, `chunk` frames per pass (a frame's
    result does not depend on its chunk)."""

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32):
        sd = strip_keys(state_dict)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        if cfg.get("hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"CLIPImageEncoder: hidden_act {cfg['hidden_act']!r} (only the exact-erf 'gelu' is supported)")
        if compute not in ("fp32", "bf16x3"):
            raise ValueError(f"CLIPImageEncoder: compute {compute!r} (fp32 or bf16x3)")
        d, H, P, S = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["image_size"]
        if d % H or (d // H) % 4 or d // H > 112 or d % 4 or cfg["intermediate_size"] % 64 or S % P:
            raise ValueError(f"CLIPImageEncoder: hidden {d} / heads {H} / mlp {cfg['intermediate_size']} / image {S} / patch {P} "
                             "(head dim a multiple of 4 up to 112, mlp width a multiple of 64)")
        if int(chunk) < 1:
            raise ValueError("CLIPImageEncoder: chunk >= 1")
        self.cfg, self.compute, self.chunk = cfg, compute, int(chunk)
        self.device = torch.device(device)
        self.d, self.H, self.P, self.S = d, H, P, S
        self.dh = d // H
        self.g = S // P
        self.T = 1 + self.g * self.g
        self.kp = (3 * P * P + 63) // 64 * 64            # patch K zero-padded to a multiple of 64
        self.dp = (d + 63) // 64 * 64                    # K of the hidden-width GEMM operands, zero-padded likewise
        self.split = compute == "bf16x3"
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        dev = lambda t: t.contiguous().to(self.device)
        wmat = lambda t: dev(L.split_planes(t) if self.split else t.float())       # GEMM weight in the mode's layout
        padk = lambda t: torch.nn.functional.pad(t, (0, self.dp - t.shape[1]))    # zero K columns up to dp
        E = "vision_model.embeddings."
        pw = torch.zeros(d, self.kp)
        pw[:, :3 * P * P] = f32(E + "patch_embedding.weight").reshape(d, 3 * P * P)
        self.patch_w = wmat(pw)
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
        self._plans: dict[tuple, tuple] = {}
        self._bufs: dict[int, dict] = {}
        L.lib()

    def to(self, device):
        """Move the weights to `device`; chunk buffers and resize tables are rebuilt there on first use."""
        self.device = torch.device(device)
        mv = lambda t: t.to(self.device)
        for k in ("patch_w", "cls", "pos", "proj", "lut"):
            setattr(self, k, mv(getattr(self, k)))
        self.pre_ln, self.post_ln = tuple(map(mv, self.pre_ln)), tuple(map(mv, self.post_ln))
        self.layers = [{k: (tuple(map(mv, v)) if isinstance(v, tuple) else mv(v)) for k, v in Lw.items()} for Lw in self.layers]
        self._plans, self._bufs = {}, {}
        return self

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A local HF directory (IP-Adapter sdxl_models/image_encoder): config.json + model.safetensors or pytorch_model.bin."""
        with open(os.path.join(path, "config.json")) as f:
            hc = json.load(f)
        hc = hc.get("vision_config", hc)
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
        keys = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                "projection_dim", "layer_norm_eps", "hidden_act", "num_channels")
        return cls(sd, device, config={k: hc[k] for k in keys if k in hc}, **kw)

    # ---- device pieces -----------------------------------------------------------------------------
    def _plan(self, H: int, W: int):
        key = (H, W)
        pl = self._plans.get(key)
        if pl is None:
            rp = ResizePlan(H, W, self.S)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            pl = (rp, t(rp.hb), t(rp.hk), t(rp.vb), t(rp.vk))
            self._plans[key] = pl
        return pl

    def _buffers(self, F: int) -> dict:
        bf = self._bufs.get(F)
        if bf is None:
            M, d, dff = F * self.T, self.d, self.cfg["intermediate_size"]
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
            w = 2 if self.split else 1
            adt = torch.bfloat16 if self.split else torch.float32
            z = lambda *s: torch.zeros(*s, dtype=adt, device=self.device)      # K pad columns (dp > d) stay zero
            dp = self.dp
            bf = dict(h=e(M, d), qkv=e(M, 3 * d), x=z(M, w * dp), ao=z(M, w * dp), ff=e(M, w * dff, dt=adt),
                      emb=e(M, d), pooled=z(F, w * dp), out=e(F, self.cfg["projection_dim"]),
                      patches=torch.zeros(M, w * self.kp, dtype=adt, device=self.device))   # class rows and pad columns stay zero
            self._bufs = {F: bf}           # one live chunk size
        return bf

    def _gemm(self, a, lda, k, w, out, *, M, N, epilogue=L.EPI_STORE, bias=None, resid=None, out_split=False, ldo=None):
        if self.split:
            L.gemm([(a, lda, k)], w, out, M=M, N=N, compute=L.BF16, epilogue=epilogue, bias=bias, resid=resid, a_split=True,
                   out_split=out_split, ldo=ldo, tile_hint=_SPLIT_TILE)
        else:
            L.gemm([(a, lda, k)], w, out, M=M, N=N, compute=L.F32, epilogue=epilogue, bias=bias, resid=resid, ldo=ldo)

    def preprocess(self, frames: torch.Tensor, patches: torch.Tensor, crop: torch.Tensor | None = None):
        """frames (F, H, W, 3) uint8 on the device -> the patch matrix (and optionally the uint8 crop)."""
        F, H, W, _ = frames.shape
        rp, hb, hk, vb, vk = self._plan(H, W)
        tmp = torch.empty(F, rp.rows, self.S, 3, dtype=torch.uint8, device=self.device)
        lib, s = L.lib(), L.stream_ptr()
        L.check(lib.v2a_clip_resize_h(frames.data_ptr(), F, H, W, tmp.data_ptr(), rp.y0, rp.rows, self.S, hb.data_ptr(), hk.data_ptr(),
                                      hk.shape[1], s))
        L.check(lib.v2a_clip_resize_v(tmp.data_ptr(), F, rp.rows, self.S, self.P, vb.data_ptr(), vk.data_ptr(), vk.shape[1],
                                      self.lut.data_ptr(), patches.data_ptr(), patches.stride(0), L.BF16_SPLIT if self.split else L.F32,
                                      self.kp if self.split else 0, L._p(crop), s))

    def layernorm(self, x, y, ln, *, rows, ldx=None):
        L.check(L.lib().v2a_clip_layernorm(x.data_ptr(), ldx or self.d, y.data_ptr(), y.stride(0), L.BF16_SPLIT if self.split else L.F32,
                                           rows, self.d, ln[0].data_ptr(), ln[1].data_ptr(), float(self.cfg["layer_norm_eps"]),
                                           L.stream_ptr()))

    def attention(self, qkv, out, F: int):
        a = L.ClipAttnArgs()
        d = self.d
        a.q, a.k, a.v, a.out = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, out.data_ptr()
        a.row_stride, a.batch_stride = 3 * d, self.T * 3 * d
        a.out_row_stride, a.out_batch_stride = out.stride(0), self.T * out.stride(0)
        a.B, a.H, a.N, a.d_head = F, self.H, self.T, self.dh
        a.scale, a.out_split = self.dh ** -0.5, 1 if self.split else 0
        L.check(L.lib().v2a_clip_attention(ctypes.byref(a), L.stream_ptr()))

    @torch.no_grad()
    def encode_chunk(self, frames: torch.Tensor, *, taps: dict | None = None, crop: torch.Tensor | None = None) -> torch.Tensor:
        """One chunk: frames (F, H, W, 3) uint8 on the device -> (F, projection_dim) float32 (a view of a reused buffer).
        `taps`: dict whose keys are layer numbers 1..L; each receives a device copy of the residual stream (F, T, d) after that
        layer.  `crop`: optional (F, S, S, 3) uint8 buffer for the preprocessed crop."""
        F = frames.shape[0]
        M, d, dp, dff, T = F * self.T, self.d, self.dp, self.cfg["intermediate_size"], self.T
        bf = self._buffers(F)
        h, qkv, x, ao, ff, emb = bf["h"], bf["qkv"], bf["x"], bf["ao"], bf["ff"], bf["emb"]
        w = 2 if self.split else 1
        self.preprocess(frames, bf["patches"], crop)
        L.check(L.lib().v2a_clip_embed_init(emb.data_ptr(), d, M, T, d, self.cls.data_ptr(), self.pos.data_ptr(), L.stream_ptr()))
        self._gemm(bf["patches"], w * self.kp, self.kp, self.patch_w, emb, M=M, N=d, epilogue=L.EPI_RESID, resid=emb)
        # pre_layrnorm: fp32 into the residual stream
        L.check(L.lib().v2a_clip_layernorm(emb.data_ptr(), d, h.data_ptr(), d, L.F32, M, d, self.pre_ln[0].data_ptr(),
                                           self.pre_ln[1].data_ptr(), float(self.cfg["layer_norm_eps"]), L.stream_ptr()))
        for li, Lw in enumerate(self.layers):
            self.layernorm(h, x, Lw["ln1"], rows=M)
            self._gemm(x, w * dp, dp, Lw["qkv"], qkv, M=M, N=3 * d, bias=Lw["qkv_b"])
            self.attention(qkv, ao, F)
            self._gemm(ao, w * dp, dp, Lw["o"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=h)
            self.layernorm(h, x, Lw["ln2"], rows=M)
            self._gemm(x, w * dp, dp, Lw["fc1"], ff, M=M, N=dff, epilogue=L.EPI_GELU, bias=Lw["fc1_b"], out_split=self.split,
                       ldo=w * dff)
            self._gemm(ff, w * dff, dff, Lw["fc2"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=h)
            if taps is not None and li + 1 in taps:
                taps[li + 1] = h.view(F, T, d).clone()
        # post_layernorm on the class rows (row stride T * d), visual_projection (no bias)
        self.layernorm(h, bf["pooled"], self.post_ln, rows=F, ldx=T * d)
        self._gemm(bf["pooled"], w * dp, dp, self.proj, bf["out"], M=F, N=self.cfg["projection_dim"])
        return bf["out"]

    @torch.no_grad()
    def __call__(self, frames) -> torch.Tensor:
        """frames: uint8 (F, H, W, 3) RGB array or tensor -> image_embeds (F, projection_dim) float32 on the device."""
        fr = torch.as_tensor(np.asarray(frames)) if not torch.is_tensor(frames) else frames
        if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[-1] != 3:
            raise ValueError(f"CLIPImageEncoder: frames must be uint8 (F, H, W, 3), got {tuple(fr.shape)} {fr.dtype}")
        F = fr.shape[0]
        out = torch.empty(F, self.cfg["projection_dim"], dtype=torch.float32, device=self.device)
        for i in range(0, F, self.chunk):
            part = fr[i:i + self.chunk].to(self.device).contiguous()
            out[i:i + part.shape[0]] = self.encode_chunk(part)
        return out
