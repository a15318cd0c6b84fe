"""DINOv2 image encoder on the HIP kernels of include/v2a_cfm.h: the `video_encoder="dinov2"` model of the reference
(x3:1432-1433) -- transformers `AutoImageProcessor` (a `BitImageProcessor`: shortest edge to 256, centre crop 224, ImageNet
mean / std, BICUBIC) followed by `AutoModel` of dinov2-giant (`Dinov2Model`, ViT-g/14: 40 layers, d = 1536, 24 heads of 64, SwiGLU
feed-forward with 4096 hidden values, LayerScale) -- which turns every decoded video frame into one `pooler_output` row
(x3:1714, 1742-1744).

Preprocessing is clip.py's: Pillow's integer BICUBIC on host tables (`ResizePlan`, here with a resize target that differs from
the crop), the processor's rescale / normalise as a byte table, both on the kernels `v2a_clip_resize_h/_v`.

Prepared on the host at load time: the position table interpolated to the crop's grid with the library's own call
(`Dinov2Embeddings.interpolate_pos_encoding`: F.interpolate, bicubic, align_corners=False, float32), the patch bias folded into its
patch rows, LayerScale folded into the `dense` / `weights_out` (`fc2`) weights and biases in float64 before rounding or
splitting, and `weights_in` regrouped [16 value | 16 gate] for the SWIGLU epilogue of v2a_gemm (gate = x1, value = x2).

Compute modes as in clip.py: `"fp32"` -- exact-fp32 MFMA GEMMs; `"bf16x3"` -- every GEMM operand and the attention products as
hi | lo bf16 planes.  LayerNorm, softmax and the residual stream are fp32 in both.  Attention runs on the MFMA kernels of
v2a_attention (64-wide heads, no gate, no clamp), reading the fused qkv buffer in place.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import _lib as L
from .clip import _SPLIT_TILE, ResizePlan, normalize_table, strip_keys

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PIL_BICUBIC = 3
_CFG_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size", "layer_norm_eps", "use_swiglu_ffn",
             "num_channels")
# v2a_attention picks the key-split form of its split-operand kernel while a launch has fewer workgroups than this and more than
# 128 keys; that form sums a row's keys in another order (see DINOv2ImageEncoder._attn_frames)
_ATTN_KEY_SPLIT_BELOW = 200


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


class DINOv2ImageEncoder:
    """`BitImageProcessor` + `Dinov2Model` (pooler_output) on the HIP kernels.

    `DINOv2ImageEncoder(state_dict, device, config=None, compute="bf16x3", chunk=32, resize=256, crop=224, image_mean=IMAGENET,
    image_std=IMAGENET)`: plain Dinov2Model keys or a reference checkpoint's `image_encoder.*`; config = a dict of Dinov2Config fields
    (inferred from the shapes when absent).  `__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, hidden_size) float32 on the device,
    `chunk` frames per pass (a frame's result does not depend on its chunk)."""

    def __init__(self, state_dict, device, config: dict | None = None, compute: str = "bf16x3", chunk: int = 32, resize: int = 256,
                 crop: int = 224, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD):
        sd = strip_keys(state_dict)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        if compute not in ("fp32", "bf16x3"):
            raise ValueError(f"DINOv2ImageEncoder: compute {compute!r} (fp32 or bf16x3)")
        d, H, P = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
        if d % H or d // H != 64:
            raise ValueError(f"DINOv2ImageEncoder: hidden {d} / heads {H}: the attention kernels take 64-wide heads only")
        if int(chunk) < 1:
            raise ValueError("DINOv2ImageEncoder: chunk >= 1")
        if int(crop) % P or int(resize) < int(crop):
            raise ValueError(f"DINOv2ImageEncoder: crop {crop} must be a multiple of the patch size {P} and resize {resize} >= crop")
        self.cfg, self.compute, self.chunk = cfg, compute, int(chunk)
        self.device = torch.device(device)
        self.d, self.H, self.P, self.S, self.resize = d, H, P, int(crop), int(resize)
        self.dh = 64
        self.g = self.S // P
        self.T = 1 + self.g * self.g
        self.kp = (cfg["num_channels"] * P * P + 63) // 64 * 64            # patch K zero-padded to a multiple of 64
        self.split = compute == "bf16x3"
        self.swiglu = bool(cfg["use_swiglu_ffn"])
        self.f32_attention = "v2a_attention"         # fp32 mode: "v2a_attention" (MFMA, V2A_F32) or "v2a_clip_attention" (VALU)
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        dev = lambda t: t.contiguous().to(self.device)
        wmat = lambda t: dev(L.split_planes(t) if self.split else t.float())       # GEMM weight in the mode's layout
        E = "embeddings."
        kin = cfg["num_channels"] * P * P
        pw = torch.zeros(d, self.kp)
        pw[:, :kin] = f32(E + "patch_embeddings.projection.weight").reshape(d, kin)
        self.patch_w = wmat(pw)
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
                o=wmat(o_w), o_b=dev(o_b),
                ln2=(dev(f32(p + "norm2.weight")), dev(f32(p + "norm2.bias"))),
                fc1=wmat(w1), fc1_b=dev(b1), fc2=wmat(w2), fc2_b=dev(b2)))
        self.dff = w2.shape[1]                       # hidden values of the feed-forward (K of its second Linear)
        if self.dff % 64:
            raise ValueError(f"DINOv2ImageEncoder: feed-forward width {self.dff} must be a multiple of 64")
        self.lut = dev(torch.from_numpy(normalize_table(image_mean, image_std)))
        self._plans: dict[tuple, tuple] = {}
        self._bufs: dict[int, dict] = {}
        L.lib()

    def to(self, device):
        """Move the weights to `device`; chunk buffers and resize tables are rebuilt there on first use."""
        self.device = torch.device(device)
        mv = lambda t: t.to(self.device)
        for k in ("patch_w", "cls", "pos", "lut"):
            setattr(self, k, mv(getattr(self, k)))
        self.final_ln = tuple(map(mv, self.final_ln))
        self.layers = [{k: (tuple(map(mv, v)) if isinstance(v, tuple) else mv(v)) for k, v in Lw.items()} for Lw in self.layers]
        self._plans, self._bufs = {}, {}
        return self

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A local HF directory (facebook/dinov2-giant): config.json, preprocessor_config.json (size.shortest_edge, crop_size,
        image_mean / image_std; a resample other than BICUBIC is refused), model.safetensors or pytorch_model.bin."""
        with open(os.path.join(path, "config.json")) as f:
            hc = json.load(f)
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
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
        return cls(sd, device, config={k: hc[k] for k in _CFG_KEYS if k in hc}, **kw)

    # ---- device pieces -----------------------------------------------------------------------------
    def _plan(self, H: int, W: int):
        key = (H, W)
        pl = self._plans.get(key)
        if pl is None:
            rp = ResizePlan(H, W, self.S, self.resize)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            pl = (rp, t(rp.hb), t(rp.hk), t(rp.vb), t(rp.vk))
            self._plans[key] = pl
        return pl

    def _attn_frames(self, F: int) -> int:
        """Frames one attention launch covers.  v2a_attention chooses between two forms of its split-operand kernel by the launch's
        workgroup count, and they sum a row's keys in different orders: a launch is never left below that count, so that a frame's
        result does not depend on its chunk.  The rows behind the chunk are zero, and their outputs are not read."""
        if not self.split or self.T <= 128:
            return F
        per_frame = self.H * ((self.T + 63) // 64)
        return max(F, (_ATTN_KEY_SPLIT_BELOW + per_frame - 1) // per_frame)

    def _buffers(self, F: int) -> dict:
        bf = self._bufs.get(F)
        if bf is None:
            M, Ma, d, dff = F * self.T, self._attn_frames(F) * self.T, self.d, self.dff
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
            w = 2 if self.split else 1
            adt = torch.bfloat16 if self.split else torch.float32
            bf = dict(h=e(M, d), qkv=torch.zeros(Ma, 3 * d, device=self.device), x=e(M, w * d, dt=adt),
                      ao=torch.zeros(Ma, w * d, dtype=adt, device=self.device), ff=e(M, w * dff, dt=adt), out=e(F, d),
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

    def layernorm(self, x, y, ln, *, rows, ldx=None, y_dtype=None):
        ydt = (L.BF16_SPLIT if self.split else L.F32) if y_dtype is None else y_dtype
        L.check(L.lib().v2a_clip_layernorm(x.data_ptr(), ldx or self.d, y.data_ptr(), y.stride(0), ydt, rows, self.d, ln[0].data_ptr(),
                                           ln[1].data_ptr(), float(self.cfg["layer_norm_eps"]), L.stream_ptr()))

    def attention(self, qkv, out, F: int):
        """softmax(q k^T / 8) v per frame and head on the fused qkv rows, into the out-projection's operand."""
        d, T = self.d, self.T
        if not self.split and self.f32_attention == "v2a_clip_attention":
            import ctypes
            a = L.ClipAttnArgs()
            a.q, a.k, a.v, a.out = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, out.data_ptr()
            a.row_stride, a.batch_stride = 3 * d, T * 3 * d
            a.out_row_stride, a.out_batch_stride = out.stride(0), T * out.stride(0)
            a.B, a.H, a.N, a.d_head = F, self.H, T, 64
            a.scale, a.out_split = 0.125, 0
            L.check(L.lib().v2a_clip_attention(ctypes.byref(a), L.stream_ptr()))
            return
        B = self._attn_frames(F)
        ors = out.stride(0)
        L.attention(qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, None, out.data_ptr(),
                    strides=(3 * d, 3 * d, 3 * d, 0, ors, T * 3 * d, T * 3 * d, T * 3 * d, 0, T * ors), B=B, H=self.H, Nq=T, Nk=T,
                    scale=0.125, softclamp=0.0, dtype=L.BF16_SPLIT if self.split else L.F32, out_split=self.split)

    @torch.no_grad()
    def encode_chunk(self, frames: torch.Tensor, *, taps: dict | None = None, crop: torch.Tensor | None = None) -> torch.Tensor:
        """One chunk: frames (F, H, W, 3) uint8 on the device -> (F, hidden_size) float32 (a view of a reused buffer).
        `taps`: dict whose keys are layer numbers 1..L; each receives a device copy of the residual stream (F, T, d) after that
        layer.  `crop`: optional (F, S, S, 3) uint8 buffer for the preprocessed crop."""
        F = frames.shape[0]
        M, d, dff, T = F * self.T, self.d, self.dff, self.T
        bf = self._buffers(F)
        h, qkv, x, ao, ff = bf["h"], bf["qkv"], bf["x"], bf["ao"], bf["ff"]
        w = 2 if self.split else 1
        self.preprocess(frames, bf["patches"], crop)
        # embeddings straight into the residual stream (no pre-LayerNorm): class / position rows, then the patch GEMM adds onto them
        L.check(L.lib().v2a_clip_embed_init(h.data_ptr(), d, M, T, d, self.cls.data_ptr(), self.pos.data_ptr(), L.stream_ptr()))
        self._gemm(bf["patches"], w * self.kp, self.kp, self.patch_w, h, M=M, N=d, epilogue=L.EPI_RESID, resid=h)
        for li, Lw in enumerate(self.layers):
            self.layernorm(h, x, Lw["ln1"], rows=M)
            self._gemm(x, w * d, d, Lw["qkv"], qkv, M=M, N=3 * d, bias=Lw["qkv_b"])
            self.attention(qkv, ao, F)
            self._gemm(ao, w * d, d, Lw["o"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=h)      # LayerScale 1 folded
            self.layernorm(h, x, Lw["ln2"], rows=M)
            if self.swiglu:
                self._gemm(x, w * d, d, Lw["fc1"], ff, M=M, N=2 * dff, epilogue=L.EPI_SWIGLU, bias=Lw["fc1_b"], out_split=self.split,
                           ldo=w * dff)
            else:
                self._gemm(x, w * d, d, Lw["fc1"], ff, M=M, N=dff, epilogue=L.EPI_GELU, bias=Lw["fc1_b"], out_split=self.split, ldo=w * dff)
            self._gemm(ff, w * dff, dff, Lw["fc2"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=h)  # LayerScale 2 folded
            if taps is not None and li + 1 in taps:
                taps[li + 1] = h.view(F, T, d).clone()
        # pooler_output: the final layernorm on the class rows (row stride T * d); no projection
        self.layernorm(h, bf["out"], self.final_ln, rows=F, ldx=T * d, y_dtype=L.F32)
        return bf["out"]

    @torch.no_grad()
    def __call__(self, frames) -> torch.Tensor:
        """frames: uint8 (F, H, W, 3) RGB array or tensor -> pooler_output (F, hidden_size) float32 on the device."""
        fr = torch.as_tensor(np.asarray(frames)) if not torch.is_tensor(frames) else frames
        if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[-1] != 3:
            raise ValueError(f"DINOv2ImageEncoder: frames must be uint8 (F, H, W, 3), got {tuple(fr.shape)} {fr.dtype}")
        F = fr.shape[0]
        out = torch.empty(F, self.d, dtype=torch.float32, device=self.device)
        for i in range(0, F, self.chunk):
            part = fr[i:i + self.chunk].to(self.device).contiguous()
            out[i:i + part.shape[0]] = self.encode_chunk(part)
        return out
