"""The ViT image-encoder engine on the HIP kernels of include/v2a_cfm.h that clip.py and dinov2.py both are: an image processor
(shortest-edge BICUBIC resize, centre crop, rescale / normalise) followed by a pre-norm vision transformer, one output row per
frame.

Preprocessing runs on the GPU and equals the processor's Pillow path bit for bit (resample.py holds the host tables; the kernels
are `v2a_clip_resize_h/_v`).  The embedding is `v2a_clip_embed_init` (class / position rows) plus the patch GEMM added onto it;
every layer is LayerNorm, fused qkv GEMM, attention, out-projection onto the residual stream, LayerNorm, and a two-GEMM
feed-forward onto the residual stream, computed on all tokens.

Compute modes: `"fp32"` -- exact-fp32 MFMA GEMMs; `"bf16x3"` -- every GEMM operand as hi | lo bf16 planes (three bf16 MFMA
products per fp32 product, fp32 accumulate).  LayerNorm, softmax and the residual stream are fp32 in both.

A model states what is its own: the geometry and feed-forward epilogue it hands to `__init__`, its prepared weights (`patch_w`,
`cls`, `pos`, `lut`, optionally `pre_ln`, and `layers`: one dict `ln1, qkv, qkv_b, o, o_b, ln2, fc1, fc1_b, fc2, fc2_b` per
layer), `head`, and its attention: the VALU kernel `v2a_clip_attention` (any head width up to 112), or -- `mfma_attention = True`, 64-wide
heads only -- the MFMA kernels of `v2a_attention` together with the floor on the workgroups of a launch (`_attn_frames`).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L
from .resample import ResizePlan
from .weights import read_hf_dir

# bf16x3 tile of every GEMM pinned (the 256x256 8-phase kernel, three products per 32-wide K stage): the summation order of a split GEMM depends on
# the kernel, and a by-shape choice would make a frame's result depend on how many frames share its chunk
_SPLIT_TILE = 5
# v2a_attention picks the key-split form of its split-operand kernel while a launch has fewer workgroups than this and more than
# 128 keys; that form sums a row's keys in another order (see ViTImageEncoder._attn_frames)
_ATTN_KEY_SPLIT_BELOW = 200


class ViTImageEncoder:
    """`__call__(frames)`: uint8 (F, H, W, 3) RGB -> (F, out_dim) float32 on the device, `chunk` frames per pass (a frame's result
    does not depend on its chunk)."""

    _CFG_KEYS: tuple[str, ...] = ()      # the config.json fields from_pretrained hands to the constructor
    pre_ln = None                        # (weight, bias) of a LayerNorm between the embeddings and the first layer, if the model has one
    mfma_attention = False               # True: v2a_attention (MFMA, 64-wide heads; bf16x3: its products on hi | lo planes too), False: v2a_clip_attention
    f32_attention = "v2a_attention"      # with mfma_attention, the fp32 mode's kernel: "v2a_attention" (MFMA, V2A_F32) or "v2a_clip_attention" (VALU)
    crop_offset = "floor"                # ResizePlan's: the transformers processors' (h - S) // 2, or "torchvision" (convnext.py)

    def __init__(self, cfg: dict, device, compute: str, chunk: int, *, S: int, resize: int, kin: int, dp: int, dff: int, ffn: tuple[int, int],
                 out_dim: int):
        """S: the crop (image) size, resize: the shortest-edge target before the crop, kin: values per patch, dp: K of the
        hidden-width GEMM operands (d, or d zero-padded), dff: hidden values of the feed-forward, ffn: (epilogue, N) of its first
        GEMM, out_dim: width of an output row."""
        name = type(self).__name__
        if compute not in ("fp32", "bf16x3"):
            raise ValueError(f"{name}: compute {compute!r} (fp32 or bf16x3)")
        if int(chunk) < 1:
            raise ValueError(f"{name}: chunk >= 1")
        self.cfg, self.compute, self.chunk = cfg, compute, int(chunk)
        self.device = torch.device(device)
        self.d, self.H, self.P = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
        self.S, self.resize = int(S), int(resize)
        self.dh = self.d // self.H
        self.g = self.S // self.P
        self.T = 1 + self.g * self.g
        self.kp = (kin + 63) // 64 * 64                  # patch K zero-padded to a multiple of 64
        self.dp, self.dff, self.ffn, self.out_dim = dp, dff, ffn, out_dim
        self.eps = float(cfg["layer_norm_eps"])
        self.split = compute == "bf16x3"
        self.w = 2 if self.split else 1                  # planes per GEMM operand row
        self.adt = torch.bfloat16 if self.split else torch.float32
        self.ydt = L.BF16_SPLIT if self.split else L.F32
        self._plans: dict[tuple, tuple] = {}
        self._bufs: dict[int, dict] = {}
        L.lib()

    # ---- weights ------------------------------------------------------------------------------------
    def _dev(self, t):
        return t.contiguous().to(self.device)

    def _wmat(self, t):
        """A GEMM weight in the mode's layout."""
        return self._dev(L.split_planes(t) if self.split else t.float())

    def _patch_weight(self, w):
        """The patch convolution's (d, C, P, P) weight as the patch GEMM's, K zero-padded to kp."""
        pw = torch.zeros(self.d, self.kp)
        pw[:, :w[0].numel()] = w.reshape(self.d, -1)
        return self._wmat(pw)

    def to(self, device):
        """Move the weights to `device`; chunk buffers and resize tables are rebuilt there on first use."""
        self.device = torch.device(device)

        def mv(v):
            if torch.is_tensor(v):
                return v.to(self.device)
            if isinstance(v, (tuple, list)):
                return type(v)(map(mv, v))
            return {k: mv(x) for k, x in v.items()} if isinstance(v, dict) else v

        self._plans, self._bufs = {}, {}
        for k, v in list(vars(self).items()):
            if k != "cfg":
                setattr(self, k, mv(v))
        return self

    @classmethod
    def from_pretrained(cls, path: str, device, **kw):
        """A local HF directory: config.json + model.safetensors or pytorch_model.bin."""
        hc, sd = read_hf_dir(path)
        hc = hc.get("vision_config", hc)
        return cls(sd, device, config={k: hc[k] for k in cls._CFG_KEYS if k in hc}, **kw)

    # ---- device pieces -----------------------------------------------------------------------------
    def _plan(self, H: int, W: int):
        key = (H, W)
        pl = self._plans.get(key)
        if pl is None:
            rp = ResizePlan(H, W, self.S, self.resize, crop_offset=self.crop_offset)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            pl = (rp, t(rp.hb), t(rp.hk), t(rp.vb), t(rp.vk))
            self._plans[key] = pl
        return pl

    def _attn_frames(self, F: int) -> int:
        """Frames one attention launch covers (the qkv / ao buffers hold that many); the rows behind the chunk stay zero, and their
        outputs are not read.  v2a_attention chooses between two forms of its split-operand kernel by the launch's workgroup count, and
        they sum a row's keys in different orders: a launch is never left below that count, so that a frame's result does not depend
        on its chunk."""
        if not self.mfma_attention or not self.split or self.T <= 128:
            return F
        per_frame = self.H * ((self.T + 63) // 64)
        return max(F, (_ATTN_KEY_SPLIT_BELOW + per_frame - 1) // per_frame)

    def _head_buffers(self, F: int) -> dict:
        return {}

    def _buffers(self, F: int) -> dict:
        bf = self._bufs.get(F)
        if bf is None:
            M, Ma, d, w = F * self.T, self._attn_frames(F) * self.T, self.d, self.w
            e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
            z = lambda *s, dt=self.adt: torch.zeros(*s, dtype=dt, device=self.device)
            # zeroed: the K pad columns (dp > d) of x and ao, the rows of qkv and ao behind the chunk, the class rows and pad columns of patches
            bf = dict(h=e(M, d), qkv=z(Ma, 3 * d, dt=torch.float32), x=z(M, w * self.dp), ao=z(Ma, w * self.dp),
                      ff=e(M, w * self.dff, dt=self.adt), out=e(F, self.out_dim), patches=z(M, w * self.kp))
            if self.pre_ln is not None:
                bf["emb"] = e(M, d)
            bf.update(self._head_buffers(F))
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
                                      self.lut.data_ptr(), patches.data_ptr(), patches.stride(0), self.ydt,
                                      self.kp if self.split else 0, L._p(crop), s))

    def layernorm(self, x, y, ln, *, rows, ldx=None, y_dtype=None):
        """LayerNorm of `rows` rows of x (row stride ldx, default d) into y: a GEMM operand in the mode's layout, or `y_dtype`."""
        L.check(L.lib().v2a_clip_layernorm(x.data_ptr(), ldx or self.d, y.data_ptr(), y.stride(0), self.ydt if y_dtype is None else y_dtype,
                                           rows, self.d, ln[0].data_ptr(), ln[1].data_ptr(), self.eps, L.stream_ptr()))

    def attention(self, qkv, out, F: int):
        """softmax(q k^T / sqrt(dh)) v per frame and head on the fused qkv rows (read in place), into the out-projection's operand."""
        d, T = self.d, self.T
        if self.mfma_attention and (self.split or self.f32_attention != "v2a_clip_attention"):
            ors = out.stride(0)
            L.attention(qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, None, out.data_ptr(),
                        strides=(3 * d, 3 * d, 3 * d, 0, ors, T * 3 * d, T * 3 * d, T * 3 * d, 0, T * ors), B=self._attn_frames(F), H=self.H,
                        Nq=T, Nk=T, scale=self.dh ** -0.5, softclamp=0.0, dtype=self.ydt, out_split=self.split)
            return
        a = L.ClipAttnArgs()
        a.q, a.k, a.v, a.out = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, out.data_ptr()
        a.row_stride, a.batch_stride = 3 * d, self.T * 3 * d
        a.out_row_stride, a.out_batch_stride = out.stride(0), self.T * out.stride(0)
        a.B, a.H, a.N, a.d_head = F, self.H, self.T, self.dh
        a.scale, a.out_split = self.dh ** -0.5, 1 if self.split else 0
        L.check(L.lib().v2a_clip_attention(ctypes.byref(a), L.stream_ptr()))

    def head(self, bf: dict, F: int) -> torch.Tensor:
        """The residual stream bf["h"] after the last layer -> the output rows bf["out"]."""
        raise NotImplementedError

    @torch.no_grad()
    def encode_chunk(self, frames: torch.Tensor, *, taps: dict | None = None, crop: torch.Tensor | None = None) -> torch.Tensor:
        """One chunk: frames (F, H, W, 3) uint8 on the device -> (F, out_dim) float32 (a view of a reused buffer).
        `taps`: dict whose keys are layer numbers 1..L; each receives a device copy of the residual stream (F, T, d) after that
        layer.  `crop`: optional (F, S, S, 3) uint8 buffer for the preprocessed crop."""
        F = frames.shape[0]
        M, d, dp, dff, T, w = F * self.T, self.d, self.dp, self.dff, self.T, self.w
        epi, nff = self.ffn
        bf = self._buffers(F)
        h, qkv, x, ao, ff = bf["h"], bf["qkv"], bf["x"], bf["ao"], bf["ff"]
        self.preprocess(frames, bf["patches"], crop)
        # class / position rows, then the patch GEMM adds onto them: straight into the residual stream, or through the pre-LayerNorm (fp32)
        emb = h if self.pre_ln is None else bf["emb"]
        L.check(L.lib().v2a_clip_embed_init(emb.data_ptr(), d, M, T, d, self.cls.data_ptr(), self.pos.data_ptr(), L.stream_ptr()))
        self._gemm(bf["patches"], w * self.kp, self.kp, self.patch_w, emb, M=M, N=d, epilogue=L.EPI_RESID, resid=emb)
        if self.pre_ln is not None:
            self.layernorm(emb, h, self.pre_ln, rows=M, y_dtype=L.F32)
        for li, Lw in enumerate(self.layers):
            self.layernorm(h, x, Lw["ln1"], rows=M)
            self._gemm(x, w * dp, dp, Lw["qkv"], qkv, M=M, N=3 * d, bias=Lw["qkv_b"])
            self.attention(qkv, ao, F)
            self._gemm(ao, w * dp, dp, Lw["o"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=h)
            self.layernorm(h, x, Lw["ln2"], rows=M)
            self._gemm(x, w * dp, dp, Lw["fc1"], ff, M=M, N=nff, epilogue=epi, bias=Lw["fc1_b"], out_split=self.split, ldo=w * dff)
            self._gemm(ff, w * dff, dff, Lw["fc2"], h, M=M, N=d, epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=h)
            if taps is not None and li + 1 in taps:
                taps[li + 1] = h.view(F, T, d).clone()
        return self.head(bf, F)

    @torch.no_grad()
    def __call__(self, frames) -> torch.Tensor:
        """frames: uint8 (F, H, W, 3) RGB array or tensor -> (F, out_dim) float32 on the device."""
        fr = torch.as_tensor(np.asarray(frames)) if not torch.is_tensor(frames) else frames
        if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[-1] != 3:
            raise ValueError(f"{type(self).__name__}: frames must be uint8 (F, H, W, 3), got {tuple(fr.shape)} {fr.dtype}")
        F = fr.shape[0]
        out = torch.empty(F, self.out_dim, dtype=torch.float32, device=self.device)
        for i in range(0, F, self.chunk):
            part = fr[i:i + self.chunk].to(self.device).contiguous()
            out[i:i + part.shape[0]] = self.encode_chunk(part)
        return out
