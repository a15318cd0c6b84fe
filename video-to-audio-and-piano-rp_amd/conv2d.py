"""The conv-as-GEMM host layer that the 2-D convolution engines (video2roll.py, roll2midi.py) share.

Both run a convolution as ONE `v2a_gemm`: in the bf16 / bf16x3 modes an implicit GEMM that gathers its patch rows from zero-bordered
NHWC maps through offset tables, in fp32 mode over an explicit `v2a_im2col` patch matrix.  What that needs on the host exists once,
here: the eval-mode BatchNorm fold, the (ky, kx, c) GEMM-row packing of a weight, the offset tables with their in-bounds asserts (a
wrong table is an out-of-bounds DMA), the bordered map with its bf16 or hi | lo shadow, and the per-engine memory that caches them.
Each engine keeps its own network walk and its own `_conv`: the epilogues differ (residuals and pooling there, channel slices and
`v2a_leaky_shadow` here).
"""
from __future__ import annotations

import torch

from . import _lib as L


def check_state_dict(sd: dict, want: dict, who: str) -> None:
    """KeyError / ValueError unless sd has every key of `want` (num_batches_tracked aside) in its shape."""
    missing = [k for k in want if k not in sd and not k.endswith("num_batches_tracked")]
    if missing:
        raise KeyError(f"{who}: state dict lacks {len(missing)} keys, e.g. {missing[:4]}")
    bad = [k for k, shp in want.items() if k in sd and not k.endswith("num_batches_tracked") and tuple(sd[k].shape) != tuple(shp)]
    if bad:
        raise ValueError(f"{who}: shape mismatch for {bad[:4]}")


def fold_batchnorm(w, bias, gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm behind a convolution, folded into it: fp32 weight [co][ci][kh][kw] and bias (None: the convolution has
    none) -> (weight, bias).  Plain fp32 in this order: the packed weights keep their bits."""
    s = gamma / torch.sqrt(var + eps)
    shift = beta - mean * s
    return w * s[:, None, None, None], shift if bias is None else bias * s + shift


def gemm_weight(w: torch.Tensor, segments: tuple[int, ...] | None = None, pad_to: int = 0, k_granule: int = 1) -> torch.Tensor:
    """[co][ci][kh][kw] -> GEMM rows [co][K], K in (ky, kx, c) order (NHWC sources).  segments (fp32 mode): the input channels are the
    concatenation of maps with these widths, each its own patch matrix: K = [(ky, kx, c of map 0) | (ky, kx, c of map 1) ...].
    pad_to: zero rows up to that many outputs; k_granule: zero columns up to a multiple of it."""
    co = w.shape[0]
    parts, c0 = [], 0
    for c in segments or (w.shape[1],):
        parts.append(w[:, c0:c0 + c].permute(0, 2, 3, 1).reshape(co, -1))
        c0 += c
    assert c0 == w.shape[1]
    wk = torch.cat(parts, 1)
    if wk.shape[1] % k_granule:
        wk = torch.cat([wk, torch.zeros(co, -wk.shape[1] % k_granule)], 1)
    if pad_to > co:
        wk = torch.cat([wk, torch.zeros(pad_to - co, wk.shape[1])], 0)
    return wk.contiguous()


def conv_tables(n, H, W, src_border, src_pitch, src_off, ci, kh, kw, stride, pad, Ho, Wo, dst_pitch, dst_border, device="cpu"):
    """Offset tables (elements, int32) of one convolution geometry for v2a_gemm's implicit-GEMM mode: a kh x kw / stride / pad
    convolution reads the ci channels at channel offset src_off of n bordered NHWC maps H x W of src_pitch channels and writes
    Ho x Wo pixels of a map of dst_pitch channels.  The A pointer is map + src_off and the out pointer map + the destination slice's
    offset, so the tables hold pixel offsets only: a_row[m] = the top-left tap of output pixel m, a_k[kt] = the tap and channel of K
    tile kt, o_row[m] = the interior pixel m of a bordered destination (None without a border: the output rows are dense)."""
    assert src_border >= pad, "the source map's zero border must cover the convolution's padding"
    assert ci % 64 == 0 and src_off % 8 == 0 and src_pitch % 8 == 0 and dst_pitch % 8 == 0, "whole 64-element K tiles, 16-byte aligned slices"
    assert src_off + ci <= src_pitch
    Hp, Wp = H + 2 * src_border, W + 2 * src_border
    ni = torch.arange(n, device=device, dtype=torch.int64)[:, None, None]
    yo = torch.arange(Ho, device=device, dtype=torch.int64)[None, :, None]
    xo = torch.arange(Wo, device=device, dtype=torch.int64)[None, None, :]
    a_row = ((ni * Hp + yo * stride - pad + src_border) * Wp + xo * stride - pad + src_border) * src_pitch
    k0 = torch.arange(0, kh * kw * ci, 64, device=device, dtype=torch.int64)
    tap, c0 = k0 // ci, k0 % ci
    a_k = ((tap // kw) * Wp + tap % kw) * src_pitch + c0
    i32 = lambda t: t.reshape(-1).to(torch.int32).contiguous()
    # every 64-element read of the hi plane stays inside the map (the lo plane starts one whole map further)
    assert src_off + int(a_row.max()) + int(a_k.max()) + 64 <= n * Hp * Wp * src_pitch < 2 ** 31
    if not dst_border:
        return i32(a_row), i32(a_k), None
    Hq, Wq = Ho + 2 * dst_border, Wo + 2 * dst_border
    o_row = ((ni * Hq + yo + dst_border) * Wq + xo + dst_border) * dst_pitch
    assert int(o_row.max()) + dst_pitch <= n * Hq * Wq * dst_pitch < 2 ** 31
    return i32(a_row), i32(a_k), i32(o_row)


class Map:
    """C channels at channel offset `off` of an NHWC fp32 activation (n, H + 2b, W + 2b, pitch) with a zero border of b pixels, and
    of its shadow `sh`: the bf16 copy a convolution reads (the DMA GEMM moves raw bf16 bytes), (n, H + 2b, W + 2b, pitch), or in
    bf16x3 mode the split copy (2, n, H + 2b, W + 2b, pitch) -- plane 0 hi, plane 1 lo, both zero-bordered.  plane: the elements of
    one whole map; lo: the distance from the hi to the lo plane (0 unless the shadow is split)."""
    __slots__ = ("f32", "sh", "n", "H", "W", "C", "border", "off", "pitch", "plane", "lo")

    def __init__(self, f32, sh, H, W, border=0, off=0, C=None):
        self.f32, self.sh, self.n, self.H, self.W, self.border, self.off = f32, sh, f32.shape[0], H, W, border, off
        self.pitch, self.plane = f32.shape[-1], f32.numel()
        self.C = self.pitch if C is None else C
        self.lo = self.plane if sh is not None and sh.dim() == 5 else 0
        assert f32.shape == (self.n, H + 2 * border, W + 2 * border, self.pitch) and off + self.C <= self.pitch

    def slice(self, off, C):
        """The channels [off, off + C) of the same memory."""
        return Map(self.f32, self.sh, self.H, self.W, self.border, off, C)

    def base(self):
        """The fp32 map from this slice's first channel on: what a kernel's pointer + pitch address."""
        return self.f32.view(-1)[self.off:] if self.off else self.f32

    def shadow(self):
        return self.sh.view(-1)[self.off:] if self.off and self.sh is not None else self.sh

    def operand(self, K):
        """The shadow as the A operand of an implicit GEMM with K = kh*kw*C (the rows come from the offset tables)."""
        return L.Operand(self.shadow(), K, K, self.lo)

    def interior(self, C=None):
        b = self.border
        v = self.f32 if b == 0 else self.f32[:, b:-b, b:-b]
        return v[..., self.off:self.off + (C or self.C)]

    def nchw(self, C=None):
        return self.interior(C).permute(0, 3, 1, 2)


def split_args(split, shadowed=None):
    """gemm()'s keyword arguments of the bf16x3 mode: the A operand's lo plane lies a whole map behind its hi plane (weight rows are
    [W_hi | W_lo]), and so does the lo plane of the shadow of `shadowed`, the map whose shadow the GEMM writes (None: it writes none)."""
    if not split:
        return {}
    if shadowed is None or shadowed.sh is None:
        return dict(a_split=True)
    return dict(a_split=True, out_bf16_split=True, out_bf16_lo_offset=shadowed.lo)


class ConvMemory:
    """The device memory of one engine's convolutions: activation maps, offset tables and the patch-matrix scratch."""

    def __init__(self, dev, split):
        self.dev, self.split = dev, split
        self._maps, self._tabs, self._cols = {}, {}, {}

    def map(self, name, n, H, W, C, border=0, shadow=False):
        """Cached by full geometry: a bordered map relies on its border staying zero, so two geometries never share memory (nor does
        a split shadow share memory with a plain one)."""
        key = (name, n, H, W, C, border, shadow)
        m = self._maps.get(key)
        if m is None:
            shp = (n, H + 2 * border, W + 2 * border, C)
            f32 = torch.zeros(shp, device=self.dev, dtype=torch.float32)
            sh = torch.zeros(((2,) if self.split else ()) + shp, device=self.dev, dtype=torch.bfloat16) if shadow else None
            m = self._maps[key] = Map(f32, sh, H, W, border)
        return m

    def tables(self, src, dst, kh, kw, stride, pad):
        """`conv_tables` of the convolution that reads the slice `src` and writes the slice `dst`, cached by geometry."""
        key = (src.n, src.H, src.W, src.border, src.pitch, src.off, src.C, kh, kw, stride, pad, dst.H, dst.W, dst.pitch, dst.border)
        t = self._tabs.get(key)
        if t is None:
            t = self._tabs[key] = conv_tables(*key, device=self.dev)
        return t

    def col(self, rows, K, which=0):
        """Grow-only fp32 patch matrix (rows, K); `which` tells the segments of one GEMM apart."""
        need = rows * K
        buf = self._cols.get(which)
        if buf is None or buf.numel() < need:
            buf = self._cols[which] = torch.empty(need, device=self.dev, dtype=torch.float32)
        return buf[:need].view(rows, K)
