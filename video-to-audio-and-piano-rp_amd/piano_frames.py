"""Piano-frame preprocessor on the HIP kernels of csrc/piano_frames.hip: the uncached half of the `piano` branch of the reference's
`E2TTS.encode_video_frames` (x3:1876-1891 with the module-level `transform`, x3:60-63), which turns every decoded RGB video frame
into one grey 100 x 900 float32 image in [0, 1] -- `Image.convert('L')`, `Image.resize((900, 100))` (Pillow's default filter,
BICUBIC), `/ 255.` -- before `encode_frames` reads the stack.

The result equals Pillow's bit for bit.  In Pillow's order: the grey byte `(19595 R + 38470 G + 7471 B + 0x8000) >> 16` of
every pixel; a horizontal pass of 22-bit fixed-point integer sums over those grey bytes, clipped to uint8, for the input rows
the vertical pass reads; the vertical pass, clipped again; and a 256-entry host table of `float32(float64(u) / 255.0)` (the
reference divides a uint8 array by a Python float and casts afterwards).  Rounding the grey value to a byte before filtering is
part of the result: the three channels are never filtered separately.  The coefficient tables are `resample.resample_coeffs`
(Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc`); a pass Pillow skips (equal sizes) has identity tables here, which give
the same bytes.

The 88-key configuration (x3_2 = e2_tts_crossatt3_2.py:65-68) resizes to 100 wide x 900 tall and transposes: layout="portrait",
out[f, i, j] = img[j, i], again (F, 100, 900).  Same arithmetic, other tables (W -> 100, H -> 900); the vertical pass stores
transposed (`v2a_piano_resize_vt`).  The cache file has the same name and shapes under both layouts (features.load_piano_frames).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .resample import PRECISION_BITS, resample_coeffs, vertical_window

PIANO_HW = (100, 900)          # x3:60: `x.resize((900, 100))`; x3_2:65-67: `x.resize((100, 900))`, transposed
LAYOUTS = ("landscape", "portrait")
_HALF = 1 << (PRECISION_BITS - 1)


def grey_numpy(frames: np.ndarray) -> np.ndarray:
    """Pillow's rgb2l on (..., 3) uint8: the ITU-R 601-2 luma in 16-bit fixed point, rounded to a byte."""
    x = frames.astype(np.int64)
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16


def scale_table() -> np.ndarray:
    """(256,) float32: byte u -> u / 255. as the reference rounds it (float64 division, then the cast to float32, x3:1890)."""
    return (np.arange(256, dtype=np.uint8) / 255.).astype(np.float32)


class PianoFramePlan:
    """Host tables of one input size: horizontal bounds / coefficients of all Wo columns, the input rows [y0, y0 + rows) the
    vertical pass reads, and its bounds relative to y0.  Ho, Wo: the shape of an output frame.  layout="portrait": the image is
    resized to Ho wide x Wo tall and stored transposed, so the tables are those of W -> Ho and H -> Wo."""

    def __init__(self, H: int, W: int, Ho: int = PIANO_HW[0], Wo: int = PIANO_HW[1], layout: str = "landscape"):
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'landscape' or 'portrait', got {layout!r}")
        self.layout, self.out_hw = layout, (int(Ho), int(Wo))
        if layout == "portrait":
            Ho, Wo = Wo, Ho                                  # from here on: the resized image's rows and columns
        self.H, self.W, self.Ho, self.Wo = int(H), int(W), int(Ho), int(Wo)
        self.hb, self.hk = resample_coeffs(self.W, self.Wo)
        vb, self.vk = resample_coeffs(self.H, self.Ho)
        self.y0, self.rows, self.vb = vertical_window(vb)
        self.lut = scale_table()
        # the kernels read what the tables say: every tap must lie inside the image (checked here, the device cannot)
        assert (self.hb[:, 0] >= 0).all() and (self.hb[:, 1] > 0).all() and (self.hb[:, 0] + self.hb[:, 1] <= self.W).all()
        assert (self.hb[:, 1] <= self.hk.shape[1]).all() and (self.vb[:, 1] <= self.vk.shape[1]).all()
        assert (self.vb[:, 0] >= 0).all() and (self.vb[:, 1] > 0).all() and (self.vb[:, 0] + self.vb[:, 1] <= self.rows).all()
        assert self.y0 >= 0 and self.y0 + self.rows <= self.H

    def integer_passes(self, frames: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """(F, H, W, 3) uint8 -> the sums of both passes after the shift and before the clip, int64 (F, rows, Wo) and
        (F, Ho, Wo) of the resized image (untransposed): what `preprocess_numpy` clips, and what tells whether a test image
        overshoots [0, 255] at all."""
        fr = np.asarray(frames)
        if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[1:] != (self.H, self.W, 3):
            raise ValueError(f"PianoFramePlan({self.H}, {self.W}): frames must be uint8 (F, {self.H}, {self.W}, 3), got {fr.shape} {fr.dtype}")
        g = grey_numpy(fr[:, self.y0:self.y0 + self.rows])
        hs = np.empty((fr.shape[0], self.rows, self.Wo), np.int64)
        for j in range(self.Wo):
            x0, n = self.hb[j]
            hs[:, :, j] = ((g[:, :, x0:x0 + n] * self.hk[j, :n]).sum(2) + _HALF) >> PRECISION_BITS
        tmp = np.clip(hs, 0, 255)
        vs = np.empty((fr.shape[0], self.Ho, self.Wo), np.int64)
        for i in range(self.Ho):
            r0, n = self.vb[i]
            vs[:, i] = ((tmp[:, r0:r0 + n] * self.vk[i, :n, None]).sum(1) + _HALF) >> PRECISION_BITS
        return hs, vs

    def preprocess_numpy(self, frames: np.ndarray) -> np.ndarray:
        """(F, H, W, 3) uint8 RGB -> (F, Ho, Wo) float32, the reference's `frames_raw[:, :, :, 0]`: the pure-integer restatement
        the kernels follow.  Portrait: the resized (Wo tall, Ho wide) image transposed (x3_2:66-67)."""
        out = self.lut[np.clip(self.integer_passes(frames)[1], 0, 255)]
        return np.ascontiguousarray(out.transpose(0, 2, 1)) if self.layout == "portrait" else out


def lib_vpass(layout: str):
    """The vertical pass of a layout: `v2a_piano_resize_v` stores (n, Ho, Wo), `v2a_piano_resize_vt` the transposed (n, Wo, Ho)."""
    return L.lib().v2a_piano_resize_vt if layout == "portrait" else L.lib().v2a_piano_resize_v


class PianoFramePreprocessor:
    """`__call__(frames, select=None)`: uint8 (F, H, W, 3) RGB frames (tensor or array) -> (n, Ho, Wo) float32 on the device, for
    the frame numbers `select` (any order, repeats allowed) or all F.  Frames are processed `chunk` at a time so that the uint8
    intermediate of the two passes stays bounded; no arithmetic crosses frames, so the chunk size changes no byte.
    layout: "landscape" (x3) or "portrait" (x3_2, the 88-key configuration); (Ho, Wo) is the output frame's shape in both."""

    def __init__(self, device, Ho: int = PIANO_HW[0], Wo: int = PIANO_HW[1], chunk: int = 64, layout: str = "landscape"):
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'landscape' or 'portrait', got {layout!r}")
        self.layout = layout
        self.device = torch.device(device)
        self.Ho, self.Wo, self.chunk = int(Ho), int(Wo), int(chunk)
        self.frames_done = 0          # frames resized so far (callers and tests count the work)
        self._plans: dict[tuple, tuple] = {}
        self._lut = None
        L.lib()

    def _plan(self, H: int, W: int):
        pl = self._plans.get((H, W))
        if pl is None:
            p = PianoFramePlan(H, W, self.Ho, self.Wo, self.layout)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            if self._lut is None:
                self._lut = t(p.lut)
            pl = (p, t(p.hb), t(p.hk), t(p.vb), t(p.vk))
            self._plans[(H, W)] = pl
        return pl

    @torch.no_grad()
    def __call__(self, frames, select=None, *, chunk: int | None = None) -> torch.Tensor:
        fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[-1] != 3:
            raise ValueError(f"PianoFramePreprocessor: frames must be uint8 (F, H, W, 3), got {tuple(fr.shape)} {fr.dtype}")
        F, H, W, _ = fr.shape
        sel = None
        if select is not None:
            sel = torch.as_tensor(select, dtype=torch.int64).reshape(-1).cpu()
            if sel.numel() and (int(sel.min()) < 0 or int(sel.max()) >= F):
                raise IndexError(f"PianoFramePreprocessor: select outside [0, {F})")
        n = F if sel is None else sel.numel()
        out = torch.empty(n, self.Ho, self.Wo, dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        p, hb, hk, vb, vk = self._plan(H, W)
        if fr.device != self.device and sel is not None:
            # upload only the frames that are used, each once
            uniq, inv = torch.unique(sel, return_inverse=True)
            fr, sel, F = fr[uniq], inv, uniq.numel()
        fr = fr.to(self.device).contiguous()
        step = max(1, int(chunk or self.chunk))
        # p.Ho, p.Wo are the rows and columns of the resized image: the output's (Ho, Wo), or for portrait the output's (Wo, Ho)
        ldt = -(-p.Wo // 4) * 4
        vpass = lib_vpass(self.layout)
        tmp = torch.empty(min(step, n), p.rows, ldt, dtype=torch.uint8, device=self.device)
        whole = sel is None and step >= n
        seld = None if whole else (torch.arange(F, dtype=torch.int32) if sel is None else sel.to(torch.int32)).to(self.device)
        lib, s = L.lib(), L.stream_ptr()
        for i in range(0, n, step):
            m = min(step, n - i)
            sp = 0 if whole else seld.data_ptr() + 4 * i
            L.check(lib.v2a_piano_resize_h(fr.data_ptr(), F, H, W, sp, m, tmp.data_ptr(), ldt, p.y0, p.rows, p.Wo, hb.data_ptr(),
                                           hk.data_ptr(), hk.shape[1], s))
            L.check(vpass(tmp.data_ptr(), m, p.rows, ldt, p.Ho, p.Wo, vb.data_ptr(), vk.data_ptr(), vk.shape[1],
                          self._lut.data_ptr(), out[i:i + m].data_ptr(), s))
        self.frames_done += n
        return out
