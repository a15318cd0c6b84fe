"""Host tables of the image preprocessors (clip.py, dinov2.py through vit.py; piano_frames.py): Pillow's BICUBIC resample and the
transformers image processors' rescale / normalise, restated so that the kernels that read them equal the Pillow path bit for bit.

Pillow resizes in two separable passes of 22-bit fixed-point integer sums, the intermediate clipped to uint8, the filter widened by
the downscale factor.  The integer coefficient tables are built here in double precision with the expressions of Pillow's
`precompute_coeffs` / `normalize_coeffs_8bpc`.
"""
from __future__ import annotations

import math

import numpy as np

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit resample


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


def vertical_window(vb: np.ndarray) -> tuple[int, int, np.ndarray]:
    """Bounds (n, 2) of a vertical pass -> (y0, rows, bounds relative to y0): the pass reads the input rows [y0, y0 + rows), the only
    ones the horizontal pass before it has to produce."""
    y0 = int(vb[:, 0].min())
    rows = int((vb[:, 0] + vb[:, 1]).max()) - y0
    vb = vb.copy()
    vb[:, 0] -= y0
    return y0, rows, vb


def resize_output_size(h: int, w: int, size: int) -> tuple[int, int]:
    """transformers get_resize_output_image_size(default_to_square=False): shortest edge -> size, long edge int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


class ResizePlan:
    """Host tables of one input size: the crop columns of the horizontal pass, the input rows it covers and the crop rows of the
    vertical pass (bounds relative to the first covered row).  `resize`: the shortest-edge target when it differs from the crop S
    (DINOv2's processor resizes to 256 and crops 224; CLIP's resizes to the crop size, the default).  `crop_offset`: "floor", the
    transformers processors' (h - S) // 2, or "torchvision", CenterCrop's int(round((h - S) / 2.0)) with Python's rounding (half to
    even), which differs where h - S is odd: 199 / 2 = 99.5 -> 100, not 99."""

    def __init__(self, H: int, W: int, S: int, resize: int | None = None, crop_offset: str = "floor"):
        if crop_offset not in ("floor", "torchvision"):
            raise ValueError(f"ResizePlan: crop_offset {crop_offset!r} (floor or torchvision)")
        self.H, self.W, self.S = H, W, S
        self.resize = S if resize is None else int(resize)
        if self.resize < S:
            raise ValueError(f"ResizePlan: resize {self.resize} below the crop {S} (the processor would pad)")
        oh, ow = resize_output_size(H, W, self.resize)
        self.out_hw = (oh, ow)
        if crop_offset == "torchvision":
            self.top, self.left = int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))
        else:
            self.top, self.left = (oh - S) // 2, (ow - S) // 2
        hb, hk = resample_coeffs(W, ow)
        vb, vk = resample_coeffs(H, oh)
        self.hb, self.hk = hb[self.left:self.left + S].copy(), hk[self.left:self.left + S].copy()
        self.y0, self.rows, self.vb = vertical_window(vb[self.top:self.top + S])
        self.vk = vk[self.top:self.top + S].copy()
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


def normalize_table(mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD, formula: str = "transformers") -> np.ndarray:
    """(3, 256) float32: the processor's value of byte u in channel c -- rescale in float64 then cast (transformers `rescale`),
    normalise in float32 (`normalize`).  formula="torchvision": ToTensor's float32 division u / 255 followed by Normalize's
    (t - mean) / std in float32 (open_clip's image_transform)."""
    if formula not in ("transformers", "torchvision"):
        raise ValueError(f"normalize_table: formula {formula!r} (transformers or torchvision)")
    u = np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1)
    if formula == "torchvision":
        x = u.astype(np.float32) / np.float32(255)
    else:
        x = (u.astype(np.float64) * (1 / 255)).astype(np.float32)
    y = (x - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32)
    return np.ascontiguousarray(y.T.astype(np.float32))
