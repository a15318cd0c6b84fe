"""A plain-torch restatement of the reference's "clip_convnext" image path, for the tests and the probe: open_clip's eval
`image_transform` (Resize(n, BICUBIC) on the PIL image, CenterCrop(n), ToTensor, Normalize) and `TimmModel.forward` =
`head(trunk(x))` around timm's ConvNeXt, under the timm / open_clip key names (`trunk.*`, `head.proj.*`), with the LayerNorm eps as a
parameter.  Neither timm, open_clip nor torchvision is installed: the size and crop arithmetic is restated from torchvision's
published `Resize` / `CenterCrop` (the resize itself and the crop are Pillow's own calls), and the network from timm's `ConvNeXt` /
`ConvNeXtBlock` (conv_mlp=False) and open_clip's `TimmModel` (pool 'avg' kept inside the trunk, linear projection without bias
unless the state dict has one).  tests/test_clip_convnext_refs.py pins it at eps 1e-6 against transformers' `ConvNextModel`.

The tensors decide dtype and device: float64 on the CPU for the tests, float32 on the GPU for the probe."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_PREFIXES = ("image_encoder.visual.", "image_encoder.", "visual.")


def bare_keys(sd: dict, dtype=torch.float64, device="cpu") -> dict:
    """open_clip / reference-checkpoint keys -> `trunk.*` / `head.*` in `dtype` on `device`."""
    out = {}
    for k, v in sd.items():
        for p in _PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        out[k] = v.to(device=device, dtype=dtype)
    return out


def resized_size(h: int, w: int, size: int) -> tuple[int, int]:
    """torchvision Resize(size: int): the shortest edge becomes `size`, the long one int(size * long / short) -> (height, width)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def crop_offsets(h: int, w: int, size: int) -> tuple[int, int]:
    """torchvision CenterCrop: top = int(round((h - size) / 2.0)), left likewise -- Python's round, half to even."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def preprocess(frames: np.ndarray, resize: int = 256, crop: int = 256, mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD):
    """frames (F, H, W, 3) uint8 -> (the uint8 crops (F, S, S, 3), the fp32 pixel values (F, 3, S, S)): Pillow's resize and crop on each
    frame, then ToTensor's u / 255 and Normalize's (t - mean) / std as torch float32 operations."""
    from PIL import Image
    crops = []
    for fr in frames:
        img = Image.fromarray(fr)
        oh, ow = resized_size(img.height, img.width, resize)
        img = img.resize((ow, oh), Image.BICUBIC)
        top, left = crop_offsets(oh, ow, crop)
        crops.append(np.asarray(img.crop((left, top, left + crop, top + crop))))
    crops = np.stack(crops)
    t = torch.from_numpy(crops).permute(0, 3, 1, 2).to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1), torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return crops, t.sub(m).div(s)


def _ln(x, sd, k, eps):
    """LayerNorm over the channels of an NCHW map, per pixel."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), sd[k + ".weight"], sd[k + ".bias"], eps).permute(0, 3, 1, 2)


def forward(sd: dict, x: torch.Tensor, eps: float = 1e-5, taps: dict | None = None) -> torch.Tensor:
    """sd: bare keys (bare_keys); x (F, 3, S, S) pixel values in sd's dtype -> (F, embed_dim).  taps: keys "stem" or (stage, block),
    both from 0; each receives the NHWC map (F, h, w, C) behind the stem's LayerNorm or behind that block."""
    h = _ln(F.conv2d(x, sd["trunk.stem.0.weight"], sd["trunk.stem.0.bias"], stride=4), sd, "trunk.stem.1", eps)
    if taps is not None and "stem" in taps:
        taps["stem"] = h.permute(0, 2, 3, 1).clone()
    s = 0
    while f"trunk.stages.{s}.blocks.0.gamma" in sd:
        p = f"trunk.stages.{s}."
        if s:
            h = F.conv2d(_ln(h, sd, p + "downsample.0", eps), sd[p + "downsample.1.weight"], sd[p + "downsample.1.bias"], stride=2)
        j = 0
        while p + f"blocks.{j}.gamma" in sd:
            b = p + f"blocks.{j}."
            C = h.shape[1]
            y = F.conv2d(h, sd[b + "conv_dw.weight"], sd[b + "conv_dw.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (C,), sd[b + "norm.weight"], sd[b + "norm.bias"], eps)
            y = F.linear(F.gelu(F.linear(y, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"])), sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
            h = h + (y * sd[b + "gamma"]).permute(0, 3, 1, 2)
            if taps is not None and (s, j) in taps:
                taps[(s, j)] = h.permute(0, 2, 3, 1).clone()
            j += 1
        s += 1
    pooled = F.layer_norm(h.mean((-2, -1)), (h.shape[1],), sd["trunk.head.norm.weight"], sd["trunk.head.norm.bias"], eps)
    return F.linear(pooled, sd["head.proj.weight"], sd.get("head.proj.bias"))
