"""Write tests/golden/dinov2_{small,wide,full}.npz: transformers' own BitImageProcessor (shortest edge -> resize, centre crop,
ImageNet mean / std, BICUBIC) + Dinov2Model (attn_implementation="eager", float64, CPU) on the seeded weights of
v2a_amd.synth.random_dinov2_state_dict and the seeded frames of synth.synthetic_video_frames.  CPU only; the full case holds ~9 GB
of float64 weights and takes minutes.

Each file: meta (json: versions, and per case config, resize, crop, seeds, clips, taps), and per case c and clip:
  c_frames_md5 (F,) -- md5 of each generated frame (the test regenerates them and checks these first)
  c_crop_md5 (F,) -- md5 of the processor's uint8 image after resize + centre crop (bit-exact target of the GPU preprocessing),
  c_crop_idx (n,) int64 / c_crop_vals (F, n) uint8 -- that image at sampled flat (S, S, 3) positions
  c_pix_idx (n,) int64 / c_pix (F, n) float32 -- pixel_values at sampled flat (C, S, S) positions
  c_embeds (F, hidden_size) float64 -- pooler_output
  c_tap{l}_rows (r,) int64 / c_tap{l} (F, r, d) float32 -- sampled token rows of the residual stream after layer l (1, L/2, L)
Usage: python scripts/make_golden_dinov2.py [small|wide|full ...]
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from v2a_amd.dinov2 import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from v2a_amd.synth import DINOV2_GIANT, random_dinov2_state_dict, synthetic_video_frames  # noqa: E402

# the stored position grid is 5 x 5 (image_size 70) and the run crops 56 (4 x 4): the interpolation is exercised
SMALL = dict(hidden_size=192, num_hidden_layers=3, num_attention_heads=3, mlp_ratio=4, image_size=70, patch_size=14, layer_norm_eps=1e-6,
             use_swiglu_ffn=True, num_channels=3, layerscale_value=1.0)
OUTLIER = 30.0
SMALL_CLIPS = [("land", 2, 360, 640, 1), ("port", 2, 640, 360, 2), ("up", 1, 40, 50, 3), ("odd", 1, 97, 131, 4)]
# name -> (config, resize, crop, weight seed, outlier, [(case, frames, h, w, frame seed)], tap rows per frame)
CASES = {
    "small": (SMALL, 64, 56, 21, 0.0, SMALL_CLIPS, 5),
    "small_gelu": (dict(SMALL, use_swiglu_ffn=False), 64, 56, 25, 0.0, [("land", 2, 360, 640, 7)], 5),
    "wide": (dict(DINOV2_GIANT, num_hidden_layers=4), 256, 224, 22, 0.0,
             [("land", 1, 360, 640, 1), ("port", 1, 640, 360, 2), ("up", 1, 150, 200, 3), ("odd", 1, 227, 301, 4)], 3),
    "wide_outlier": (dict(DINOV2_GIANT, num_hidden_layers=4), 256, 224, 23, OUTLIER, [("land", 2, 360, 640, 5)], 3),
    "full": (DINOV2_GIANT, 256, 224, 24, 0.0, [("land", 2, 360, 640, 6)], 3),
}
FILES = {"small": ["small", "small_gelu"], "wide": ["wide", "wide_outlier"], "full": ["full"]}


def frames_md5(fr: np.ndarray) -> np.ndarray:
    return np.array([hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr])


def build_model(config: dict, sd: dict):
    from transformers import Dinov2Config, Dinov2Model
    cfg = Dinov2Config(**config, attn_implementation="eager")
    with torch.device("meta"):
        m = Dinov2Model(cfg)
    missing = m.load_state_dict(sd, strict=True, assign=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.double().eval()


def run_case(name: str, out: dict, meta: dict):
    from PIL import Image
    from transformers import BitImageProcessor
    config, resize, S, seed, outlier, clips, tap_rows = CASES[name]
    L = config["num_hidden_layers"]
    sd = random_dinov2_state_dict(config, seed, outlier)
    model = build_model(config, sd)
    del sd
    proc = BitImageProcessor(size={"shortest_edge": resize}, crop_size={"height": S, "width": S}, resample=Image.BICUBIC,
                             image_mean=list(IMAGENET_MEAN), image_std=list(IMAGENET_STD))
    T = 1 + (S // config["patch_size"]) ** 2
    rng = np.random.default_rng(seed + 1000)
    taps = sorted({1, max(1, L // 2), L})
    meta["cases"][name] = dict(config=config, resize=resize, crop=S, seed=seed, outlier=outlier, clips=[list(c) for c in clips], taps=taps)
    for (case, n, h, w, fseed) in clips:
        key = f"{name}_{case}"
        fr = synthetic_video_frames(n, h, w, fseed)
        pix = proc(images=list(fr), return_tensors="np", do_normalize=False, do_rescale=False)["pixel_values"]
        crop = np.rint(pix).astype(np.uint8).transpose(0, 2, 3, 1)          # the uint8 image after resize + crop
        pv = proc(images=list(fr), return_tensors="np")["pixel_values"].astype(np.float32)
        assert pv.shape[1:] == (3, S, S), pv.shape
        idx = np.sort(rng.choice(pv[0].size, size=min(2048, pv[0].size), replace=False))
        with torch.no_grad():
            o = model(pixel_values=torch.from_numpy(pv).double(), output_hidden_states=True)
        assert o.hidden_states[L].shape[1] == T
        rows = np.unique(np.concatenate([[0, T - 1], rng.choice(T, size=tap_rows, replace=False)]))[:max(tap_rows, 2)]
        out[key + "_frames_md5"] = frames_md5(fr)
        out[key + "_crop_md5"] = frames_md5(crop)                          # the whole crop, bit for bit
        cidx = np.sort(rng.choice(crop[0].size, size=min(4096, crop[0].size), replace=False))
        out[key + "_crop_idx"] = cidx
        out[key + "_crop_vals"] = crop.reshape(n, -1)[:, cidx]               # where a mismatch lies
        out[key + "_pix_idx"] = idx
        out[key + "_pix"] = pv.reshape(n, -1)[:, idx]
        out[key + "_embeds"] = o.pooler_output.numpy()
        for l in taps:
            out[key + f"_tap{l}_rows"] = rows
            out[key + f"_tap{l}"] = o.hidden_states[l][:, rows].numpy().astype(np.float32)
        print(f"{key}: {n} x {h}x{w}, |pooler_output| max {np.abs(o.pooler_output.numpy()).max():.3f}, |h_L| max "
              f"{o.hidden_states[L].abs().max().item():.1f}", flush=True)
    del model


def main(which):
    import PIL
    import transformers
    for f in which:
        out, meta = {}, dict(transformers=transformers.__version__, pillow=PIL.__version__, torch=torch.__version__, numpy=np.__version__,
                             cases={})
        for name in FILES[f]:
            run_case(name, out, meta)
        out["meta"] = np.array(json.dumps(meta))
        path = os.path.join(ROOT, "tests", "golden", f"dinov2_{f}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main(sys.argv[1:] or ["small", "wide", "full"])
