"""Write tests/golden/clip_vit2_{small,wide,full}.npz: transformers' own CLIPImageProcessor(size={"shortest_edge": S}, crop_size=S) +
CLIPVisionModelWithProjection (attn_implementation="eager", hidden_act="quick_gelu", float64, CPU) on the seeded weights of
v2a_amd.synth.random_clip_vision_state_dict and the seeded frames of synth.synthetic_video_frames -- the `video_encoder="clip_vit2"`
model, openai/clip-vit-large-patch14-336 (synth.VIT_L_14_336), whose own weights are not reachable offline.  CPU only; the full case
holds ~2.5 GB of float64 weights.

The keys are those of scripts/make_golden_clip.py (whose model builder and md5 helper are used here); per case c:
  c_frames_md5, c_crop_md5, c_crop_idx / c_crop_vals, c_pix_idx / c_pix, c_embeds (float64), c_tap{l}_rows / c_tap{l} for l in 1, L/2, L
and `meta` (json: versions, config, cases).
Usage: python scripts/make_golden_clip_vit2.py [small|wide|full ...]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from make_golden_clip import build_model, frames_md5  # noqa: E402
from v2a_amd.synth import VIT_L_14_336, random_clip_vision_state_dict, synthetic_video_frames  # noqa: E402

# 64-wide heads: the MFMA attention; 104-wide heads: the VALU attention beside the new epilogue
SMALL = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, image_size=56, patch_size=14,
             projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3)
SMALL104 = dict(hidden_size=208, intermediate_size=832, num_hidden_layers=3, num_attention_heads=2, image_size=56, patch_size=14,
                projection_dim=128, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3)
WIDE = dict(VIT_L_14_336, num_hidden_layers=4)
OUTLIER = 30.0
# name -> (config, weight seed, outlier, [(case, frames, h, w, frame seed)], taps rows per frame)
CASES = {
    "small": (SMALL, 21, 0.0, [("land", 2, 360, 640, 1), ("port", 2, 640, 360, 2), ("up", 1, 40, 50, 3), ("odd", 1, 97, 131, 4)], 5),
    "small104": (SMALL104, 25, 0.0, [("land", 2, 360, 640, 1)], 5),
    "wide": (WIDE, 22, 0.0, [("land", 1, 360, 640, 1), ("port", 1, 640, 360, 2), ("up", 1, 150, 200, 3), ("odd", 1, 227, 301, 4)], 3),
    "wide_outlier": (WIDE, 23, OUTLIER, [("land", 2, 360, 640, 5)], 3),
    "full": (VIT_L_14_336, 24, 0.0, [("land", 2, 360, 640, 6)], 3),
}
FILES = {"small": ["small", "small104"], "wide": ["wide", "wide_outlier"], "full": ["full"]}


def run_case(name: str, out: dict, meta: dict):
    from transformers import CLIPImageProcessor
    config, seed, outlier, clips, tap_rows = CASES[name]
    S, L = config["image_size"], config["num_hidden_layers"]
    sd = random_clip_vision_state_dict(config, seed, outlier)
    model = build_model(config, sd)
    assert type(model.vision_model.encoder.layers[0].mlp.activation_fn).__name__ == "QuickGELUActivation"
    del sd
    proc = CLIPImageProcessor(size={"shortest_edge": S}, crop_size=S)
    T = 1 + (S // config["patch_size"]) ** 2
    rng = np.random.default_rng(seed + 1000)
    taps = sorted({1, max(1, L // 2), L})
    meta["cases"][name] = dict(config=config, seed=seed, outlier=outlier, clips=[list(c) for c in clips], taps=taps)
    for (case, n, h, w, fseed) in clips:
        key = f"{name}_{case}"
        fr = synthetic_video_frames(n, h, w, fseed)
        pix = proc(images=list(fr), return_tensors="np", do_normalize=False, do_rescale=False)["pixel_values"]
        assert pix.shape == (n, 3, S, S), pix.shape
        crop = np.rint(pix).astype(np.uint8).transpose(0, 2, 3, 1)          # the uint8 image after resize + crop
        pv = proc(images=list(fr), return_tensors="np")["pixel_values"].astype(np.float32)
        idx = np.sort(rng.choice(pv[0].size, size=min(2048, pv[0].size), replace=False))
        with torch.no_grad():
            o = model(pixel_values=torch.from_numpy(pv).double(), output_hidden_states=True)
        rows = np.unique(np.concatenate([[0, T - 1], rng.choice(T, size=tap_rows, replace=False)]))[:max(tap_rows, 2)]
        out[key + "_frames_md5"] = frames_md5(fr)
        out[key + "_crop_md5"] = frames_md5(crop)                          # the whole crop, bit for bit
        cidx = np.sort(rng.choice(crop[0].size, size=min(4096, crop[0].size), replace=False))
        out[key + "_crop_idx"] = cidx
        out[key + "_crop_vals"] = crop.reshape(n, -1)[:, cidx]               # where a mismatch lies
        out[key + "_pix_idx"] = idx
        out[key + "_pix"] = pv.reshape(n, -1)[:, idx]
        out[key + "_embeds"] = o.image_embeds.numpy()
        for l in taps:
            out[key + f"_tap{l}_rows"] = rows
            out[key + f"_tap{l}"] = o.hidden_states[l][:, rows].numpy().astype(np.float32)
        print(f"{key}: {n} x {h}x{w}, |embeds| max {np.abs(o.image_embeds.numpy()).max():.3f}, |h_L| max "
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
        path = os.path.join(ROOT, "tests", "golden", f"clip_vit2_{f}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main(sys.argv[1:] or ["small", "wide", "full"])
