"""Write tests/golden/clip_convnext_{small,wide,full}.npz: transformers' float64 `ConvNextModel` -- block for block the network of
timm's ConvNeXt; its LayerNorm eps is fixed at 1e-6 in the stem, the downsample layers and the blocks, so the fixtures are made at
1e-6 throughout -- on the seeded weights of v2a_amd.synth.random_convnext_state_dict (timm keys mapped onto its names), then the
projection in float64; the pixel values come from Pillow (`Image.resize`, `crop`) and torch fp32 operations, with torchvision's size
and crop arithmetic restated (tests/convnext_ref.py: torchvision is not installed).  CPU only.

Each file: meta (json: versions, and per case config, eps, resize, crop, seeds, clips, taps, fp32_err = the error of torch's CPU fp32
run of the same model against float64, per clip), and per case c and clip:
  c_frames_md5 (F,) -- md5 of each generated frame (the test regenerates them and checks these first)
  c_crop_md5 (F,) -- md5 of the uint8 image after resize + centre crop (bit-exact target of the GPU preprocessing)
  c_crop_idx (n,) int64 / c_crop_vals (F, n) uint8 -- that image at sampled flat (S, S, 3) positions
  c_pix_idx (n,) int64 / c_pix (F, n) float32 -- the pixel values at sampled flat (3, S, S) positions
  c_embeds (F, embed_dim) float64 -- the projected embedding
  c_tap_{t}_rows (r,) int64 / c_tap_{t} (F, r, C) float32 -- sampled pixels (flat h * w) of the map behind the stem (t = stem), behind
  each stage (t = s0 .. s3) and behind the first and last block of stage 2 (t = s2b0, s2bL)
Usage: python scripts/make_golden_clip_convnext.py [small|wide|full ...]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import convnext_ref as R  # noqa: E402
from v2a_amd.synth import CONVNEXT_XXLARGE, random_convnext_state_dict, synthetic_video_frames  # noqa: E402

SMALL = dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=128)
WIDE = dict(CONVNEXT_XXLARGE, depths=(1, 1, 1, 1))
OUTLIER = 30.0
# 100 x 180 at 64 resizes to 115 wide: (115 - 64) / 2 = 25.5 -> torchvision's left is 26, the floor 25 (likewise its portrait twin's top)
CLIPS64 = [("land", 2, 360, 640, 1), ("port", 2, 640, 360, 2), ("half", 1, 100, 180, 3), ("halfp", 1, 180, 100, 4), ("up", 1, 40, 50, 5)]
# name -> (config, resize = crop, weight seed, outlier, [(clip, frames, h, w, frame seed)], tap pixels per map)
CASES = {
    "small": (SMALL, 64, 31, 0.0, CLIPS64, 6),
    # the real preprocessing size: 360 x 640 resizes to 455 wide, (455 - 256) / 2 = 99.5 -> left 100, not 99
    "small_256": (dict(SMALL, depths=(1, 1, 1, 1)), 256, 32, 0.0, [("land", 1, 360, 640, 6), ("port", 1, 640, 360, 7)], 6),
    "wide": (WIDE, 64, 33, 0.0, [("land", 1, 360, 640, 1), ("half", 1, 100, 180, 2)], 3),
    "wide_outlier": (WIDE, 64, 34, OUTLIER, [("land", 2, 360, 640, 5)], 3),
    "full": (dict(SMALL, depths=CONVNEXT_XXLARGE["depths"]), 64, 35, 0.0, [("land", 2, 360, 640, 6), ("halfp", 1, 180, 100, 8)], 6),
}
FILES = {"small": ["small", "small_256"], "wide": ["wide", "wide_outlier"], "full": ["full"]}
EPS = 1e-6


def frames_md5(fr: np.ndarray) -> np.ndarray:
    return np.array([hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr])


def hf_state_dict(sd: dict) -> dict:
    """timm keys (bare `trunk.*`) -> ConvNextModel's."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("trunk."):
            continue
        k = k[len("trunk."):]
        k = k.replace("stem.0.", "embeddings.patch_embeddings.").replace("stem.1.", "embeddings.layernorm.")
        k = k.replace("head.norm.", "layernorm.")
        if k.startswith("stages."):
            k = "encoder." + k.replace(".downsample.", ".downsampling_layer.").replace(".blocks.", ".layers.")
            k = k.replace(".conv_dw.", ".dwconv.").replace(".norm.", ".layernorm.").replace(".mlp.fc1.", ".pwconv1.").replace(".mlp.fc2.", ".pwconv2.")
            if k.endswith(".gamma"):
                k = k[:-len("gamma")] + "layer_scale_parameter"
        out[k] = v
    return out


def build_model(config: dict, sd: dict, image: int):
    from transformers import ConvNextConfig, ConvNextModel
    cfg = ConvNextConfig(num_channels=3, patch_size=4, num_stages=len(config["dims"]), hidden_sizes=list(config["dims"]), depths=list(config["depths"]),
                         hidden_act="gelu", layer_norm_eps=EPS, layer_scale_init_value=1.0, image_size=image)
    with torch.device("meta"):
        m = ConvNextModel(cfg)
    res = m.load_state_dict(hf_state_dict(sd), strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.eval()


def run_model(model, pv, proj):
    """pixel values -> (embedding, {tap name: NHWC map}) in the model's dtype."""
    got = {}
    st2 = model.encoder.stages[2].layers
    hooks = [st2[0].register_forward_hook(lambda m, i, o: got.__setitem__("s2b0", o)),
             st2[len(st2) - 1].register_forward_hook(lambda m, i, o: got.__setitem__("s2bL", o))]
    with torch.no_grad():
        o = model(pixel_values=pv, output_hidden_states=True)
    for h in hooks:
        h.remove()
    got["stem"] = o.hidden_states[0]
    for s in range(len(model.encoder.stages)):
        got[f"s{s}"] = o.hidden_states[s + 1]
    return o.pooler_output @ proj.t(), {k: v.permute(0, 2, 3, 1) for k, v in got.items()}


def run_case(name: str, out: dict, meta: dict):
    config, S, seed, outlier, clips, tap_rows = CASES[name]
    sd32 = R.bare_keys(random_convnext_state_dict(config, seed, outlier), torch.float32)
    m64 = build_model(config, {k: v.double() for k, v in sd32.items()}, S)
    m32 = build_model(config, sd32, S)
    proj = sd32["head.proj.weight"]
    rng = np.random.default_rng(seed + 1000)
    taps = ["stem"] + [f"s{s}" for s in range(len(config["dims"]))] + ["s2b0", "s2bL"]
    fp32_err = {}
    for (clip, n, h, w, fseed) in clips:
        key = f"{name}_{clip}"
        fr = synthetic_video_frames(n, h, w, fseed)
        crop, pv = R.preprocess(fr, S, S)
        assert pv.shape[1:] == (3, S, S) and pv.dtype == torch.float32
        emb, maps = run_model(m64, pv.double(), proj.double())
        emb32, _ = run_model(m32, pv, proj)
        fp32_err[clip] = float((emb32.double() - emb).abs().max() / emb.abs().max())
        out[key + "_frames_md5"] = frames_md5(fr)
        out[key + "_crop_md5"] = frames_md5(crop)
        cidx = np.sort(rng.choice(crop[0].size, size=min(4096, crop[0].size), replace=False))
        out[key + "_crop_idx"], out[key + "_crop_vals"] = cidx, crop.reshape(n, -1)[:, cidx]
        idx = np.sort(rng.choice(pv[0].numel(), size=min(2048, pv[0].numel()), replace=False))
        out[key + "_pix_idx"], out[key + "_pix"] = idx, pv.reshape(n, -1)[:, idx].numpy()
        out[key + "_embeds"] = emb.numpy()
        for t in taps:
            mp = maps[t]
            px = mp.shape[1] * mp.shape[2]
            rows = np.sort(rng.choice(px, size=min(tap_rows, px), replace=False))
            out[key + f"_tap_{t}_rows"] = rows
            out[key + f"_tap_{t}"] = mp.reshape(n, px, -1)[:, rows].numpy().astype(np.float32)
        print(f"{key}: {n} x {h}x{w}, |embeds| max {emb.abs().max().item():.3f}, |last map| max {maps[taps[-3]].abs().max().item():.1f}, "
              f"CPU fp32 vs float64 {fp32_err[clip]:.2e}", flush=True)
    meta["cases"][name] = dict(config=dict(config, depths=list(config["depths"]), dims=list(config["dims"])), eps=EPS, resize=S, crop=S, seed=seed,
                               outlier=outlier, clips=[list(c) for c in clips], taps=taps, fp32_err=fp32_err)


def main(which):
    import PIL
    import transformers
    for f in which:
        out, meta = {}, dict(transformers=transformers.__version__, pillow=PIL.__version__, torch=torch.__version__, numpy=np.__version__,
                             cases={})
        for name in FILES[f]:
            run_case(name, out, meta)
        worst = max(e for c in meta["cases"].values() for e in c["fp32_err"].values())
        assert worst <= 0.25 * 2e-5, f"CPU fp32 error {worst:.2e} above a quarter of the fp32 bar 2e-5: pick another seed or regime"
        out["meta"] = np.array(json.dumps(meta))
        path = os.path.join(ROOT, "tests", "golden", f"clip_convnext_{f}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main(sys.argv[1:] or ["small", "wide", "full"])
