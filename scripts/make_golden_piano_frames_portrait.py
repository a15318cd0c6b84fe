"""Write tests/golden/piano_frames_portrait.npz: Pillow's own result for the piano-frame preprocessing of the reference's 88-key
configuration (x3_2 = e2_tts_crossatt3_2.py:65-68, 1901-1906) on seeded frames -- per frame `Image.fromarray(rgb).convert('L')`,
`.resize((100, 900))` (100 wide, 900 tall; the default filter, BICUBIC), the reshape to (900, 100, 1), the transpose [2, 1, 0] to
(1, 100, 900) and `/ 255.` (float64), concatenated and cast to float32.  CPU only.

The layout of tests/golden/piano_frames.npz (scripts/make_golden_piano_frames.py): hashes and samples, not images -- meta (json:
pillow / numpy versions, cases), and per case c
  c_frames_md5 (F,) -- md5 of each generated input frame (the tests regenerate them and check these first)
  c_out_md5 (F,)    -- md5 of each output frame's float32 bytes (the bit-exact target)
  c_idx (n,) int64 / c_vals (F, n) float32 -- the output at sampled flat (100, 900) positions, so that a mismatch is readable
Frames: v2a_amd.synth.synthetic_video_frames (smooth) followed by synth.synthetic_edge_frames (hard 0 / 255 edges).  For the case
of edge frames the script asserts, with the integers of PianoFramePlan.integer_passes, that the unclipped sums of both passes leave
[0, 255] on both sides: otherwise the clip of either pass would never be exercised.

Usage: python scripts/make_golden_piano_frames_portrait.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from v2a_amd.piano_frames import PianoFramePlan  # noqa: E402
from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames  # noqa: E402

# (case, H, W, smooth frames, edge frames, seed, overshoot asserted)
CASES = [
    ("common", 360, 640, 2, 0, 11, False),        # horizontal 6.4x reduce (ksize 27), vertical upscale
    ("tall", 640, 360, 1, 0, 12, False),          # a portrait source: horizontal 3.6x reduce, vertical upscale
    ("odd", 97, 131, 1, 0, 13, False),            # odd sizes, bounds clipped at both borders
    ("up", 40, 50, 1, 0, 14, False),              # upscaled both ways
    ("hd", 1080, 1920, 1, 0, 15, False),          # the widest filter: 19.2x reduce, ksize 79; vertical 1.2x reduce
    ("thin", 1000, 80, 1, 0, 16, False),          # vertical reduce with horizontal upscale
    ("edge", 360, 640, 0, 1, 17, True),           # one hard-edged black / white frame: both clips
]
SAMPLES = 4096


def case_frames(case) -> np.ndarray:
    _, H, W, ns, ne, seed, _ = case
    parts = ([synthetic_video_frames(ns, H, W, seed)] if ns else []) + ([synthetic_edge_frames(ne, H, W, seed + 100)] if ne else [])
    return np.concatenate(parts)


def md5s(a: np.ndarray) -> np.ndarray:
    return np.array([hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in a])


def pillow_piano_frames_portrait(frames: np.ndarray) -> np.ndarray:
    """(F, H, W, 3) uint8 -> (F, 100, 900) float32 through Pillow, step by step as the reference applies it."""
    from PIL import Image
    out = []
    for f in frames:
        grey = np.array(Image.fromarray(f).convert("L"))
        img = Image.fromarray(grey.astype(np.uint8)).resize((100, 900))
        x = np.transpose(np.reshape(img, (900, 100, 1)), [2, 1, 0])
        out.append(x / 255.)
    return np.concatenate(out).astype(np.float32)


def main():
    import PIL
    out, meta = {}, dict(pillow=PIL.__version__, numpy=np.__version__, cases=[list(c) for c in CASES])
    rng = np.random.default_rng(2025)
    for case in CASES:
        name, H, W, _, _, _, overshoot = case
        fr = case_frames(case)
        ref = pillow_piano_frames_portrait(fr)
        plan = PianoFramePlan(H, W, layout="portrait")
        hs, vs = plan.integer_passes(fr)
        assert np.array_equal(plan.preprocess_numpy(fr), ref), f"{name}: the integer restatement differs from Pillow"
        rng_txt = f"horizontal sums [{hs.min()}, {hs.max()}], vertical sums [{vs.min()}, {vs.max()}]"
        if overshoot:
            assert hs.min() < 0 and hs.max() > 255 and vs.min() < 0 and vs.max() > 255, f"{name}: no overshoot on some side: {rng_txt}"
        idx = np.sort(rng.choice(ref[0].size, size=SAMPLES, replace=False))
        out[name + "_frames_md5"] = md5s(fr)
        out[name + "_out_md5"] = md5s(ref)
        out[name + "_idx"] = idx
        out[name + "_vals"] = ref.reshape(len(fr), -1)[:, idx]
        print(f"{name}: {len(fr)} x {H}x{W}, ksize {plan.hk.shape[1]} / {plan.vk.shape[1]}, rows {plan.rows}, {rng_txt}", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "piano_frames_portrait.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
