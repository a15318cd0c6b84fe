"""Write tests/golden/video2roll_88.npz: the reference module `Video2RollNet.resnet18(num_classes=88)` of the 88-key piano
configuration (x3_2 = e2_tts_crossatt3_2.py:1523), run in float64 on seeded weights and frames, and the expansion in time of its
`encode_frames` (x3_2:1546-1554) applied to the network's output.  CPU only.

The module is read from `--reference DIR` (`DIR/src/audeo/Video2RollNet.py`, which imports only torch and math) and none of its
text is copied; the five-frame windows come from oracle.video2roll_oracle.frame_windows, and the one expression of x3_2:1546-1547
that the fixture pins is written out once below.
The fixture holds outputs only; weights and frames are regenerated from seeds by v2a_amd.synth (numpy RandomState):
  logits (6, 88) float64       ResNet.forward on the 6 five-frame windows of one 6-frame clip (windows clamp at both ends)
  probs (1, 6, 88) float64     their sigmoid, per video frame
  roll_l13 / roll_l15 / roll_l20 (1, l, 88) float64   encode_frames(x, l): rows x5, cut to (t*5//2)*2, pairs averaged -> d = 15 rows,
                               cropped (l = 13), as they are (15) or zero padded (20)

Usage: python scripts/make_golden_video2roll_88.py --reference DIR
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import v2a_amd  # noqa: E402,F401
from oracle.video2roll_oracle import frame_windows  # noqa: E402
from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames  # noqa: E402

PARAM_SEED, INPUT_SEED = 8801, 88
NOTES, T, LENGTHS = 88, 6, (13, 15, 20)


def load_reference_net(ref_root):
    path = os.path.join(ref_root, "src", "audeo", "Video2RollNet.py")
    spec = importlib.util.spec_from_file_location("ref_Video2RollNet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.resnet18(num_classes=NOTES)
    net.load_state_dict(random_video2roll_state_dict(PARAM_SEED, NOTES), strict=True)      # every key present, none extra
    return net.double().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    net = load_reference_net(args.reference)
    x = synthetic_piano_frames(1, T, seed=INPUT_SEED).double()          # (1, 1, 6, 100, 900)
    b, t = x.shape[0], x.shape[2]
    logits = net(frame_windows(x))                                      # (b * t, 5, 100, 900): frames i - 2 .. i + 2, clamped
    probs = torch.sigmoid(logits)
    rec = dict(logits=logits.numpy(), probs=probs.reshape(b, t, NOTES).numpy())
    for l in LENGTHS:
        t5 = (t * 5 // 2) * 2
        y = probs.reshape(b, t, 1, NOTES).repeat(1, 1, 5, 1).reshape(b, t * 5, NOTES)[:, :t5, :].reshape(b, t5 // 2, 2, NOTES).mean(2)
        out = torch.zeros(b, l, NOTES, dtype=y.dtype)                   # cropped or zero padded to l rows
        out[:, :min(l, y.shape[1])] = y[:, :l]
        rec[f"roll_l{l}"] = out.numpy()
    path = os.path.join(ROOT, "tests", "golden", "video2roll_88.npz")
    np.savez_compressed(path, **rec)
    print("logits", logits.shape, "range", float(logits.min()), float(logits.max()), "mean prob", float(probs.mean()),
          {k: v.shape for k, v in rec.items()}, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
