"""Generates tests/golden/encodec_enc_*.npz by running the third-party library the reference calls, in float64.

The reference's audio encoder is `EncodecModel.from_pretrained("facebook/encodec_24khz").encoder` (x3:421-432, predict.py:222).
The checkpoint cannot be fetched offline; `EncodecModel(EncodecConfig())` is the same architecture (default config ==
encodec_24khz), loaded here with seeded weights (v2a_amd.synth.random_encodec_encoder_state_dict) and run in float64 on seeded
waves (v2a_amd.synth.synthetic_wave).  Taps are the outputs of layers 1, 3, 6, 9, 12 (residual block at C = 32, the four strided
convolutions) and 13 (LSTM + skip).

  encodec_enc_small.npz    n = 2 333 -> 8 frames (right pads 1, 1, 3, 5): the full latent + 256 sampled points of every tap
  encodec_enc_full.npz     n = 240 000 -> 750 frames (no right pad): 4 096 sampled latent points + statistics + taps
  encodec_enc_ragged.npz   n = 196 161 -> 614 frames (right pads 1, 3, 4, 7: the largest each strided layer can take)

Usage:  python scripts/make_golden_encodec_encoder.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import v2a_amd  # noqa: E402,F401
from v2a_amd.encodec import encoder_padding_plan  # noqa: E402
from v2a_amd.synth import random_encodec_encoder_state_dict, synthetic_wave  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PARAM_SEED, INPUT_SEED = 9753, 531
CASES = (("small", 2333), ("full", 240000), ("ragged", 196161))
TAPS = (1, 3, 6, 9, 12, 13)


def main():
    from transformers import EncodecConfig, EncodecModel
    torch.set_grad_enabled(False)
    enc = EncodecModel(EncodecConfig()).eval().encoder
    enc.load_state_dict(random_encodec_encoder_state_dict(PARAM_SEED), strict=True)
    enc = enc.double()
    os.makedirs(OUT, exist_ok=True)
    for name, n in CASES:
        wave = synthetic_wave(n, INPUT_SEED + n)
        taps = {}
        hooks = [enc.layers[i].register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"layer{i}", o.detach().clone())) for i in TAPS]
        z = enc(wave.double().view(1, 1, n))[0].numpy()                            # (128, T) float64
        for h in hooks:
            h.remove()
        plan = encoder_padding_plan(n)
        meta = dict(n=n, frames=int(z.shape[1]), param_seed=PARAM_SEED, input_seed=INPUT_SEED + n, dtype="float64",
                    right_pads=[pr for p, _, pr, _ in plan if p in ("layers.3", "layers.6", "layers.9", "layers.12")])
        rec = dict(meta=np.array(json.dumps(meta)), shape=np.array(z.shape),
                   stats=np.array([z.mean(), np.abs(z).mean(), z.max(), z.min()]))
        rs = np.random.RandomState(17)
        if name == "small":
            rec["z"] = z
        else:
            ii = np.stack([rs.randint(0, z.shape[0], 4096), rs.randint(0, z.shape[1], 4096)], 1)
            rec["z_idx"], rec["z_val"] = ii, z[tuple(ii.T)]
        for k, v in taps.items():
            a = v[0].numpy()                                                       # (C, L)
            ii = np.stack([rs.randint(0, a.shape[0], 256), rs.randint(0, a.shape[1], 256)], 1)
            rec[f"{k}_shape"], rec[f"{k}_idx"], rec[f"{k}_val"] = np.array(a.shape), ii, a[tuple(ii.T)]
            rec[f"{k}_absmean"] = np.array(np.abs(a).mean())
        np.savez_compressed(os.path.join(OUT, f"encodec_enc_{name}.npz"), **rec)
        print(name, meta, "latent abs mean %.4f max %.3f" % (np.abs(z).mean(), np.abs(z).max()),
              {k: round(float(np.abs(v.numpy()).mean()), 4) for k, v in taps.items()})


if __name__ == "__main__":
    main()
