"""Generates tests/golden/encodec_rvq.npz by running the third-party library's own quantizer in float64 on the CPU.

`EncodecModel.encode` / `.decode` put `EncodecResidualVectorQuantizer` (transformers/models/encodec/modeling_encodec.py) between the
encoder and the decoder.  The facebook/encodec_24khz checkpoint cannot be fetched offline; the class is built from
`EncodecConfig(target_bandwidths=[1.5, 3, 6, 12, 24])` (the checkpoint's: 32 codebooks of 1024 x 128 at 75 Hz), loaded with seeded
codebooks (v2a_amd.synth.random_encodec_quantizer_state_dict) and run in float64 at 24 kbps on seeded latents
(v2a_amd.synth.synthetic_encodec_latents), which the tests regenerate from the seed and check by md5.

Two families of latents -- `structured` (a sum of one random codeword per stage plus 30 % noise: what an encoder emits) and `gaussian`
-- at (2, 128, 750), (3, 128, 17) and (1, 128, 1).  Per case `<family>_<b>x<t>_*`:
  codes       int16 (32, b, t), `quantizer.encode(x, 24.0)`
  dec_idx     int32 (n, 3) sampled (batch, channel, frame) positions, dec_val float64 (n,) `quantizer.decode(codes)` there
  resid_norm  float64 (b, t), |x - quantizer.decode(codes)| per frame

Usage:  python scripts/make_golden_encodec_rvq.py
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
import v2a_amd  # noqa: E402,F401
from v2a_amd.encodec import quantizer_codebooks  # noqa: E402
from v2a_amd.synth import random_encodec_quantizer_state_dict, synthetic_encodec_latents  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "encodec_rvq.npz")
PARAM_SEED, INPUT_SEED = 8642, 975
SHAPES = ((2, 750), (3, 17), (1, 1))
FAMILIES = ("structured", "gaussian")
BANDWIDTHS = [1.5, 3.0, 6.0, 12.0, 24.0]


def case_seed(family: str, b: int, t: int) -> int:
    return INPUT_SEED + 1000 * FAMILIES.index(family) + 10 * t + b


def main():
    import transformers
    from transformers import EncodecConfig
    from transformers.models.encodec.modeling_encodec import EncodecResidualVectorQuantizer
    torch.set_grad_enabled(False)
    sd = random_encodec_quantizer_state_dict(PARAM_SEED)
    q = EncodecResidualVectorQuantizer(EncodecConfig(target_bandwidths=BANDWIDTHS)).eval()
    q.load_state_dict(sd, strict=True)
    q = q.double()
    cb = quantizer_codebooks(sd)
    meta = dict(param_seed=PARAM_SEED, bandwidth=24.0, dtype="float64", transformers=transformers.__version__, torch=torch.__version__,
                numpy=np.__version__, codebooks_md5=hashlib.md5(cb.numpy().tobytes()).hexdigest(), cases={})
    rec = {}
    for family in FAMILIES:
        for b, t in SHAPES:
            seed = case_seed(family, b, t)
            x = synthetic_encodec_latents(cb, b, t, seed, structured=family == "structured")
            codes = q.encode(x.double(), 24.0)                                     # (32, b, t)
            assert codes.shape == (32, b, t) and int(codes.max()) < 1024
            dec = q.decode(codes)                                                  # (b, 128, t) float64
            name = f"{family}_{b}x{t}"
            rs = np.random.RandomState(23)
            n = min(4096, dec.numel())
            ii = np.stack([rs.randint(0, b, n), rs.randint(0, 128, n), rs.randint(0, t, n)], 1).astype(np.int32)
            rec[name + "_codes"] = codes.numpy().astype(np.int16)
            rec[name + "_dec_idx"], rec[name + "_dec_val"] = ii, dec.numpy()[tuple(ii.T)]
            rec[name + "_resid_norm"] = (x.double() - dec).norm(dim=1).numpy()
            meta["cases"][name] = dict(seed=seed, md5=hashlib.md5(x.numpy().tobytes()).hexdigest())
            # what the library's own fp32 arithmetic makes of the same input: frames whose codes differ from the float64 run
            c32 = q.float().encode(x, 24.0)
            q = q.double()
            meta["cases"][name]["library_fp32_differing_frames"] = int((c32 != codes).any(0).sum())
            print(name, "frames", b * t, "library fp32 vs float64 differing frames", meta["cases"][name]["library_fp32_differing_frames"])
    rec["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
