#!/usr/bin/env python3
"""Time Video2RollEngine.encode_frames on one 251-frame clip for a list of chunk sizes (tuning aid).
usage: python scripts/v2r_probe.py [--compute bf16|bf16x3|fp32 ...] 25 50 126 251
Several --compute values are timed side by side; no chunk size = the engine's default for that mode."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import v2a_amd  # noqa: E402,F401
from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames  # noqa: E402
from v2a_amd.video2roll import Video2RollEngine  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--compute", action="append", choices=["bf16", "bf16x3", "fp32"], help="engine mode (repeatable; default bf16)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("chunks", type=int, nargs="*")
a = ap.parse_args()

sd = random_video2roll_state_dict(0)
x = synthetic_piano_frames(1, 251, seed=0).to("cuda")
for mode in a.compute or ["bf16"]:
    for ch in a.chunks or [None]:
        eng = Video2RollEngine(sd, "cuda", compute=mode, chunk=ch)
        eng.encode_frames(x, 750)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            eng.encode_frames(x, 750)
        torch.cuda.synchronize()
        print(f"{mode:6s} chunk {eng.chunk:4d}: {(time.perf_counter() - t0) / a.reps * 1e3:7.2f} ms per 251-frame clip", flush=True)
        del eng
        torch.cuda.empty_cache()
