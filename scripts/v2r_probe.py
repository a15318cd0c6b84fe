#!/usr/bin/env python3
"""Time Video2RollEngine.encode_frames on one 251-frame clip for a list of chunk sizes (tuning aid).
usage: python scripts/v2r_probe.py [--compute bf16|bf16x3|fp32 ...] 25 50 126 251
Several --compute values are timed side by side; no chunk size = the engine's default for that mode.
--keys 88 (repeatable, beside 51): the 88-key configuration -- 88 classes, a 301-frame clip (30 fps), rows expanded by 5 / 2."""
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
ap.add_argument("--keys", action="append", type=int, choices=[51, 88], help="piano configuration (repeatable; default 51)")
ap.add_argument("chunks", type=int, nargs="*")
a = ap.parse_args()

for keys in a.keys or [51]:
    pc = v2a_amd.piano_config(keys)
    T = int(750 // pc.video_multi) + 1
    sd = random_video2roll_state_dict(0, pc.notes)
    x = synthetic_piano_frames(1, T, seed=0).to("cuda")
    for mode in a.compute or ["bf16"]:
        for ch in a.chunks or [None]:
            eng = Video2RollEngine(sd, "cuda", compute=mode, chunk=ch, expand=pc.expand)
            eng.encode_frames(x, 750)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                eng.encode_frames(x, 750)
            torch.cuda.synchronize()
            tag = "" if keys == 51 else f"{keys} keys "
            print(f"{tag}{mode:6s} chunk {eng.chunk:4d}: {(time.perf_counter() - t0) / a.reps * 1e3:7.2f} ms per {T}-frame clip", flush=True)
            del eng
            torch.cuda.empty_cache()
    # the expansion in time alone (v2a_roll_expand, or v2a_roll_expand_ratio for a group of 2): device events around 200 launches
    from v2a_amd import _lib as L
    roll, out = torch.rand(1, T, pc.notes, device="cuda"), torch.empty(1, 750, pc.notes, device="cuda")
    rep, group = pc.expand
    if group == 1:
        fn = lambda: L.roll_expand(roll, out, B=1, t=T, notes=pc.notes, rep=rep, l=750)
    else:
        fn = lambda: L.roll_expand_ratio(roll, out, B=1, t=T, notes=pc.notes, rep=rep, group=group, l=750)
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        fn()
    e1.record()
    e1.synchronize()
    print(f"{keys} keys: roll expansion x{rep}/{group}, t = {T} -> 750 rows: {e0.elapsed_time(e1) / 200 * 1e3:.2f} us per launch (back to back)", flush=True)
