"""Time v2a_amd.WaveFrontEnd (resample to 24 kHz + normalize_wav) on one 10 s clip at 48 000, 44 100, 22 050 and 11 025 Hz on one
GPU -- the first three keep the filter table in LDS, the last reads it from global memory -- alone and in front of
v2a_amd.EncodecEncoder, next to the encoder alone and to the fp32 `conv1d` restatement of the resampler on this host's CPU.

Device events around `--iters` calls form one window; the runs alternate window by window for `--rounds` rounds after a warm-up,
and the table gives the median and the min - max spread over the rounds.

    python scripts/wave_front_end_probe.py [--iters 20] [--rounds 7] [--out table.txt] [--no-cpu] [--no-encoder]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATES = (48000, 44100, 22050, 11025)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def cpu_resample(x, table, width, o, n):
    """The fp32 `conv1d` restatement of torchaudio's `_apply_sinc_resample_kernel` with the float64-built table."""
    y = F.conv1d(F.pad(x[None, None], (width, width + o)), table[:, None, :], stride=o)
    return y[0].t().reshape(-1)[:-(-n * x.shape[0] // o)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from v2a_amd import EncodecEncoder, WaveFrontEnd
    from v2a_amd.synth import random_encodec_encoder_state_dict, synthetic_wave
    from v2a_amd.wave import sinc_resample_table, table_in_lds
    assert torch.cuda.is_available(), "wave_front_end_probe needs a GPU"
    fe = WaveFrontEnd("cuda:0")
    enc = None if a.no_encoder else EncodecEncoder(random_encodec_encoder_state_dict(0), "cuda:0")
    waves = {r: synthetic_wave(int(round(r * a.seconds)), 1, r).to("cuda:0") for r in RATES}
    w24 = synthetic_wave(int(round(24000 * a.seconds)), 1).to("cuda:0")
    runs, note = {}, {}
    for r in RATES:
        t, width, o, n = fe.table(r)
        lds = table_in_lds(o, n, t.shape[1])
        note[r] = "%d x %d table, %s" % (t.shape[0], t.shape[1], "LDS" if lds else "global")
        runs["%5d Hz  resample" % r] = lambda r=r: fe.resample(waves[r], r)
        runs["%5d Hz  resample + normalize" % r] = lambda r=r: fe(waves[r], r)
        if enc is not None:
            runs["%5d Hz  front end + encoder" % r] = lambda r=r: enc.encode_list([fe(waves[r], r)])
    runs["24000 Hz  stats + normalize"] = lambda: fe(w24, 24000)
    if enc is not None:
        runs["24000 Hz  encoder alone"] = lambda: enc.encode_list([w24])
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            ms[k].append(window_ms(fn, a.iters))
    lines = [f"one {a.seconds:.1f} s clip per call; {a.rounds} rounds of {a.iters} calls per run, alternating, device events, profiler off",
             "tables: " + "; ".join("%d Hz: %s" % (r, note[r]) for r in RATES),
             "%-36s %10s %10s %10s" % ("per clip", "median ms", "min ms", "max ms")]
    for k, v in ms.items():
        lines.append("%-36s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
    if not a.no_cpu:
        for r in RATES:
            t, width, o, n = sinc_resample_table(r, 24000)
            x = waves[r].cpu()
            got = fe.resample(waves[r], r).cpu()
            ts = []
            with torch.no_grad():
                ref = cpu_resample(x, t, width, o, n)
                for _ in range(5):
                    t0 = time.perf_counter()
                    cpu_resample(x, t, width, o, n)
                    ts.append((time.perf_counter() - t0) * 1e3)
            lines.append("%-36s %10.2f %10.2f %10.2f   (torch fp32 conv1d, %d threads; max |HIP - CPU| = %.2e)"
                         % ("%5d Hz  CPU conv1d resample" % r, statistics.median(ts), min(ts), max(ts), torch.get_num_threads(),
                            float((got - ref).abs().max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
