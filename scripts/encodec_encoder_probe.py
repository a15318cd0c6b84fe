"""Time v2a_amd.EncodecEncoder on one 10 s clip (240 000 samples, seeded weights and wave) on one GPU, in both `fused_stem` settings,
next to v2a_amd.EncodecDecoder (750 frames, the mirrored network) in the same run and the CPU library's fp32 encoder on this host.

Device events around `--iters` calls form one window; the three engines alternate window by window for `--rounds` rounds after a
warm-up, and the table gives the median and the min - max spread over the rounds.  Layers 0 - 1 alone (the fused kernel against
its composition) are timed the same way.

    python scripts/encodec_encoder_probe.py [--iters 20] [--rounds 7] [--out table.txt] [--no-cpu]
    rocprofv3 --kernel-trace --stats -- python scripts/encodec_encoder_probe.py --trace      (a few calls of each, no timing)
    python scripts/encodec_encoder_probe.py --summarise DIR                                   (kernel_stats.csv -> table)
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def summarise(directory):
    """Per-kernel table from the kernel_stats.csv rocprofv3 --stats left under `directory`."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    rows = list(csv.DictReader(open(paths[0])))
    lines = ["%-92s %7s %10s %10s %6s" % ("kernel", "calls", "us/call", "total ms", "%")]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        lines.append("%-92s %7d %10.1f %10.2f %6.1f" % (r["Name"][:92], int(r["Calls"]), float(r["AverageNs"]) / 1e3,
                                                       float(r["TotalDurationNs"]) / 1e6, float(r["Percentage"])))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=240000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--trace", action="store_true", help="3 calls of each engine after a warm-up, nothing timed (for rocprofv3)")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.summarise:
        text = summarise(a.summarise)
        print(text)
        if a.out:
            open(a.out, "w").write(text + "\n")
        return
    from v2a_amd.encodec import EncodecDecoder, EncodecEncoder
    from v2a_amd.synth import random_encodec_decoder_state_dict, random_encodec_encoder_state_dict, synthetic_wave
    assert torch.cuda.is_available(), "encodec_encoder_probe needs a GPU"
    n = a.samples
    esd = random_encodec_encoder_state_dict(0)
    fused, composed = EncodecEncoder(esd, "cuda:0"), EncodecEncoder(esd, "cuda:0", fused_stem=False)
    dec = EncodecDecoder(random_encodec_decoder_state_dict(0), "cuda:0")
    wave = synthetic_wave(n, 1).to("cuda:0")
    w3 = wave.view(1, 1, n)
    z = fused.encoder(w3)
    diff = float((z - composed.encoder(w3)).abs().max())
    runs = {"encoder, fused stem": lambda: fused.encoder(w3), "encoder, composed stem": lambda: composed.encoder(w3),
            "decoder": lambda: dec.decoder(z),
            "layers 0-1 alone, fused": lambda: fused._stage0(wave, n), "layers 0-1 alone, composed": lambda: composed._stage0(wave, n)}
    if a.trace:
        for fn in runs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        return
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            ms[k].append(window_ms(fn, a.iters))
    lines = [f"{n} samples ({n / 24000:.1f} s) -> {z.shape[2]} frames; {a.rounds} rounds of {a.iters} calls per engine, alternating, device events, "
             f"profiler off; max |fused - composed| = {diff:.2e}",
             "%-30s %10s %10s %10s" % ("per clip", "median ms", "min ms", "max ms")]
    for k, v in ms.items():
        lines.append("%-30s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
    if not a.no_cpu:
        from transformers import EncodecConfig, EncodecModel
        ref = EncodecModel(EncodecConfig()).eval().encoder
        ref.load_state_dict(esd, strict=True)
        wc = w3.cpu()
        ts = []
        with torch.no_grad():
            ref(wc)
            for _ in range(5):
                t0 = time.perf_counter()
                zc = ref(wc)
                ts.append((time.perf_counter() - t0) * 1e3)
        lines.append("%-30s %10.1f %10.1f %10.1f   (transformers fp32, %d threads; max |HIP - library| = %.2e)"
                     % ("CPU library encoder", statistics.median(ts), min(ts), max(ts), torch.get_num_threads(), float((z.cpu() - zc).abs().max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
