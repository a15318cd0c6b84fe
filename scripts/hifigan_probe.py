"""Measure v2a_amd.HiFiGAN at the shipped shape (HIFIGAN_16K_64, 55 M seeded weights, v2a_amd.synth) on one 10 s clip (T = 1000 frames ->
160 032 samples) and on 8 clips.  Sections, chosen with --sections (each can run in a call of its own):

  accuracy  the table of tests/test_hifigan_gpu.py: max |x - x64| / error scale per case, path and tap (its helper is imported);
  total     device time of HiFiGAN.decode with fused=True and fused=False, of the same network from torch fp32 ops on the same GPU
            (tests/hifigan_ref.py) and, with --cpu, on this host's CPU;
  shapes    per narrow stage shape (C = 128, 64, 32 at the frames of T) and per (k, d): v2a_hifigan_conv against the composition of
            the same convolution (v2a_hifigan_act_pad + the v2a_gemm chain), same inputs, same session, with the necessary-traffic
            rate of the direct kernel: input rows read once, output rows written once, the weights once;
  chunks    HiFiGAN.decode with other K chunks than K_CHUNK: device time and the largest accuracy ratio of the full configuration's cases;
  trace     nothing but a few decode calls, for `rocprofv3 --kernel-trace --stats -- python scripts/hifigan_probe.py --sections trace`.

Device events around `--iters` calls form one window; the runs alternate window by window for `--rounds` rounds after a warm-up, and the
tables give the median and the min - max spread over the rounds.  The times are recorded, not asserted.

    python scripts/hifigan_probe.py [--sections accuracy,total,shapes] [--frames 1000] [--clips 1,8] [--cpu] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(runs, a):
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window_ms(fn, a.iters))
    return t


def accuracy_lines():
    import numpy as np
    import hifigan_ref as R
    import test_hifigan_gpu as G
    from v2a_amd.hifigan import K_CHUNK
    gold = dict(np.load(R.GOLDEN, allow_pickle=False))
    lines = [f"accuracy (tests/test_hifigan_gpu.py): max |x - x64| / error scale per tap, the largest over the clips of a case; the error scale is the "
             f"reference module's own max |fp32 - float64| over the configuration's cases; the tests assert <= 4.  K_CHUNK = {K_CHUNK}"]
    worst = (0.0, None)
    for cfg in G.CASES:
        for case in G.CASES[cfg]:
            for fused in (True, False):
                r = G.tap_ratios(G.engine(cfg, fused), cfg, case, gold)
                worst = max(worst, max((v, f"{k} of {cfg} {case} fused={fused}") for k, v in r.items()))
                lines.append("%-6s %-7s fused=%-5s " % (cfg, case, fused) + " ".join(f"{k} {v:.2f}" for k, v in r.items()))
    lines.append("largest ratio over every case, path and tap: %.2f (%s)" % worst)
    return lines


def summarise(path, label):
    """Per-kernel lines of a `rocprofv3 --kernel-trace --stats` kernel_stats CSV, template arguments dropped, kernels of one name added."""
    import csv
    import re
    agg = {}
    for row in csv.DictReader(open(path)):
        name = re.sub(r"^void ", "", row["Name"]).replace("(anonymous namespace)::", "")
        name = re.sub(r"\(.*$", "", name)
        name = re.sub(r"<.*$", "", name) if not name.startswith("hifigan") else name
        e = agg.setdefault(name, [0, 0.0])
        e[0] += int(row["Calls"])
        e[1] += float(row["TotalDurationNs"])
    total = sum(v[1] for v in agg.values())
    lines = [f"{label}: {total / 1e6:.2f} ms of kernels in the traced process (3 decode calls, weights and buffers made on the way)"]
    for name, (calls, ns) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:14]:
        lines.append("  %-64s %6d launches %10.3f ms %6.1f %%" % (name[:64], calls, ns / 1e6, 100.0 * ns / total))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", nargs=2, metavar=("CSV", "LABEL"), default=None, help="print the per-kernel share of a kernel_stats CSV and exit")
    ap.add_argument("--sections", default="accuracy,total,shapes")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--clips", default="1,8")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.summarise:
        print("\n".join(summarise(*a.summarise)))
        return
    sections = a.sections.split(",")
    import hifigan_ref as R
    from v2a_amd import HiFiGAN
    from v2a_amd import hifigan as H
    from v2a_amd.synth import synthetic_log_mel
    assert torch.cuda.is_available(), "hifigan_probe needs a GPU"
    dev, T = "cuda:0", a.frames
    lines = []
    if "accuracy" in sections:
        lines += accuracy_lines() + [""]
    sd = R.state_dict("full")
    cfg = R.CONFIGS["full"]
    if "total" in sections or "shapes" in sections or "trace" in sections:
        fused, comp = HiFiGAN(sd, dev, fused="all"), HiFiGAN(sd, dev, fused=False)
    if "trace" in sections:
        for b in (int(v) for v in a.clips.split(",")):
            x = synthetic_log_mel(b, T, 64, 5).to(dev)
            for _ in range(3):
                fused.decode(x)
        torch.cuda.synchronize()
    if "total" in sections:
        sd_gpu = {k: v.to(dev) for k, v in sd.items()}
        lines.append(f"timings: clips of T = {T} frames -> {H.output_length(T)} samples; {a.rounds} rounds of {a.iters} calls per run, alternating, device "
                     f"events, profiler off; every GEMM in K chunks of {H.K_CHUNK}")
        slen = H.stage_lengths(T, cfg["upsample_rates"], cfg["upsample_kernel_sizes"])
        flop = 2.0 * T * 7 * 64 * 1024
        for i, (k, u) in enumerate(zip(cfg["upsample_kernel_sizes"], cfg["upsample_rates"])):
            c = 1024 >> (i + 1)
            flop += 2.0 * slen[i] * k * 2 * c * c + sum(2.0 * slen[i + 1] * rk * c * c * 6 for rk in cfg["resblock_kernel_sizes"])
        flop += 2.0 * slen[-1] * 7 * 32
        for b in (int(v) for v in a.clips.split(",")):
            x = synthetic_log_mel(b, T, 64, 5).to(dev)
            with torch.no_grad():
                runs = {"HIP  HiFiGAN.decode, fused=\"all\" (v2a_hifigan_conv at C = 128, 64, 32)": lambda: fused.decode(x),
                        "HIP  HiFiGAN.decode, fused=False (GEMM composition everywhere)": lambda: comp.decode(x),
                        "torch fp32 ops on the GPU (tests/hifigan_ref.py)": lambda: R.generator(sd_gpu, x, cfg, torch.float32)["wave"]}
                t = alternate(runs, a)
                got, alt, want = fused.decode(x), comp.decode(x), R.generator(sd_gpu, x, cfg, torch.float32)["wave"]
            lines.append("")
            lines.append("%-80s %10s %10s %10s" % ("%d clip%s per call" % (b, "" if b == 1 else "s"), "median ms", "min ms", "max ms"))
            for k, v in t.items():
                lines.append("%-80s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
            call = statistics.median(t[next(iter(runs))])
            lines.append("convolutions of a call: %.1f GFLOP (the taps the transposed convolutions need, not the polyphase zeros) -> %.1f TFLOP/s of the "
                         "fused call (exact fp32); max |HIP - torch GPU| fused %.2e, composition %.2e"
                         % (b * flop / 1e9, b * flop / call / 1e9, float((got - want).abs().max()), float((alt - want).abs().max())))
            if a.cpu and b == 1:
                xc, ts = x.cpu(), []
                with torch.no_grad():
                    R.generator(sd, xc, cfg, torch.float32)
                    for _ in range(3):
                        t0 = time.perf_counter()
                        R.generator(sd, xc, cfg, torch.float32)
                        ts.append((time.perf_counter() - t0) * 1e3)
                lines.append("%-80s %10.1f %10.1f %10.1f" % ("torch fp32 ops on the host CPU, %d threads" % torch.get_num_threads(), statistics.median(ts), min(ts),
                                                              max(ts)))
        lines.append("")
    if "shapes" in sections:
        lines.append(f"per stage shape, one convolution: v2a_hifigan_conv (leaky ReLU and padding inside) against v2a_hifigan_act_pad + the v2a_gemm chain "
                     f"(K chunks of {H.K_CHUNK}); GB/s = 4 (2 b n C + k C C) bytes over the direct kernel's time")
        lines.append("%-34s %12s %12s %8s %10s" % ("b  C  frames  k  d", "direct ms", "composed ms", "ratio", "GB/s"))
        for b in (int(v) for v in a.clips.split(",")):
            geo = fused._geometry(b, T)
            slen, pitch, chans = geo
            buf = fused._buffers(b, T)
            wf, wc = fused._weights(), comp._weights()
            for s in range(1, len(chans)):
                C, n = chans[s], slen[s]
                if C not in H.FUSED_CHANNELS:
                    continue
                for j, rk in enumerate(cfg["resblock_kernel_sizes"]):
                    for m, d in enumerate(cfg["resblock_dilation_sizes"][j]):
                        cf, cc = wf["stages"][s - 1]["blocks"][j]["c1"][m], wc["stages"][s - 1]["blocks"][j]["c1"][m]

                        def composed():
                            comp._act_pad([buf["u"]], pitch[s], b, n, C, None, 1.0, H.LRELU_SLOPE, buf["op"], pitch[s], comp.halo)
                            comp._conv_gemm(cc, buf["op"], d, buf["t"], pitch[s], b, n)

                        with torch.no_grad():
                            t = alternate({"direct": lambda: fused._conv_fused(cf, buf["u"], d, buf["t"], pitch[s], b, n, None), "composed": composed}, a)
                        td, tc = statistics.median(t["direct"]), statistics.median(t["composed"])
                        lines.append("%-34s %12.4f %12.4f %8.2f %10.0f" % (f"{b}  {C}  {n}  {rk}  {d}", td, tc, tc / td, 4.0 * (2 * b * n * C + rk * C * C) / td / 1e6))
        lines.append("")
    if "chunks" in sections:
        import numpy as np
        import test_hifigan_gpu as G
        gold = dict(np.load(R.GOLDEN, allow_pickle=False))
        lines.append("K of one GEMM launch (k_chunk), fused=\"all\": device time of a decode call and the largest accuracy ratio over the taps of the "
                     "full configuration's t16 and ragged cases")
        lines.append("%-10s %16s %16s %14s" % ("k_chunk", "1 clip, ms", "8 clips, ms", "worst ratio"))
        engines = {kc: HiFiGAN(sd, dev, fused="all", k_chunk=kc) for kc in (128, 256, 512, 1024)}
        xs = {b: synthetic_log_mel(b, T, 64, 5).to(dev) for b in (1, 8)}
        with torch.no_grad():
            t = {b: alternate({kc: (lambda v=v, b=b: v.decode(xs[b])) for kc, v in engines.items()}, a) for b in (1, 8)}
        for kc, v in engines.items():
            worst = max(max(G.tap_ratios(v, "full", case, gold).values()) for case in ("t16", "ragged"))
            lines.append("%-10d %16.3f %16.3f %14.2f" % (kc, statistics.median(t[1][kc]), statistics.median(t[8][kc]), worst))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
