"""Measure v2a_amd.AudioLDMVaeDecoder at the shipped shape (AUDIOLDM_VAE, 33 M seeded weights, v2a_amd.synth) on one 10 s clip (l = 250
latent frames -> a 1000 x 64 mel image) and on 8 clips.  Sections, chosen with --sections (each can run in a call of its own):

  accuracy  the table of tests/test_audioldm_vae_gpu.py: max |x - x64| / error scale per case, regime and tap (its helper is imported);
  total     device time of AudioLDMVaeDecoder.decode_latents, of the same network from torch fp32 ops on the same GPU (tests/audioldm_vae_ref.py,
            channels-last) and, with --cpu, on this host's CPU at 16 threads;
  kernels   per-kernel shares of one decode call: every launch between its own pair of device events (v2a_amd._lib.KernelProfiler), added
            up by kernel -- the GEMMs by epilogue, the two GroupNorm kernels, softmax, upsample, the rest;
  gn        the GroupNorm pair on the largest map (l x 4 rows of 64 bins, 128 channels): time against its necessary traffic (the map read
            twice, the bordered map written once) and against a device-to-device copy of the same map.

Device events around `--iters` calls form one window; the runs alternate window by window for `--rounds` rounds after a warm-up, and the
tables give the median and the min - max spread over the rounds.  The times are recorded, not asserted.

    python scripts/audioldm_vae_probe.py [--sections accuracy,total,kernels,gn] [--frames 250] [--clips 1,8] [--cpu] [--out FILE]
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


def fmt(ts):
    return "%9.3f ms (min %.3f, max %.3f over %d rounds)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def accuracy_lines():
    import numpy as np
    import audioldm_vae_ref as R
    import test_audioldm_vae_gpu as G
    from v2a_amd.audioldm_vae import K_CHUNK
    gold = dict(np.load(R.GOLDEN, allow_pickle=False))
    lines = [f"accuracy (tests/test_audioldm_vae_gpu.py): max |x - x64| / error scale per tap, the largest over the clips of a case; the error scale is "
             f"the reference module's own max |fp32 - float64| over the cases of the configuration and regime; the tests assert <= 4.  K_CHUNK = {K_CHUNK}"]
    worst = (-1.0, "")
    for cfg in G.CASES:
        for regime in R.REGIMES:
            for case in G.CASES[cfg]:
                r = G.tap_ratios(G.engine(cfg, regime), cfg, regime, case, gold)
                worst = max(worst, max((v, f"{k} of {cfg} {regime} {case}") for k, v in r.items()))
                lines.append("%-6s %-7s %-7s " % (cfg, regime, case) + " ".join(f"{k} {v:.2f}" for k, v in r.items()))
    lines.append("largest ratio over every case, regime and tap: %.2f (%s)" % worst)
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="accuracy,total,kernels,gn")
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--clips", default="1,8")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    sections = a.sections.split(",")
    import audioldm_vae_ref as R
    from v2a_amd import AudioLDMVaeDecoder, _lib as L
    from v2a_amd.synth import synthetic_vae_latents
    dev = "cuda:0"
    lines = [f"# scripts/audioldm_vae_probe.py --sections {a.sections} --frames {a.frames} --clips {a.clips} --iters {a.iters} --rounds {a.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    if "accuracy" in sections:
        lines += accuracy_lines() + [""]
    sd = R.state_dict("full", "plain")
    dec = AudioLDMVaeDecoder(sd, dev)
    l = a.frames
    for b in [int(v) for v in a.clips.split(",")]:
        emb = synthetic_vae_latents(b, l, 128, 9).to(dev)
        if "total" in sections:
            p32 = {k: v.to(dev) for k, v in sd.items()}
            z = R.to_z(emb).contiguous(memory_format=torch.channels_last)
            p32 = {k: (v.contiguous(memory_format=torch.channels_last) if v.ndim == 4 else v) for k, v in p32.items()}
            runs = {"hip": lambda: dec.decode_latents(emb), "torch": lambda: R.decoder(p32, z, R.CONFIGS["full"], 1.0, torch.float32)["mel"]}
            t = alternate(runs, a)
            diff = float((runs["hip"]()[:, :, :, :] - runs["torch"]()).abs().max())
            flops = 0.65e12 * l / 250 * b
            lines.append(f"total, {b} clip(s) of l = {l} ({4 * l} x 64 mel rows each), fp32:")
            lines.append("  AudioLDMVaeDecoder.decode_latents        " + fmt(t["hip"]) + "  = %.1f TFLOP/s of the network's 0.65 TFLOP per 10 s clip" %
                         (flops / statistics.median(t["hip"]) / 1e9))
            lines.append("  torch fp32 ops, same GPU, channels-last  " + fmt(t["torch"]) + "  (max |delta mel| between the two: %.3e)" % diff)
            del p32
            if a.cpu and b == 1:
                torch.set_num_threads(16)
                zc = R.to_z(emb.cpu())
                t0 = time.perf_counter()
                R.decoder(sd, zc, R.CONFIGS["full"], 1.0, torch.float32)
                lines.append("  torch fp32 ops, host CPU, 16 threads     %9.3f ms (one call)" % ((time.perf_counter() - t0) * 1e3))
            torch.cuda.empty_cache()
        if "kernels" in sections:
            dec.decode_latents(emb)
            torch.cuda.synchronize()
            prof = L.KernelProfiler()
            L.set_profiler(prof)
            try:
                dec.decode_latents(emb)
            finally:
                L.set_profiler(None)
            agg = prof.summary()
            total = sum(v["ms"] for v in agg.values())
            lines.append(f"kernels, {b} clip(s) of l = {l}: {total:.3f} ms summed over {sum(v['launches'] for v in agg.values())} launches, each between its own "
                         f"pair of events (an eager pair includes the dispatch gap: the sum exceeds the call's device time)")
            for name, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
                rate = "%7.1f TFLOP/s" % (v["flops"] / v["ms"] / 1e9) if name.startswith("gemm") else "%7.0f GB/s of its necessary traffic" % (v["bytes"] / v["ms"] / 1e6)
                lines.append("  %-44s %5d launches %9.3f ms %5.1f %%  %s" % (name, v["launches"], v["ms"], 100 * v["ms"] / total, rate))
        if "gn" in sections:
            H, W, C = 4 * l, 64, 128
            pitch = (H + 2) * (W + 2)
            x = torch.randn(b * pitch * C, device=dev)
            out = torch.empty_like(x)
            g = torch.ones(C, device=dev)
            buf = dict(part=torch.zeros(b * ((H * W + 511) // 512) * 64, dtype=torch.float64, device=dev))
            runs = {"gn": lambda: dec._norm(dict(g=g, b=g), x, pitch, W + 2, (H, W, pitch), b, C, None, True, out, pitch, 1, buf),
                    "copy": lambda: out.copy_(x)}
            t = alternate(runs, a)
            need = 4.0 * b * C * (2 * H * W + pitch)
            lines.append(f"GroupNorm pair, {b} map(s) of {H} x {W} x {C}: gn_stats + gn_act_pad " + fmt(t["gn"]) +
                         "  = %.0f GB/s of its necessary traffic (%.1f MB: the map read twice, the bordered map written once)" %
                         (need / statistics.median(t["gn"]) / 1e6, need / 1e6))
            lines.append("  device-to-device copy of the same map (read once, written once)  " + fmt(t["copy"]) +
                         "  = %.0f GB/s" % (8.0 * b * pitch * C / statistics.median(t["copy"]) / 1e6))
            del x, out
            torch.cuda.empty_cache()
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
