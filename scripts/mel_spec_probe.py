"""Measure v2a_amd.MelSpec (reflect pad, DFT as exact-fp32 GEMMs over overlapping rows, magnitude + mel + log) at the default setting
(STFT 1024 / hop 256 / Hann, 100 HTK mel channels, 24 kHz) on one 10 s clip (240 000 samples, T = 938) and on 8 clips:

  * the accuracy table of tests/test_mel_spec_gpu.py: r_gpu and r_cpu32 per case (its helpers are imported, nothing is restated);
  * device time per stage -- pad, the DFT GEMMs, the mel kernel -- and of the whole call;
  * the bytes the mel kernel has to move (the partial DFTs read once, the mel frames written once) over its time, next to the rate of a
    device-to-device copy of as many bytes measured in the same run;
  * the same work from torch ops on the same GPU in fp32 (torch.stft, abs, matmul, clamp, log);
  * the same torch ops on this host's CPU.

Device events around `--iters` calls form one window; the runs alternate window by window for `--rounds` rounds after a warm-up, and the
table gives the median and the min - max spread over the rounds.

    python scripts/mel_spec_probe.py [--iters 50] [--rounds 7] [--out profiles/mel_spec.txt] [--no-cpu] [--no-accuracy]
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


def torch_logmel(x, window, fb, n_fft=1024, hop=256):
    """The reference's module from torch ops in fp32: torch.stft, abs, matmul, clamp, log -> (b, n_mels, T)."""
    S = torch.stft(x, n_fft, hop, n_fft, window=window, center=True, pad_mode="reflect", return_complex=True)
    return torch.matmul(fb.t(), S.abs()).clamp(min=1e-5).log()


def accuracy_lines():
    import test_mel_spec_gpu as T
    lines = ["accuracy against float64 (tests/test_mel_spec_gpu.py): r = max |mel - mel64| / S, S the error scale of its docstring",
             "%-64s %5s %8s %8s" % ("n_fft hop win n_mels sr nw power norm normalize center", "T", "r_gpu", "r_cpu32")]
    for i, case in enumerate(T.CASES):
        x, ref = T.case_data(i)
        mel = T.module(case).mel(x).cpu()
        lines.append("%-64s %5d %8.3f %8.3f" % (" ".join(str(v) for v in case), mel.shape[-1], T.ratio(mel, ref["mel64"], ref["scale"]), ref["r_cpu32"]))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from v2a_amd import MelSpec
    from v2a_amd.mel import mel_filterbank
    from v2a_amd.synth import synthetic_wave
    assert torch.cuda.is_available(), "mel_spec_probe needs a GPU"
    dev = "cuda:0"
    nw = int(round(24000 * a.seconds))
    ms = MelSpec(device=dev)
    window = torch.hann_window(1024, periodic=True, device=dev)
    fb = mel_filterbank(513, 100, 24000).float().to(dev)
    lines = [] if a.no_accuracy else accuracy_lines() + [""]
    lines.append(f"timings: {a.seconds:.1f} s clips of {nw} samples, T = {ms.frames(nw)}; {a.rounds} rounds of {a.iters} calls per run, alternating, device "
                 f"events, profiler off; K in {ms.n_chunks} chunks of 256 samples")
    for b in (1, 8):
        x = torch.stack([synthetic_wave(nw, 10 + i) for i in range(b)]).to(dev)
        T = ms.frames(nw)
        padded, dft, pitch, rows = ms._buffers(b, nw, T)
        out = torch.empty(b, 100, T, device=dev)
        mel_bytes = 4.0 * b * T * (2 * ms.n_bins * ms.n_chunks + 100)          # partial DFTs read once (rows between clips excluded), mel written once
        src = torch.empty(int(mel_bytes // 8), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        runs = {
            "HIP  pad": lambda: ms._stage_pad(x, padded, pitch),
            "HIP  DFT GEMMs (%d x %dx%dx%d)" % (ms.n_chunks, rows, ms.n_pad, 256): lambda: ms._stage_dft(padded, dft, rows),
            "HIP  mel kernel": lambda: ms._stage_mel(dft, pitch, b, T, 1e-5, out),
            "HIP  MelSpec call": lambda: ms(x),
            "torch ops on the GPU (stft, abs, matmul, clamp, log)": lambda: torch_logmel(x, window, fb),
            "copy of the mel kernel's bytes (%.1f MB read + %.1f MB written)" % (mel_bytes / 2e6, mel_bytes / 2e6): lambda: dst.copy_(src),
        }
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        d = float((ms(x) - torch_logmel(x, window, fb)).abs().max())
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(window_ms(fn, a.iters))
        lines.append("")
        lines.append("%-72s %10s %10s %10s" % ("%d clip%s per call" % (b, "" if b == 1 else "s"), "median ms", "min ms", "max ms"))
        for k, v in t.items():
            lines.append("%-72s %10.4f %10.4f %10.4f" % (k, statistics.median(v), min(v), max(v)))
        keys = list(t)
        mel_ms, copy_ms, gemm_ms = statistics.median(t[keys[2]]), statistics.median(t[keys[5]]), statistics.median(t[keys[1]])
        lines.append("mel kernel: %.2f MB necessary (partial DFTs in, mel out) -> %.0f GB/s; the copy of as many bytes runs at %.0f GB/s"
                     % (mel_bytes / 1e6, mel_bytes / mel_ms / 1e6, mel_bytes / copy_ms / 1e6))
        lines.append("DFT GEMMs: %.2f GFLOP -> %.1f TFLOP/s (exact fp32);  max |HIP log-mel - torch GPU log-mel| = %.2e"
                     % (2.0 * rows * ms.n_pad * ms.k_pad / 1e9, 2.0 * rows * ms.n_pad * ms.k_pad / gemm_ms / 1e9, d))
        if not a.no_cpu:
            xc, wc, fc = x.cpu(), window.cpu(), fb.cpu()
            ts = []
            with torch.no_grad():
                torch_logmel(xc, wc, fc)
                for _ in range(7):
                    t0 = time.perf_counter()
                    torch_logmel(xc, wc, fc)
                    ts.append((time.perf_counter() - t0) * 1e3)
            lines.append("%-72s %10.3f %10.3f %10.3f" % ("torch ops on the host CPU, %d threads" % torch.get_num_threads(), statistics.median(ts), min(ts), max(ts)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
