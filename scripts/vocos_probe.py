"""Measure v2a_amd.Vocos at the shape of charactr/vocos-mel-24khz (100 mels, dim 512, hidden 1536, 8 blocks, n_fft 1024, hop 256; seeded
weights, tests/vocos_ref.py) on one 10 s clip (T = 938 frames -> 239 872 samples) and on 8 clips:

  * the accuracy table of tests/test_vocos_gpu.py: r_gpu and r_cpu32 per case and tap (its helpers are imported, nothing is restated);
  * device time per stage -- stage_in, embed + norm, the 8 blocks, final norm + head, spectrum, inverse DFT, overlap-add -- and of the
    whole decode() call;
  * the same network from torch ops on the same GPU (nn modules in fp32 plus torch.istft);
  * the same torch ops on this host's CPU.

Device events around `--iters` calls form one window; the runs alternate window by window for `--rounds` rounds after a warm-up, and the
table gives the median and the min - max spread over the rounds.  The times are recorded, not asserted.

    python scripts/vocos_probe.py [--iters 20] [--rounds 5] [--out profiles/vocos.txt] [--no-cpu] [--no-accuracy]
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


def accuracy_lines():
    import vocos_ref as R
    from v2a_amd import Vocos
    lines = ["accuracy against float64 (tests/test_vocos_gpu.py): r = max |x - x64| / max |x64| per clip, the largest over the clips; the tests "
             "assert r_gpu <= 4 r_cpu32",
             "%-40s %-8s %10s %10s %6s" % ("C dim hidden depth n_fft hop T", "tap", "r_gpu", "r_cpu32", "ratio")]
    worst = (0.0, None)
    for i, case in enumerate(R.CASES):
        d = R.case_data(i)
        taps = {}
        Vocos(d["sd"], "cuda:0", hop_length=d["hop"]).decode(d["x"], taps=taps)
        for name, want in d["t64"].items():
            rg, rc = R.ratio(taps[name].cpu(), want), R.ratio(d["t32"][name], want)
            worst = max(worst, (rg / rc, "%s of case %d" % (name, i)))
            if name in ("embed", "block0", "block%d" % (case[3] - 1), "final", "logits", "S", "wave"):
                lines.append("%-40s %-8s %10.3e %10.3e %6.2f" % (" ".join(str(v) for v in case), name, rg, rc, rg / rc))
    lines.append("largest r_gpu / r_cpu32 over every case and tap: %.2f (%s)" % worst)
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=938)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import vocos_ref as R
    from v2a_amd import Vocos
    from v2a_amd.vocos import K_CHUNK
    assert torch.cuda.is_available(), "vocos_probe needs a GPU"
    dev = "cuda:0"
    T = a.frames
    ref = R.VocosRef(100, 512, 1536, 8, 1024, 256, seed=1).eval()
    voc = Vocos(ref.state_dict(), dev)
    ref_gpu = R.VocosRef(100, 512, 1536, 8, 1024, 256, seed=1).eval()
    ref_gpu.load_state_dict(ref.state_dict())
    ref_gpu = ref_gpu.to(dev)
    lines = [] if a.no_accuracy else accuracy_lines() + [""]
    lines.append(f"timings: clips of T = {T} frames -> {(T - 1) * 256} samples; {a.rounds} rounds of {a.iters} calls per run, alternating, device events, "
                 f"profiler off; every GEMM in K chunks of {K_CHUNK}")
    for b in (1, 8):
        x = R.make_features(b, 100, T, seed=5).to(dev)
        buf = voc._buffers(b, T)
        w = voc._weights()
        out = torch.empty(b, (T - 1) * 256, device=dev)
        voc.decode(x)                                                    # every buffer holds the data of a real call

        def blocks():
            src = 0
            for blk in w["blocks"]:
                voc._stage_block(blk, buf, None, b, T, src)
                src = 1 - src

        logits = voc._stage_head(buf, 0)
        frames = voc._stage_idft(buf)
        with torch.no_grad():
            runs = {
                "HIP  stage_in": lambda: voc._stage_in(x, None, buf, b, T),
                "HIP  embed GEMMs + LayerNorm": lambda: voc._stage_embed(buf),
                "HIP  8 blocks (dwconv_ln, pwconv1, gelu, pwconv2, scale_residual)": blocks,
                "HIP  final LayerNorm + head GEMMs": lambda: voc._stage_head(buf, 0),
                "HIP  spectrum": lambda: voc._stage_spectrum(logits, buf),
                "HIP  inverse DFT GEMMs": lambda: voc._stage_idft(buf),
                "HIP  overlap-add": lambda: voc._stage_overlap_add(frames, buf, None, b, T, out),
                "HIP  Vocos.decode call": lambda: voc.decode(x),
                "torch ops on the GPU (nn modules in fp32, torch.istft)": lambda: ref_gpu(x)["wave"],
            }
            for fn in runs.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            got, want = voc.decode(x), ref_gpu(x)["wave"]
            d = float((got - want).abs().max() / want.abs().max())
            t = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    t[k].append(window_ms(fn, a.iters))
        lines.append("")
        lines.append("%-72s %10s %10s %10s" % ("%d clip%s per call" % (b, "" if b == 1 else "s"), "median ms", "min ms", "max ms"))
        for k, v in t.items():
            lines.append("%-72s %10.4f %10.4f %10.4f" % (k, statistics.median(v), min(v), max(v)))
        M = buf["M"]
        flop = 2.0 * M * (7 * voc.c_pad * 512 + 8 * 2 * 512 * 1536 + 512 * voc.n_logits + voc.k_spec * 1024)
        call = statistics.median(t["HIP  Vocos.decode call"])
        lines.append("GEMMs of a call: %.2f GFLOP over %d rows -> %.1f TFLOP/s of the whole call (exact fp32);  max |HIP wave - torch GPU wave| / max |wave| = %.2e"
                     % (flop / 1e9, M, flop / call / 1e9, d))
        if not a.no_cpu:
            xc, ts = x.cpu(), []
            with torch.no_grad():
                ref(xc)
                for _ in range(5):
                    t0 = time.perf_counter()
                    ref(xc)
                    ts.append((time.perf_counter() - t0) * 1e3)
            lines.append("%-72s %10.3f %10.3f %10.3f" % ("torch ops on the host CPU, %d threads" % torch.get_num_threads(), statistics.median(ts), min(ts), max(ts)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
