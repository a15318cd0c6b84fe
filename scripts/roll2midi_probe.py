"""Timing of the Roll2Midi generator (roll2midi.py) on the GPU, and of the reference module on the host's CPU.

  python scripts/roll2midi_probe.py [--out FILE]                   on a machine with an MI355X: per-window and per-clip time in the three
                                                                   compute modes, and the share of the three row kernels
  python scripts/roll2midi_probe.py --reference DIR [--out FILE]   anywhere: the same clip through `Generator` of the reference tree's
                                                                   src/audeo/Roll2MidiNet.py on the CPU (fp32, torch's own threads)

  python scripts/roll2midi_probe.py --enhance [...]                the same for the attention-gated generator (Roll2MidiNet_enhance.py,
                                                                   `Roll2MidiEnhanceEngine`), plus the gate kernel against the same work
                                                                   composed from torch ops and against v2a_leaky_shadow on the same map

A window is 51 keys x 100 frames; a clip is 10 s of 50 fps video = 500 frames = 5 windows, run as `refine` runs them (one pass of 5).
Times are device events around `repeats` back-to-back calls after a warm-up of every shape; the kernel shares come from a separate
pass with one event pair per launch (`_lib.KernelProfiler`), which adds the launch gaps to every kernel and so is only used as a ratio.
FLOP are counted from the layer shapes (2 * pixels * K * N per convolution, the network's own 16 channels for up5), not measured.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import v2a_amd  # noqa: E402,F401
from v2a_amd import _lib as L  # noqa: E402
from v2a_amd.conv2d import ConvMemory  # noqa: E402
from v2a_amd.roll2midi import _DOWN, _GATES, _UP, _UP_ENH, Roll2MidiEngine, Roll2MidiEnhanceEngine  # noqa: E402
from v2a_amd.synth import random_roll2midi_enhance_state_dict, random_roll2midi_state_dict, synthetic_key_roll  # noqa: E402

KEYS, WINDOW, CLIP_WINDOWS = 51, 100, 5
BF16_MFMA_PEAK = 2516.6e12          # dense bf16 MFMA rate of an MI355X, FLOP/s (spec)


def window_flop(keys=KEYS, w=WINDOW, enhance=False) -> float:
    """Counted per window.  Enhanced net: its own convolutions, conv1d over 128 channels and the gates as folded (one dot per pixel)."""
    if enhance:
        kn = sum(9 * ci * co for ci, co in _DOWN + _UP_ENH) + 128 + sum(c for c, _, _ in _GATES)
    else:
        kn = sum(9 * ci * co for ci, co in _DOWN + _UP) + 80
    return 2.0 * keys * w * kn


def timed(fn, repeats):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(repeats):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / repeats


def gpu_part(log, repeats, enhance=False):
    sd = random_roll2midi_enhance_state_dict(4321) if enhance else random_roll2midi_state_dict(4321)
    Engine = Roll2MidiEnhanceEngine if enhance else Roll2MidiEngine
    one = synthetic_key_roll(1, WINDOW, KEYS, 1).transpose(1, 2)[:, None].contiguous().cuda()
    clip = synthetic_key_roll(1, WINDOW * CLIP_WINDOWS, KEYS, 2).cuda()
    flop = window_flop(enhance=enhance)
    log(f"device: {torch.cuda.get_device_name(0)}; {flop / 1e9:.1f} GFLOP per {KEYS}x{WINDOW} window (counted), {repeats} repeats per figure")
    for mode in ("bf16", "bf16x3", "fp32"):
        eng = Engine(sd, "cuda:0", compute=mode, chunk=CLIP_WINDOWS)
        for _ in range(2):                                           # warm-up of both shapes
            eng.forward(one)
            eng.refine(clip)
        torch.cuda.synchronize()
        t1 = [timed(lambda: eng.forward(one), repeats) for _ in range(3)]
        t5 = [timed(lambda: eng.refine(clip), repeats) for _ in range(3)]
        w_ms, c_ms = min(t1), min(t5)
        log(f"{mode:7s} window {w_ms:8.3f} ms (3 runs: {', '.join(f'{t:.3f}' for t in t1)})   10 s clip, 5 windows in one pass {c_ms:8.3f} ms "
            f"({', '.join(f'{t:.3f}' for t in t5)})   {flop / w_ms / 1e9:7.1f} / {5 * flop / c_ms / 1e9:7.1f} TFLOP/s of network arithmetic"
            + (f" = {100 * flop / (w_ms * 1e-3) / BF16_MFMA_PEAK:.1f} % / {100 * 5 * flop / (c_ms * 1e-3) / BF16_MFMA_PEAK:.1f} % of the bf16 MFMA rate"
               if mode == "bf16" else ""))
        prof = L.KernelProfiler()
        L.set_profiler(prof)
        eng.refine(clip)
        L.set_profiler(None)
        agg = prof.summary()
        total = sum(a["ms"] for a in agg.values())
        own = ("roll2midi_stem", "leaky_shadow", "roll2midi_head") + (("roll2midi_gate",) if enhance else ())
        log(f"        per-launch events over one clip: {total:.3f} ms in {sum(a['launches'] for a in agg.values())} launches; "
            + ", ".join(f"{k} {agg[k]['ms']:.3f} ms x{agg[k]['launches']} ({agg[k]['bytes'] / agg[k]['ms'] / 1e9:.2f} TB/s)" for k in own if k in agg)
            + f"; the {len(own)} row kernels {100 * sum(agg[k]['ms'] for k in own if k in agg) / total:.1f} % of the launches' time")
        del eng
        torch.cuda.empty_cache()


def gate_part(log, repeats):
    """One gate launch over the u_k map of a 5-window clip against (a) the same work from torch ops on the same buffers -- einsum,
    sigmoid, multiply, the shadow casts -- and (b) v2a_leaky_shadow over the same map: both move fp32 in, fp32 out and the shadow out.
    The map holds positive values and the gate's bias is 40 (alpha rounds to 1), so that repeated in-place launches leave it as it is."""
    n, H, W = CLIP_WINDOWS, KEYS, WINDOW
    log(f"gate launch alone, map (n={n}, {H} x {W}, border 1), best of 3 runs of {repeats} back-to-back launches, all shown:")
    for mode, split, sm in (("bf16x3", True, L.SH_SPLIT), ("bf16", False, L.SH_BF16), ("fp32", False, L.SH_NONE)):
        mem = ConvMemory(torch.device("cuda:0"), split)
        for k, (C, Cg, _) in enumerate(_GATES, 1):
            u = mem.map(f"u{k}", n, H, W, C, 1, sm != L.SH_NONE)
            u.interior().copy_(torch.rand(n, H, W, C, device="cuda"))
            p, d = u.slice(0, C - Cg), u.slice(C - Cg, Cg)
            w = (torch.randn(C, device="cuda") / C ** 0.5).contiguous()
            seg = lambda sl: (sl.base(), sl.pitch, sl.C, sl.shadow(), sl.lo)

            def gate():
                L.roll2midi_gate(seg(p), seg(d), w, bias=40.0, shadow_mode=sm, n=n, H=H, W=W, border=1)

            def leaky():
                L.leaky_shadow(u.base(), u.shadow(), n=n, H=H, W=W, C_=C, shadow_mode=sm, lo_offset=u.lo, pitch=u.pitch, border=1)

            def composed():
                x = u.interior()
                y = x * torch.sigmoid(torch.einsum("nhwc,c->nhw", x, w) + 40.0)[..., None]
                x.copy_(y)
                if sm == L.SH_BF16:
                    u.sh[:, 1:-1, 1:-1].copy_(y)
                elif sm == L.SH_SPLIT:
                    hi = y.to(torch.bfloat16)
                    u.sh[0, :, 1:-1, 1:-1].copy_(hi)
                    u.sh[1, :, 1:-1, 1:-1].copy_(y - hi.float())

            out = {}
            for name, fn in (("gate", gate), ("leaky_shadow", leaky), ("torch", composed)):
                fn()
                torch.cuda.synchronize()
                out[name] = [timed(fn, repeats) for _ in range(3)]
            nbytes = n * H * W * C * (8.0 + 2 * sm)
            g, l, t = (min(out[k]) for k in ("gate", "leaky_shadow", "torch"))
            log(f"  {mode:7s} att{k} C={C:5d}: gate {g * 1e3:7.1f} us ({', '.join(f'{v * 1e3:.1f}' for v in out['gate'])}; {nbytes / g / 1e9:.2f} TB/s)   "
                f"leaky_shadow {l * 1e3:7.1f} us ({', '.join(f'{v * 1e3:.1f}' for v in out['leaky_shadow'])})   gate / leaky_shadow {g / l:.2f}   "
                f"torch composition {t * 1e3:7.1f} us ({', '.join(f'{v * 1e3:.1f}' for v in out['torch'])}) = {t / g:.1f}x the gate")
        del mem
        torch.cuda.empty_cache()


def cpu_part(log, ref_root, enhance=False):
    name = "Roll2MidiNet_enhance" if enhance else "Roll2MidiNet"
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_root, "src", "audeo", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.Generator((1, KEYS, WINDOW))
    net.load_state_dict(random_roll2midi_enhance_state_dict(4321) if enhance else random_roll2midi_state_dict(4321), strict=True)
    net.eval()
    x = synthetic_key_roll(1, WINDOW * CLIP_WINDOWS, KEYS, 2).reshape(CLIP_WINDOWS, WINDOW, KEYS).transpose(1, 2)[:, None].contiguous()
    with torch.no_grad():
        net(x[:1])
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            for i in range(CLIP_WINDOWS):                            # one window per call, as Roll2Midi_inference.py:57-64 runs them
                net(x[i:i + 1])
            ts.append((time.perf_counter() - t) * 1e3)
    log(f"reference module on the CPU (fp32, {torch.get_num_threads()} torch threads): 10 s clip, 5 windows {min(ts):.0f} ms "
        f"({', '.join(f'{t:.0f}' for t in ts)}), {min(ts) / CLIP_WINDOWS:.0f} ms per window")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree: time its module on the CPU instead of the GPU engine")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--enhance", action="store_true", help="the attention-gated generator (Roll2MidiNet_enhance.py) and its gate kernel")
    a = ap.parse_args()

    def log(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.reference:
        cpu_part(log, a.reference, a.enhance)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("roll2midi_probe: no GPU (a timing needs one; --reference DIR times the reference module on the CPU)")
        gpu_part(log, a.repeats, a.enhance)
        if a.enhance:
            gate_part(log, a.repeats)


if __name__ == "__main__":
    main()
