"""The validation pass `E2TTS.forward(val=True)` on one GPU.

1. Precision of one `transformer_with_pred_head` evaluation in fp32 and bf16x3 mode against the float64 oracle on the inputs of
   tests/test_validation_gpu.py (b = 3, n = 40, lens 40 / 33 / 21, times 0.1 / 0.37 / 0.8; `plain` and `cond`): the bf16x3 figure,
   doubled, is that test's bound on |pred - pred64|.  The method predates forward() and forward() does not change it.
2. Time of one forward(val=True) at the full configuration (8 clips of 750 frames, 16 context tokens, bf16x3) next to one
   `transformer_with_pred_head` on the same inputs, and the three kernels of csrc/cfm_loss.hip on their own.

Device events around `--iters` calls form one window; the candidates alternate window by window for `--rounds` rounds after a
warm-up, and the table gives the median and the min - max spread over the rounds.

    python scripts/validation_probe.py [--iters 5] [--rounds 7] [--out profiles/validation_forward.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
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


def precision_lines():
    import test_validation_gpu as T
    import v2a_amd
    from oracle import e2_cfm_oracle as O
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "forward_small.npz"), allow_pickle=False))
    meta = json.loads(str(g["meta"]))
    small = dict(cfg=O.DiTConfig(**meta["cfg"]), meta=meta)
    cases = T.build_cases(small)
    lines = ["max |pred - pred64| of one transformer_with_pred_head evaluation (b = 3, n = 40, lens 40 / 33 / 21, times 0.1 / 0.37 / 0.8,",
             "frames for the last two clips), and of the pred_flow that forward(val=True) returns from the same x0, x1:"]
    for case, c in cases.items():
        for mode in ("fp32", "bf16x3"):
            m = T._model(c, mode)
            roll = torch.cat([torch.zeros(T.B - T.BF, T.N, v2a_amd.NOTES), m.encode_frames(c["frames"], T.N).cpu()])
            ref = T._reference64(c, roll)
            t = c["times"][:, None, None]
            w = (1. - t) * c["x0"] + t * c["x1"]
            cond = torch.where(c["span"][..., None], torch.zeros_like(c["x1"]), c["x1"]) if c["cfg"].cond_proj_in else None
            pred = m.transformer_with_pred_head(w, cond, times=c["times"], mask=c["mask"], text=c["text"], frames_embed=roll, context=c["ctx"],
                                                context_mask=c["cm"], drop_audio_cond=False, drop_text_cond=False, drop_text_prompt=False)
            r = m.forward(c["x1"], text=c["text"], times=c["times"], lens=c["lens"], val=True, frames=c["frames"], midis=c["midis"], x0=c["x0"],
                          context=c["ctx"], context_mask=c["cm"])
            lines.append("  %-6s %-5s transformer_with_pred_head %.3e   forward %.3e   flow loss %.9f (float64 %.9f)   roll loss %.9f"
                         % (mode, case, float((pred.double() - ref["pred"]).abs().max()), float((r.pred_flow.double() - ref["pred"]).abs().max()),
                            m.val_stats["flow"], ref["loss"], m.val_stats["roll"]))
    return lines


def timing_lines(a):
    import v2a_amd
    from v2a_amd import _lib as L
    from v2a_amd.synth import random_state_dict, synthetic_conditioning
    tk = dict(depth=12, dim=1024, dim_text=1280, heads=16, dim_head=64)
    m = v2a_amd.E2TTS(transformer=dict(if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True, **tk), num_channels=128,
                      if_cond_proj_in=False, audiocond_drop_prob=1.1, compute_dtype="bf16x3", device="cuda:0")
    m.load_state_dict(random_state_dict(m.cfg, 0), strict=False)
    b, n = 8, 750
    x0, text, roll, ctx, cm = synthetic_conditioning(m.cfg, b, n, nc=16, seed=1, piano=True)
    dev = torch.device("cuda:0")
    x1 = torch.randn(b, n, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    x0, text, roll, ctx = x0.to(dev), text.to(dev), roll.to(dev), ctx.to(dev)
    midis = (roll > 0).float()
    times, lens = torch.full((b,), 0.5), torch.full((b,), n)
    mask = v2a_amd.lens_to_mask(lens, n)
    span = v2a_amd.val_span_mask(lens, n).to(dev, torch.uint8)
    w, flow = torch.empty_like(x1), torch.empty_like(x1)
    out2, out6 = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.float64, device=dev)
    kw = dict(text=text, times=times, lens=lens, val=True, x0=x0, context=ctx, context_mask=cm)
    runs = {"transformer_with_pred_head": lambda: m.transformer_with_pred_head(x0, None, times=times, mask=mask, text=text, frames_embed=roll, context=ctx,
                                                                               context_mask=cm, drop_text_cond=False, drop_text_prompt=False),
            "forward(val=True), no frames": lambda: m.forward(x1, **kw),
            "forward(val=True), frames_embed + midis": lambda: m.forward(x1, frames_embed=roll, midis=midis, **kw),
            "v2a_cfm_interp": lambda: L.cfm_interp(x0, x1, times.to(dev), None, w, flow, None),
            "v2a_masked_sqerr": lambda: L.masked_sqerr(w, flow, span, out2),
            "v2a_roll_metrics": lambda: L.roll_metrics(roll, midis, span, out6)}
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            ms[k].append(window_ms(fn, a.iters))
    lines = [f"full configuration (depth 12, dim 1024), {b} x {n} frames, 16 context tokens, bf16x3, eager launches; {a.rounds} rounds of {a.iters} calls,",
             "alternating, device events (host work between launches included)",
             "%-46s %10s %10s %10s" % ("per call", "median ms", "min ms", "max ms")]
    for k, v in ms.items():
        lines.append("%-46s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "validation_probe needs a GPU"
    text = "\n".join(precision_lines() + [""] + timing_lines(a))
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
