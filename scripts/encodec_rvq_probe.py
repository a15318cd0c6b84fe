"""Time v2a_amd.EncodecQuantizer on one GPU: `encode` and `decode` at 8 and 32 stages on 1 x 750 and 8 x 750 frames, next to the same
search composed stage by stage from generic pieces (exact-fp32 `v2a_gemm` scores, then torch arg-max, gather and subtract) in the
same run, and to the library's quantizer on this host's CPU.

Device events around `--iters` calls form one window; the engines alternate window by window for `--rounds` rounds after a
warm-up, and the table gives the median and the min - max spread over the rounds.

    python scripts/encodec_rvq_probe.py [--iters 20] [--rounds 7] [--out profiles/encodec_rvq.txt] [--no-cpu]
"""
import argparse
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


class Composed:
    """The same search from generic pieces, one stage at a time: scores = r E^T - |e|^2 / 2 by one exact-fp32 v2a_gemm (the bias
    carries the norm term), then torch arg-max, gather and subtract -- four launches per stage where the fused kernel has none."""

    def __init__(self, q):
        from v2a_amd import _lib
        self.L, self.q = _lib, q
        self.bias = (-0.5 * q.norms).contiguous()

    def encode(self, x, n_q):
        B, D, T = x.shape
        r = x.permute(0, 2, 1).reshape(B * T, D).contiguous()
        scores = torch.empty(B * T, self.q.codebook_size, device=x.device, dtype=torch.float32)
        out = []
        for s in range(n_q):
            e = self.q.codebooks[s]
            self.L.gemm([(r, D, D)], e, scores, M=B * T, N=self.q.codebook_size, compute=self.L.F32, bias=self.bias[s], ldo=self.q.codebook_size)
            ind = scores.argmax(1)
            r = r - e[ind]
            out.append(ind)
        return torch.stack(out).view(n_q, B, T)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from v2a_amd.encodec import EncodecQuantizer
    from v2a_amd.synth import random_encodec_quantizer_state_dict, synthetic_encodec_latents
    assert torch.cuda.is_available(), "encodec_rvq_probe needs a GPU"
    sd = random_encodec_quantizer_state_dict(0)
    q = EncodecQuantizer(sd, "cuda:0")
    comp = Composed(q)
    lines = [f"{a.rounds} rounds of {a.iters} calls per engine, alternating, device events, profiler off; structured seeded latents",
             "%-46s %10s %10s %10s" % ("per call", "median ms", "min ms", "max ms")]
    for B in (1, 8):
        x = synthetic_encodec_latents(q.codebooks.cpu(), B, 750, 7).to("cuda:0")
        for n_q, bw in ((8, 6.0), (32, 24.0)):
            codes = q.encode(x, bw)
            same = float((comp.encode(x, n_q) == codes).all(0).float().mean())
            runs = {f"{B} x 750, {n_q:2d} stages: encode (fused)": lambda: q.encode(x, bw),
                    f"{B} x 750, {n_q:2d} stages: encode (composed)": lambda: comp.encode(x, n_q),
                    f"{B} x 750, {n_q:2d} stages: decode": lambda: q.decode(codes)}
            for fn in runs.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    ms[k].append(window_ms(fn, a.iters))
            for k, v in ms.items():
                lines.append("%-46s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
            lines.append(f"    frames with the same codes, fused and composed: {100 * same:.2f} %")
            if not a.no_cpu:
                from transformers import EncodecConfig
                from transformers.models.encodec.modeling_encodec import EncodecResidualVectorQuantizer
                ref = EncodecResidualVectorQuantizer(EncodecConfig(target_bandwidths=[1.5, 3.0, 6.0, 12.0, 24.0])).eval()
                ref.load_state_dict(sd, strict=True)
                xc, ts = x.cpu(), []
                with torch.no_grad():
                    ref.encode(xc, bw)
                    for _ in range(3):
                        t0 = time.perf_counter()
                        cc = ref.encode(xc, bw)
                        ts.append((time.perf_counter() - t0) * 1e3)
                lines.append("%-46s %10.1f %10.1f %10.1f   (transformers fp32, %d threads; frames with the same codes as fused: %.2f %%)"
                             % (f"{B} x 750, {n_q:2d} stages: CPU library encode", statistics.median(ts), min(ts), max(ts), torch.get_num_threads(),
                                100 * float((cc == codes.cpu()).all(0).float().mean())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
