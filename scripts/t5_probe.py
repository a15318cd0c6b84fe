"""Time v2a_amd.T5Encoder.encode_ids (flan-t5-large shape, seeded weights) for a list of (B, N) shapes on one GPU: warm-up,
then device events around `--iters` encodes; prints ms per encode and the effective fp32 weight-stream rate.

    python scripts/t5_probe.py [--shapes 1x32,8x64,1x512] [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x32,8x64,1x512")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    from v2a_amd.synth import FLAN_T5_LARGE, random_t5_encoder_state_dict
    from v2a_amd.t5 import T5Encoder
    assert torch.cuda.is_available(), "t5_probe needs a GPU"
    enc = T5Encoder(random_t5_encoder_state_dict(FLAN_T5_LARGE, 0), "cuda:0")
    wbytes = 4.0 * sum(int(v.numel()) for Lw in enc.layers for v in Lw.values())
    res = []
    for s in a.shapes.split(","):
        B, N = map(int, s.split("x"))
        ids = torch.randint(2, FLAN_T5_LARGE["vocab_size"], (B, N), generator=torch.Generator().manual_seed(B * 1000 + N))
        mask = torch.ones(B, N, dtype=torch.int32)
        for _ in range(a.warmup):
            enc.encode_ids(ids, mask)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            enc.encode_ids(ids, mask)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        M = B * N
        flops = 2.0 * M * wbytes / 4
        r = dict(B=B, N=N, ms_per_encode=round(ms, 4), weight_stream_GBps=round(wbytes / ms / 1e6, 1),
                 gemm_TFLOPs=round(flops / ms / 1e9, 2), weight_bytes=wbytes)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
