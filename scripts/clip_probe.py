"""Time v2a_amd.CLIPImageEncoder (ViT-bigG/14, seeded weights) on one GPU: a clip of `--frames` frames at `--hw` input, for each
compute mode; preprocessing (the two resize kernels) is timed on its own.  Device events around `--iters` whole-clip encodes after a
warm-up; prints ms per clip, ms per frame, the whole-encoder TF/s and the per-class GEMM rates and MFMA-issued fractions (each class
timed alone with the same operands as in the encoder).

    python scripts/clip_probe.py [--frames 250] [--hw 360x640] [--modes bf16x3,fp32] [--chunk 32] [--iters 2] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--hw", default="360x640")
    ap.add_argument("--modes", default="bf16x3,fp32")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    from v2a_amd import _lib as L
    from v2a_amd.clip import CLIPImageEncoder
    from v2a_amd.synth import VIT_BIGG_14, random_clip_vision_state_dict, synthetic_video_frames
    assert torch.cuda.is_available(), "clip_probe needs a GPU"
    cfg = dict(VIT_BIGG_14, num_hidden_layers=a.layers)
    sd = random_clip_vision_state_dict(cfg, 0)
    H, W = map(int, a.hw.split("x"))
    frames = torch.from_numpy(synthetic_video_frames(a.frames, H, W, 1)).to("cuda:0")
    d, dff, T, Lyr = cfg["hidden_size"], cfg["intermediate_size"], 257, cfg["num_hidden_layers"]
    per_frame_flops = 2.0 * T * (Lyr * (4 * d * d + 2 * d * dff) + 640 * d) + Lyr * 4.0 * T * T * d + 2.0 * d * cfg["projection_dim"]
    res = []
    for mode in a.modes.split(","):
        enc = CLIPImageEncoder(sd, "cuda:0", config=cfg, compute=mode, chunk=a.chunk)
        enc(frames[: a.chunk])                                            # warm-up: plans, buffers, code objects
        ms = _time(lambda: enc(frames), a.iters)
        bf = enc._buffers(a.chunk)
        pre = _time(lambda: [enc.preprocess(frames[i:i + a.chunk], bf["patches"]) for i in range(0, a.frames, a.chunk)], a.iters)
        # GEMM classes of one chunk, alone
        M, w, dp = a.chunk * T, (2 if enc.split else 1), enc.dp
        Lw = enc.layers[0]
        cls = {"qkv": (bf["x"], dp, Lw["qkv"], bf["qkv"], 3 * d, dict(bias=Lw["qkv_b"])),
               "out_proj": (bf["ao"], dp, Lw["o"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=bf["h"])),
               "fc1_gelu": (bf["x"], dp, Lw["fc1"], bf["ff"], dff, dict(epilogue=L.EPI_GELU, bias=Lw["fc1_b"], out_split=enc.split, ldo=w * dff)),
               "fc2": (bf["ff"], dff, Lw["fc2"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=bf["h"]))}
        rates = {}
        for name, (A, k, Wt, out, N, kw) in cls.items():
            t = _time(lambda: enc._gemm(A, w * k, k, Wt, out, M=M, N=N, **kw), 10)
            tf = 2.0 * M * N * k / t / 1e9
            # MFMA-issued fraction: bf16x3 issues three bf16 products per fp32 product (dense bf16 peak 2.5 PF), fp32 runs at 157.3 TF
            rates[name] = dict(ms=round(t, 4), TFLOPs=round(tf, 1), mfma_issued=round(3 * tf / 2500 if enc.split else tf / 157.3, 3))
        r = dict(mode=mode, frames=a.frames, hw=a.hw, chunk=a.chunk, layers=Lyr, ms_per_clip=round(ms, 2),
                 ms_per_frame=round(ms / a.frames, 3), preprocess_ms_per_clip=round(pre, 3),
                 encoder_TFLOPs=round(per_frame_flops * a.frames / ms / 1e9, 1), gemm_classes=rates)
        print(json.dumps(r), flush=True)
        res.append(r)
        del enc, bf
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
