"""Time v2a_amd.DINOv2ImageEncoder (dinov2-giant, seeded weights) on one GPU: a clip of `--frames` frames at `--hw` input, for each
compute mode; preprocessing (the two resize kernels) is timed on its own.  Device events around `--iters` whole-clip encodes after a
warm-up; prints ms per clip, ms per frame, the whole-encoder TF/s, the per-class GEMM rates (each class timed alone with the same
operands as in the encoder) with the SWIGLU GEMM beside the STORE and GELU GEMMs of the same M, N, K, and the attention A/B:
v2a_attention (MFMA; V2A_F32 and V2A_BF16_SPLIT with out_split) against v2a_clip_attention (fp32 VALU) at 257 keys, 24 heads of 64,
no gate, no clamp -- time per chunk and error against float64.  `--cpu-frames N` adds transformers' fp32 Dinov2Model on the host CPU.

    python scripts/dinov2_probe.py [--frames 250] [--hw 360x640] [--modes bf16x3,fp32] [--chunk 32] [--iters 2] [--cpu-frames 0] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

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


def attention_ab(enc32, encs, chunk):
    """Time (one chunk) and error against float64 (two frames) of the attention forms on one seeded packed qkv buffer."""
    d, T, H = enc32.d, enc32.T, enc32.H
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(chunk * T, 3 * d, generator=g) * 1.5
    q, k, v = (qkv[:2 * T].double().view(2, T, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(2 * T, d)
    qd = qkv.to("cuda:0")
    out = {}
    for name, enc, form in (("v2a_attention_f32", enc32, "v2a_attention"), ("v2a_clip_attention_f32", enc32, "v2a_clip_attention"),
                            ("v2a_attention_split", encs, "v2a_attention")):
        if enc is None:
            continue
        enc.f32_attention = form
        o = torch.zeros(chunk * T, (2 if enc.split else 1) * d, dtype=torch.bfloat16 if enc.split else torch.float32, device="cuda:0")
        enc.attention(qd, o, chunk)
        t = _time(lambda: enc.attention(qd, o, chunk), 20)
        oc = o[:2 * T].float().cpu().double()
        got = oc[:, :d] + oc[:, d:] if enc.split else oc
        out[name] = dict(ms=round(t, 4), TFLOPs=round(4.0 * chunk * H * T * T * 64 / t / 1e9, 1),
                         rel_err_vs_float64=float((got - ref).abs().max() / ref.abs().max()))
    enc32.f32_attention = "v2a_attention"
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--hw", default="360x640")
    ap.add_argument("--modes", default="bf16x3,fp32")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--cpu-frames", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    from v2a_amd import _lib as L
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    from v2a_amd.synth import DINOV2_GIANT, random_dinov2_state_dict, synthetic_video_frames
    assert torch.cuda.is_available(), "dinov2_probe needs a GPU"
    cfg = dict(DINOV2_GIANT, num_hidden_layers=a.layers)
    sd = random_dinov2_state_dict(cfg, 0)
    H, W = map(int, a.hw.split("x"))
    host_frames = synthetic_video_frames(a.frames, H, W, 1)
    frames = torch.from_numpy(host_frames).to("cuda:0")
    d, T, Lyr = cfg["hidden_size"], 257, cfg["num_hidden_layers"]
    res, encs = [], {}
    for mode in a.modes.split(","):
        enc = DINOv2ImageEncoder(sd, "cuda:0", config=cfg, compute=mode, chunk=a.chunk)
        encs[mode] = enc
        dff = enc.dff
        per_frame_flops = 2.0 * T * (Lyr * (4 * d * d + 3 * d * dff) + 640 * d) + Lyr * 4.0 * T * T * d
        enc(frames[: a.chunk])                                            # warm-up: plans, buffers, code objects
        ms = _time(lambda: enc(frames), a.iters)
        bf = enc._buffers(a.chunk)
        pre = _time(lambda: [enc.preprocess(frames[i:i + a.chunk], bf["patches"]) for i in range(0, a.frames, a.chunk)], a.iters)
        # GEMM classes of one chunk, alone; ff_* are the 2 * dff x d GEMM of the feed-forward under three epilogues
        M, w = a.chunk * T, (2 if enc.split else 1)
        Lw = enc.layers[0]
        adt = torch.bfloat16 if enc.split else torch.float32
        wide = torch.empty(M, w * 2 * dff, dtype=adt, device="cuda:0")     # GELU output of the same N: 2 dff columns (x 2 planes)
        wide32 = torch.empty(M, 2 * dff, device="cuda:0")
        cls = {"qkv": (bf["x"], d, Lw["qkv"], bf["qkv"], 3 * d, dict(bias=Lw["qkv_b"])),
               "dense": (bf["ao"], d, Lw["o"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=bf["h"])),
               "ff_swiglu": (bf["x"], d, Lw["fc1"], bf["ff"], 2 * dff, dict(epilogue=L.EPI_SWIGLU, bias=Lw["fc1_b"], out_split=enc.split, ldo=w * dff)),
               "ff_store": (bf["x"], d, Lw["fc1"], wide32, 2 * dff, dict(bias=Lw["fc1_b"])),
               "ff_gelu": (bf["x"], d, Lw["fc1"], wide, 2 * dff, dict(epilogue=L.EPI_GELU, bias=Lw["fc1_b"], out_split=enc.split, ldo=w * 2 * dff)),
               "weights_out": (bf["ff"], dff, Lw["fc2"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=bf["h"]))}
        rates = {}
        for name, (A, k, Wt, out, N, kw) in cls.items():
            t = _time(lambda: enc._gemm(A, w * k, k, Wt, out, M=M, N=N, **kw), 10)
            tf = 2.0 * M * N * k / t / 1e9
            # MFMA-issued fraction: bf16x3 issues three bf16 products per fp32 product (dense bf16 peak 2.5 PF), fp32 runs at 157.3 TF
            rates[name] = dict(ms=round(t, 4), TFLOPs=round(tf, 1), mfma_issued=round(3 * tf / 2500 if enc.split else tf / 157.3, 3))
        r = dict(mode=mode, frames=a.frames, hw=a.hw, chunk=a.chunk, layers=Lyr, ms_per_clip=round(ms, 2),
                 ms_per_frame=round(ms / a.frames, 3), preprocess_ms_per_clip=round(pre, 3),
                 encoder_TFLOPs=round(per_frame_flops * a.frames / ms / 1e9, 1), gemm_classes=rates,
                 swiglu_over_store=round(rates["ff_swiglu"]["ms"] / rates["ff_store"]["ms"], 3),
                 swiglu_over_gelu=round(rates["ff_swiglu"]["ms"] / rates["ff_gelu"]["ms"], 3))
        print(json.dumps(r), flush=True)
        res.append(r)
        del bf, wide, wide32
    if "fp32" in encs:
        ab = dict(attention_ab=attention_ab(encs["fp32"], encs.get("bf16x3"), a.chunk))
        print(json.dumps(ab), flush=True)
        res.append(ab)
    encs.clear()
    torch.cuda.empty_cache()
    if a.cpu_frames > 0:
        from transformers import BitImageProcessor, Dinov2Config, Dinov2Model
        m = Dinov2Model(Dinov2Config(**cfg, attn_implementation="eager"))
        m.load_state_dict(sd)
        m.eval()
        proc = BitImageProcessor(size={"shortest_edge": 256}, crop_size={"height": 224, "width": 224}, resample=3)
        fr = list(host_frames[: a.cpu_frames])
        with torch.no_grad():
            m(**proc(images=fr[:1], return_tensors="pt"))
            t0 = time.perf_counter()
            m(**proc(images=fr, return_tensors="pt"))
            dt = time.perf_counter() - t0
        cpu = dict(cpu_baseline=dict(frames=a.cpu_frames, threads=torch.get_num_threads(), ms_per_frame=round(1e3 * dt / a.cpu_frames, 1),
                                     ms_per_clip_extrapolated=round(1e3 * dt / a.cpu_frames * a.frames, 0)))
        print(json.dumps(cpu), flush=True)
        res.append(cpu)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
