"""Time v2a_amd.CLIPViT2ImageEncoder (ViT-L/14-336, seeded weights) on one GPU: a clip of `--frames` frames at `--hw` input, for each
compute mode; preprocessing (the two resize kernels) is timed on its own.  Device events around `--iters` whole-clip encodes after a
warm-up; prints ms per clip, ms per frame, the whole-encoder TF/s and the per-class GEMM rates and MFMA-issued fractions (each class
timed alone with the same operands as in the encoder), as scripts/clip_probe.py does for ViT-bigG.

Three further measurements:
  fc1, QUICK_GELU against GELU: the same operands, shape, tile and output, the two epilogues alternating, `--ab-repeats` repeats of
      `--ab-launches` launches each, for the full chunk (chunk * 577 rows) and for the clip's last chunk; the median of each, their ratio and
      the run-to-run spread (min .. max over the repeats) of both.
  --torch-ref: the same weights in transformers' CLIPVisionModelWithProjection (fp32, on the same GPU, its default attention), the
      pixel_values given ready-made: the time of the model alone, per clip.
  --encode-only: one clip per mode and nothing else (no warm-up, no stand-alone launches): the run to put under
      `rocprofv3 --kernel-trace --stats` for the per-kernel table of one clip.
  --errors: the worst image_embeds error of each mode over tests/golden/clip_vit2_*.npz (relative to max |ref|).

    python scripts/clip_vit2_probe.py [--frames 250] [--hw 360x640] [--modes bf16x3,fp32] [--chunk 32] [--iters 2] [--torch-ref] [--errors]
                                      [--json out.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np
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


def fc1_ab(enc, bf, rows, repeats, launches):
    """{epilogue: [ms per launch, one per repeat]} of the fc1 GEMM on `rows` rows of the chunk's operands, GELU and QUICK_GELU alternating."""
    from v2a_amd import _lib as L
    w, dp, dff, Lw = enc.w, enc.dp, enc.dff, enc.layers[0]
    run = lambda epi: enc._gemm(bf["x"], w * dp, dp, Lw["fc1"], bf["ff"], M=rows, N=dff, epilogue=epi, bias=Lw["fc1_b"], out_split=enc.split,
                                ldo=w * dff)
    ts = {"gelu": [], "quick_gelu": []}
    for epi in (L.EPI_GELU, L.EPI_QUICK_GELU):
        _time(lambda: run(epi), 3)                                       # code objects
    for _ in range(repeats):
        for name, epi in (("gelu", L.EPI_GELU), ("quick_gelu", L.EPI_QUICK_GELU)):
            ts[name].append(_time(lambda: run(epi), launches))
    return ts


def torch_reference(cfg, sd, frames, S, chunk, iters):
    """ms per clip of transformers' model in fp32 on the GPU, fed ready pixel_values (chunk frames per call)."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    with torch.device("meta"):
        m = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg))
    m.load_state_dict(sd, strict=False, assign=True)
    T = 1 + (S // cfg["patch_size"]) ** 2
    m.vision_model.embeddings.register_buffer("position_ids", torch.arange(T).unsqueeze(0), persistent=False)
    m = m.float().eval().to("cuda:0")
    pv = torch.randn(frames, 3, S, S, device="cuda:0")

    @torch.no_grad()
    def run():
        return [m(pixel_values=pv[i:i + chunk]).image_embeds for i in range(0, frames, chunk)]

    run()
    ms = _time(run, iters)
    return ms, getattr(m.config, "_attn_implementation", None)


def fixture_errors(modes):
    """{mode: (worst relative image_embeds error, its case)} over the committed fixtures."""
    from v2a_amd.clip import CLIPViT2ImageEncoder
    from v2a_amd.synth import random_clip_vision_state_dict, synthetic_video_frames
    worst = {m: (0.0, None) for m in modes}
    for name in ("small", "wide", "full"):
        z = np.load(os.path.join(ROOT, "tests", "golden", f"clip_vit2_{name}.npz"))
        for cname, case in json.loads(str(z["meta"]))["cases"].items():
            sd = random_clip_vision_state_dict(case["config"], case["seed"], case["outlier"])
            for mode in modes:
                enc = CLIPViT2ImageEncoder(sd, "cuda:0", config=case["config"], compute=mode, chunk=2)
                for (clip, n, h, w, seed) in case["clips"]:
                    key = f"{cname}_{clip}"
                    fr = synthetic_video_frames(n, h, w, seed)
                    assert [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr] == list(z[key + "_frames_md5"]), key
                    ref = z[key + "_embeds"]
                    err = float(np.abs(enc(fr).cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
                    if err > worst[mode][0]:
                        worst[mode] = (err, key)
                del enc
                torch.cuda.empty_cache()
    return worst


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--hw", default="360x640")
    ap.add_argument("--modes", default="bf16x3,fp32")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--ab-repeats", type=int, default=7)
    ap.add_argument("--ab-launches", type=int, default=20)
    ap.add_argument("--torch-ref", action="store_true")
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--encode-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    from v2a_amd import _lib as L
    from v2a_amd.clip import CLIPViT2ImageEncoder
    from v2a_amd.synth import VIT_L_14_336, random_clip_vision_state_dict, synthetic_video_frames
    assert torch.cuda.is_available(), "clip_vit2_probe needs a GPU"
    cfg = dict(VIT_L_14_336, num_hidden_layers=a.layers)
    sd = random_clip_vision_state_dict(cfg, 0)
    H, W = map(int, a.hw.split("x"))
    frames = torch.from_numpy(synthetic_video_frames(a.frames, H, W, 1)).to("cuda:0")
    d, dff, Lyr, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["patch_size"]
    T = 1 + (cfg["image_size"] // P) ** 2
    per_frame_flops = 2.0 * T * (Lyr * (4 * d * d + 2 * d * dff) + 640 * d) + Lyr * 4.0 * T * T * d + 2.0 * d * cfg["projection_dim"]
    modes = a.modes.split(",")
    res = []
    for mode in modes:
        enc = CLIPViT2ImageEncoder(sd, "cuda:0", config=cfg, compute=mode, chunk=a.chunk)
        if a.encode_only:
            ms = _time(lambda: enc(frames), 1)
            print(json.dumps(dict(mode=mode, frames=a.frames, hw=a.hw, chunk=a.chunk, layers=Lyr, tokens=T, cold_ms_per_clip=round(ms, 2))), flush=True)
            del enc
            torch.cuda.empty_cache()
            continue
        enc(frames[: a.chunk])                                            # warm-up: plans, buffers, code objects
        if a.frames % a.chunk:
            enc(frames[: a.frames % a.chunk])                             # the last chunk's shapes too
            enc(frames[: a.chunk])                                        # (one live chunk size: back to the full chunk's buffers)
        ms = _time(lambda: enc(frames), a.iters)
        bf = enc._buffers(a.chunk)
        pre = _time(lambda: [enc.preprocess(frames[i:i + a.chunk], bf["patches"]) for i in range(0, a.frames, a.chunk)], a.iters)
        # GEMM classes of one chunk, alone
        M, w, dp = a.chunk * T, (2 if enc.split else 1), enc.dp
        Lw = enc.layers[0]
        cls = {"qkv": (bf["x"], dp, Lw["qkv"], bf["qkv"], 3 * d, dict(bias=Lw["qkv_b"])),
               "out_proj": (bf["ao"], dp, Lw["o"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["o_b"], resid=bf["h"])),
               "fc1_quick_gelu": (bf["x"], dp, Lw["fc1"], bf["ff"], dff, dict(epilogue=L.EPI_QUICK_GELU, bias=Lw["fc1_b"], out_split=enc.split,
                                                                           ldo=w * dff)),
               "fc2": (bf["ff"], dff, Lw["fc2"], bf["h"], d, dict(epilogue=L.EPI_RESID, bias=Lw["fc2_b"], resid=bf["h"]))}
        rates = {}
        for name, (A, k, Wt, out, N, kw) in cls.items():
            t = _time(lambda: enc._gemm(A, w * k, k, Wt, out, M=M, N=N, **kw), 10)
            tf = 2.0 * M * N * k / t / 1e9
            # MFMA-issued fraction: bf16x3 issues three bf16 products per fp32 product (dense bf16 peak 2.5 PF), fp32 runs at 157.3 TF
            rates[name] = dict(ms=round(t, 4), TFLOPs=round(tf, 1), mfma_issued=round(3 * tf / 2500 if enc.split else tf / 157.3, 3))
        attn = _time(lambda: enc.attention(bf["qkv"], bf["ao"], a.chunk), 10)
        ab = {}
        for rows in sorted({a.chunk * T, (a.frames % a.chunk or a.chunk) * T}, reverse=True):
            ts = fc1_ab(enc, bf, rows, a.ab_repeats, a.ab_launches)
            med = {k: statistics.median(v) for k, v in ts.items()}
            ab[str(rows)] = dict(gelu_ms=round(med["gelu"], 4), quick_gelu_ms=round(med["quick_gelu"], 4),
                                 ratio=round(med["quick_gelu"] / med["gelu"], 4),
                                 gelu_spread=[round(min(ts["gelu"]), 4), round(max(ts["gelu"]), 4)],
                                 quick_gelu_spread=[round(min(ts["quick_gelu"]), 4), round(max(ts["quick_gelu"]), 4)])
        r = dict(mode=mode, frames=a.frames, hw=a.hw, chunk=a.chunk, layers=Lyr, tokens=T, ms_per_clip=round(ms, 2),
                 ms_per_frame=round(ms / a.frames, 3), preprocess_ms_per_clip=round(pre, 3),
                 encoder_TFLOPs=round(per_frame_flops * a.frames / ms / 1e9, 1), gemm_classes=rates, attention_ms_per_chunk=round(attn, 4),
                 fc1_quick_gelu_vs_gelu=ab)
        print(json.dumps(r), flush=True)
        res.append(r)
        del enc, bf
        torch.cuda.empty_cache()
    if a.torch_ref:
        ms, impl = torch_reference(cfg, sd, a.frames, cfg["image_size"], a.chunk, a.iters)
        r = dict(torch_reference="transformers CLIPVisionModelWithProjection, fp32, pixel_values ready", attention=impl, frames=a.frames,
                 chunk=a.chunk, ms_per_clip=round(ms, 2), tf32=bool(torch.backends.cuda.matmul.allow_tf32))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.errors:
        r = dict(fixture_errors={m: dict(worst=float(f"{e:.3e}"), case=k) for m, (e, k) in fixture_errors(modes).items()})
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
