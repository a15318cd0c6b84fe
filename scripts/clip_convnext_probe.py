"""Time v2a_amd.CLIPConvNeXtImageEncoder (convnext_xxlarge shapes, seeded weights) on one GPU and write profiles/clip_convnext_kernels.txt:
  - a clip of `--frames` frames at `--hw` input per compute mode: ms per clip (median of `--iters` encodes after a warm-up) and the
    per-kernel totals of one encode (device events around every launch), with the share of the convolution, its LayerNorm and the pool;
  - the same network from torch operations in fp32 on the same GPU (tests/convnext_ref.py on the device, channels-last input);
  - v2a_convnext_dwconv + v2a_clip_layernorm at the four real stage shapes, chunk `--chunk`: achieved bytes/s against the measured copy
    rate of the same map, and the time of torch's F.conv2d(groups=C) + F.layer_norm on the same tensors in the same process.

    python scripts/clip_convnext_probe.py [--frames 250] [--hw 360x640] [--modes bf16x3,fp32] [--chunk 32] [--iters 3] [--out profiles/clip_convnext_kernels.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _time(fn, iters, warm=1):
    """Median ms of `iters` timed calls after `warm` untimed ones, device events around each."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def stage_shapes(enc, chunk, lines):
    """The convolution and its LayerNorm at each stage's map, against a copy of the map and against torch on the same tensors."""
    import torch.nn.functional as F
    from v2a_amd import _lib as L
    out = []
    for g, C in zip(enc.sizes, enc.dims):
        gen = torch.Generator().manual_seed(C)
        x = torch.randn(chunk, g, g, C, generator=gen).to("cuda:0")
        y, xs = torch.empty_like(x), torch.empty(chunk * g * g, enc.w * C, dtype=enc.adt, device="cuda:0")
        w, b = (torch.randn(C, 1, 7, 7, generator=gen) / 7).to("cuda:0"), torch.randn(C, generator=gen).to("cuda:0")
        blk = dict(dw_w=w.reshape(C, 49).t().contiguous(), dw_b=b)
        ln = (torch.ones(C, device="cuda:0"), torch.zeros(C, device="cuda:0"))
        M = chunk * g * g
        t_dw = _time(lambda: enc.dwconv(x, y, blk, F=chunk, H=g, W=g, C=C), 20, 3)
        t_ln = _time(lambda: enc._ln(y, xs, ln, rows=M, d=C, ldy=enc.w * C), 20, 3)
        t_cp = _time(lambda: y.copy_(x), 20, 3)
        xc = x.permute(0, 3, 1, 2)                     # NCHW view of the NHWC memory: channels-last
        t_tc = _time(lambda: F.conv2d(xc, w, b, padding=3, groups=C), 20, 3)
        yc = F.conv2d(xc, w, b, padding=3, groups=C).permute(0, 2, 3, 1)
        t_tl = _time(lambda: F.layer_norm(yc, (C,), ln[0], ln[1], enc.eps), 20, 3)
        nbytes = 8.0 * x.numel()
        r = dict(shape=[chunk, g, g, C], dwconv_ms=round(t_dw, 4), layernorm_ms=round(t_ln, 4), copy_ms=round(t_cp, 4),
                 dwconv_GBps=round(nbytes / t_dw / 1e6, 1), copy_GBps=round(nbytes / t_cp / 1e6, 1), torch_conv2d_ms=round(t_tc, 4),
                 torch_layer_norm_ms=round(t_tl, 4), ours_over_torch=round((t_dw + t_ln) / (t_tc + t_tl), 3))
        lines.append("stage shape " + json.dumps(r))
        out.append(r)
        del x, y, xs, yc
        torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--hw", default="360x640")
    ap.add_argument("--modes", default="bf16x3,fp32")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--depths", default="3,4,30,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_convnext_kernels.txt"))
    a = ap.parse_args(argv)
    import convnext_ref as R
    from v2a_amd import _lib as L
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    from v2a_amd.synth import CONVNEXT_XXLARGE, random_convnext_state_dict, synthetic_video_frames
    assert torch.cuda.is_available(), "clip_convnext_probe needs a GPU"
    cfg = dict(CONVNEXT_XXLARGE, depths=tuple(int(v) for v in a.depths.split(",")))
    sd = random_convnext_state_dict(cfg, 0)
    H, W = map(int, a.hw.split("x"))
    frames = torch.from_numpy(synthetic_video_frames(a.frames, H, W, 1)).to("cuda:0")
    lines = [f"clip_convnext_probe: {a.frames} frames of {a.hw}, chunk {a.chunk}, depths {cfg['depths']}, widths {cfg['dims']}, seeded weights; "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    shapes_done = False
    for mode in a.modes.split(","):
        enc = CLIPConvNeXtImageEncoder(sd, "cuda:0", compute=mode, chunk=a.chunk)
        ms = _time(lambda: enc(frames), a.iters)
        prof = L.KernelProfiler()
        L.set_profiler(prof)
        enc(frames)
        summ = prof.summary()
        L.set_profiler(None)
        tot = sum(v["ms"] for v in summ.values())
        lines.append(json.dumps(dict(mode=mode, ms_per_clip=round(ms, 2), ms_per_frame=round(ms / a.frames, 3), profiled_kernel_ms=round(tot, 2))))
        for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
            lines.append(f"  {mode} {k}: {v['launches']} launches, {v['ms']:.2f} ms, {100 * v['ms'] / tot:.1f} % of the profiled kernels"
                         + (f", {v['bytes'] / v['ms'] / 1e6:.0f} GB/s" if k.startswith(("convnext", "clip_layernorm")) else ""))
        share = lambda p: 100 * sum(v["ms"] for k, v in summ.items() if k.startswith(p)) / tot
        lines.append(f"  {mode} shares: convnext_dwconv {share('convnext_dwconv'):.1f} %, clip_layernorm {share('clip_layernorm'):.1f} %, "
                     f"convnext_pool_ln {share('convnext_pool_ln'):.2f} %")
        if not shapes_done:
            stage_shapes(enc, a.chunk, lines)
            shapes_done = True
        del enc
        torch.cuda.empty_cache()
    # the same network from torch operations in fp32 on the same GPU, channels-last, the preprocessing left out
    sd32 = R.bare_keys(sd, torch.float32, "cuda:0")
    pv = torch.randn(a.frames, 3, 256, 256, device="cuda:0").contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        t = _time(lambda: [R.forward(sd32, pv[i:i + a.chunk], 1e-5) for i in range(0, a.frames, a.chunk)], a.iters)
    lines.append(json.dumps(dict(torch_fp32_same_gpu_ms_per_clip=round(t, 2), note="convnext_ref on the device, channels-last input, no preprocessing")))
    lines.append("LayerNorm behind the convolution: v2a_clip_layernorm over the convolution's output (the separate form) is what ships; a form fused "
                 "into the convolution kernel was not built, so no fused-versus-separate A/B is recorded here.")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
