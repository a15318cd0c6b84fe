"""Time v2a_amd.PianoFramePreprocessor on one GPU: a clip of `--frames` frames at each `--hw` input size.  Device events around
`--iters` whole-clip calls after a warm-up: the two kernels alone (frames already on the device), the call including the upload of
the uint8 frames from pageable host memory, and the same frames through the Pillow loop of the reference (x3:1883-1890) on this
host's CPU (`--pillow-frames` of them, scaled to the clip).  Prints the bytes the kernel pair has to move (RGB in, uint8 tmp out and
in, fp32 out) over the kernel time.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats` with `--no-pillow`.
--portrait: the 88-key configuration's layout (resize to 100 wide x 900 tall, transposed store, x3_2:65-68), and beside it the
composition the transposed vertical pass replaces: `v2a_piano_resize_v` at Ho = 900, Wo = 100 followed by a torch transpose copy.

    python scripts/piano_frames_probe.py [--frames 300] [--hw 360x640,1080x1920] [--chunk 64] [--iters 20] [--portrait] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

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


def pillow_loop(frames, portrait=False):
    from PIL import Image
    out = []
    for f in frames:
        grey = np.array(Image.fromarray(f).convert("L"))
        if portrait:
            img = Image.fromarray(grey.astype(np.uint8)).resize((100, 900))
            out.append(np.transpose(np.reshape(img, (900, 100, 1)), [2, 1, 0]) / 255.)
            continue
        img = Image.fromarray(grey.astype(np.uint8)).resize((900, 100))
        out.append(np.transpose(np.reshape(img, (100, 900, 1)), [2, 0, 1]) / 255.)
    return np.concatenate(out).astype(np.float32)


def composed_portrait(dev_frames, chunk):
    """What the parent commit can do: the landscape kernels at Ho = 900, Wo = 100, then a transpose copy."""
    from v2a_amd.piano_frames import PianoFramePreprocessor
    pre = PianoFramePreprocessor("cuda:0", 900, 100, chunk=chunk)
    return lambda: pre(dev_frames).transpose(1, 2).contiguous()


def vertical_passes(pre, dev_frames):
    """The vertical pass alone over one tmp of the whole clip: (transposed store, plain store + torch transpose copy) as callables."""
    from v2a_amd import _lib as L
    F, H, W, _ = dev_frames.shape
    p, hb, hk, vb, vk = pre._plan(H, W)
    lib, s = L.lib(), L.stream_ptr()
    ldt = -(-p.Wo // 4) * 4
    tmp = torch.empty(F, p.rows, ldt, dtype=torch.uint8, device=dev_frames.device)
    L.check(lib.v2a_piano_resize_h(dev_frames.data_ptr(), F, H, W, 0, F, tmp.data_ptr(), ldt, p.y0, p.rows, p.Wo, hb.data_ptr(), hk.data_ptr(),
                                   hk.shape[1], s))
    a = torch.empty(F, p.Wo, p.Ho, device=dev_frames.device)
    b = torch.empty(F, p.Ho, p.Wo, device=dev_frames.device)
    args = lambda o: (tmp.data_ptr(), F, p.rows, ldt, p.Ho, p.Wo, vb.data_ptr(), vk.data_ptr(), vk.shape[1], pre._lut.data_ptr(), o.data_ptr(), s)

    def vt():
        L.check(lib.v2a_piano_resize_vt(*args(a)))
        return a

    def v_then_transpose():
        L.check(lib.v2a_piano_resize_v(*args(b)))
        return b.transpose(1, 2).contiguous()

    return vt, v_then_transpose


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--hw", default="360x640,1080x1920")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pillow-frames", type=int, default=60)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--portrait", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    from v2a_amd.piano_frames import PianoFramePlan, PianoFramePreprocessor
    from v2a_amd.synth import synthetic_video_frames
    assert torch.cuda.is_available(), "piano_frames_probe needs a GPU"
    res = []
    for hw in a.hw.split(","):
        H, W = map(int, hw.split("x"))
        base = synthetic_video_frames(min(a.frames, 12), H, W, 1)
        host = torch.from_numpy(np.concatenate([base] * -(-a.frames // len(base)))[: a.frames].copy())
        dev = host.to("cuda:0")
        layout = "portrait" if a.portrait else "landscape"
        pre = PianoFramePreprocessor("cuda:0", chunk=a.chunk, layout=layout)
        plan = PianoFramePlan(H, W, layout=layout)
        out = pre(dev)                                                     # warm-up: tables, code objects
        assert np.array_equal(out[: len(base)].cpu().numpy(), plan.preprocess_numpy(base)), hw
        pre(host)
        kern = _time(lambda: pre(dev), a.iters)
        e2e = _time(lambda: pre(host), max(2, a.iters // 4))
        nbytes = a.frames * (plan.rows * W * 3 + 2 * plan.rows * plan.Wo + 100 * 900 * 4)
        r = dict(hw=hw, layout=layout, frames=a.frames, chunk=a.chunk, ksize=[int(plan.hk.shape[1]), int(plan.vk.shape[1])], rows=plan.rows,
                 kernels_ms_per_clip=round(kern, 4), with_upload_ms_per_clip=round(e2e, 3), MB_moved=round(nbytes / 1e6, 1),
                 TB_per_s=round(nbytes / kern / 1e9, 3), of_measured_copy_6p29=round(nbytes / kern / 1e9 / 6.29, 3))
        if a.portrait:
            comp = composed_portrait(dev, a.chunk)
            assert torch.equal(comp(), out), hw
            ck = _time(comp, a.iters)
            r.update(composed_v_plus_transpose_ms_per_clip=round(ck, 4), composed_over_transposed_store=round(ck / kern, 3))
            vt, vtr = vertical_passes(pre, dev)
            assert torch.equal(vt(), out) and torch.equal(vtr(), out), hw
            tvt, tvtr = _time(vt, a.iters), _time(vtr, a.iters)
            r.update(vertical_transposed_store_ms=round(tvt, 4), vertical_plus_transpose_copy_ms=round(tvtr, 4),
                     vertical_ratio=round(tvtr / tvt, 3))
        if not a.no_pillow:
            n = min(a.pillow_frames, a.frames)
            sub = host[:n].numpy()
            pillow_loop(sub[:2], a.portrait)
            t0 = time.perf_counter()
            ref = pillow_loop(sub, a.portrait)
            dt = time.perf_counter() - t0
            assert np.array_equal(ref, out[:n].cpu().numpy()), hw
            r.update(pillow_ms_per_frame=round(dt / n * 1e3, 3), pillow_ms_per_clip=round(dt / n * a.frames * 1e3, 1),
                     pillow_over_hip_with_upload=round(dt / n * a.frames * 1e3 / e2e, 1))
        print(json.dumps(r), flush=True)
        res.append(r)
        del dev, out
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
