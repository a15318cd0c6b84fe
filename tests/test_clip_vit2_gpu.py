"""GPU: the HIP CLIP ViT-L/14-336 image encoder (clip.py CLIPViT2ImageEncoder, the QUICK_GELU epilogue of v2a_gemm, the engine's MFMA
attention for 64-wide heads) against transformers' float64 CLIPImageProcessor + CLIPVisionModelWithProjection
(tests/golden/clip_vit2_*.npz, scripts/make_golden_clip_vit2.py), the epilogue against torch float64, chunk invariance at 577 tokens,
and E2TTS(video_encoder="clip_vit2").sample(video_frames=...)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
BARS = {"fp32": 2e-5, "bf16x3": 2e-4}          # of max |ref|: the bars CLIP bigG and DINOv2 are held to
EPI_BARS = {"fp32": 2e-6, "split": 2e-5}       # of max |ref|: the GELU epilogue's own (test_clip_gpu.test_gelu_epilogue_against_float64)


def _fx(name):
    z = np.load(os.path.join(GOLDEN, f"clip_vit2_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _frames(clip, key, z):
    from v2a_amd.synth import synthetic_video_frames
    _, n, h, w, seed = clip
    fr = synthetic_video_frames(n, h, w, seed)
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr]
    assert md5 == list(z[key + "_frames_md5"]), f"{key}: the seeded frames differ from the ones the fixture was made from"
    return fr


def _weights(case):
    from v2a_amd.synth import random_clip_vision_state_dict
    return random_clip_vision_state_dict(case["config"], case["seed"], case["outlier"])


def _encoder(case, compute, sd=None, **kw):
    from v2a_amd.clip import CLIPViT2ImageEncoder
    return CLIPViT2ImageEncoder(_weights(case) if sd is None else sd, DEV, config=case["config"], compute=compute, **kw)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def quick_gelu64(v):
    """transformers' QuickGELUActivation in float64 (tests/test_clip_vit2_refs.py ties the formula to the library's module)."""
    return v * torch.sigmoid(1.702 * v)


# ---- the QUICK_GELU epilogue against torch float64 ------------------------------------------------------------
# (M, N, K): the exact-fp32 kernel takes its 64x64 tile at the first and its 128x128 tile at the second; both M leave a tail in every tile
# height (514 = 2 * 256 + 2, 1154 = 4 * 256 + 130 = 18 * 64 + 2)
SHAPES = {"narrow": (514, 1024, 640), "fc1": (577 * 2, 4096, 1024)}
# every kernel v2a_gemm can pick for the epilogue: the exact-fp32 kernel (both tiles) and the split-operand shapes 1..7, 0 = by shape
EPI_CASES = [("fp32", 0, "narrow"), ("fp32", 0, "fc1")] + [("split", h, "fc1") for h in range(1, 8)] + [("split", 0, "narrow")]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """(a, w, b, float64 reference) of one shape: made once, shared by every case of the shape and never written."""
    M, N, K = SHAPES[shape]
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.3 * torch.randn(N, generator=g)
    return a, w, b, quick_gelu64(a.double() @ w.double().t() + b.double())


def _run_epilogue(mode, hint, a, w, b):
    """{name: float64 (M, N) result} of the launches of one case: fp32 compute, or split operands with fp32 and with plane output."""
    from v2a_amd import _lib as L
    (M, K), N = a.shape, w.shape[0]
    outs = {}
    if mode == "fp32":
        out = torch.empty(M, N, device=DEV)
        L.gemm([(a.to(DEV), K, K)], w.to(DEV), out, M=M, N=N, compute=L.F32, epilogue=L.EPI_QUICK_GELU, bias=b.to(DEV))
        outs["fp32"] = out
    else:
        As, Ws = L.split_planes(a).to(DEV), L.split_planes(w).to(DEV)
        o32 = torch.empty(M, N, device=DEV)
        L.gemm([(As, 2 * K, K)], Ws, o32, M=M, N=N, compute=L.BF16, epilogue=L.EPI_QUICK_GELU, bias=b.to(DEV), a_split=True, tile_hint=hint)
        osp = torch.empty(M, 2 * N, dtype=torch.bfloat16, device=DEV)
        L.gemm([(As, 2 * K, K)], Ws, osp, M=M, N=N, compute=L.BF16, epilogue=L.EPI_QUICK_GELU, bias=b.to(DEV), a_split=True, tile_hint=hint,
               out_split=True, ldo=2 * N)
        outs["f32out"], outs["splitout"] = o32, osp
    torch.cuda.synchronize()
    res = {}
    for k, o in outs.items():
        o = o.float().cpu().double()
        res[k] = o[:, :N] + o[:, N:] if k == "splitout" else o
    return res


@pytest.mark.parametrize("mode,hint,shape", EPI_CASES)
def test_quick_gelu_epilogue_against_float64(mode, hint, shape):
    a, w, b, ref = _problem(shape)
    for k, got in _run_epilogue(mode, hint, a, w, b).items():
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"quick_gelu {mode} hint {hint} {tuple(a.shape)} x {w.shape[0]} {k}: {err:.2e} (bar {EPI_BARS[mode]:.0e})")
        assert err <= EPI_BARS[mode], (k, err)


@pytest.mark.parametrize("mode,hint", [("fp32", 0), ("split", 0), ("split", 5)])
def test_quick_gelu_epilogue_at_large_arguments(mode, hint):
    """|v| of ~2e2 and ~1e4 in sixteen columns: their weight rows are scaled by 10 and their bias entries set to +-200 and +-1e4, so v is the bias
    +- ~40 and keeps its sign.  Every output is finite.  Where v << 0 (v <= -100 here) the bound |v| exp(-1.702 |v|) is below 1e-70, under
    fp32's smallest subnormal: with one fp32 ulp of the bound as slack, the output is +-0 or that subnormal.  Where v >> 0 the output lies
    within the epilogue's relative bar of v itself (sigmoid(1.702 v) = 1 to 1e-148; v = bias + a sum whose own error is 1e-4 at most
    against |v| >= 100, so the bar is spent on the epilogue, the fp32 rounding of v and the planes).  The other columns keep the bar of the
    ordinary case, relative to their own max |ref|."""
    a, w, b, _ = _problem("narrow")
    N = w.shape[0]
    w, b = w.clone(), b.clone()
    cols = torch.tensor([3, 64, 129, 255, 256, 511, 777, 1023, 5, 66, 131, 250, 260, 515, 781, 1020])      # several tiles, tile edges
    big = torch.tensor([200.0, 1e4, 200.0, 1e4, 200.0, 1e4, 200.0, 1e4] + [-200.0, -1e4, -200.0, -1e4, -200.0, -1e4, -200.0, -1e4])
    w[cols] *= 10.0
    b[cols] = big
    v = a.double() @ w.double().t() + b.double()
    pos, neg = cols[:8], cols[8:]
    assert float(v[:, neg].max()) <= -100 and float(v[:, pos].min()) >= 100 and float(v.abs().max()) > 9e3
    ref = quick_gelu64(v)
    rest = torch.ones(N, dtype=torch.bool)
    rest[cols] = False
    for k, got in _run_epilogue(mode, hint, a, w, b).items():
        assert bool(torch.isfinite(got).all()), k
        bound = (v[:, neg].abs() * torch.exp(-1.702 * v[:, neg].abs())).numpy()
        slack = np.spacing(bound.astype(np.float32)).astype(np.float64)
        over = float((got[:, neg].abs().numpy() - bound - slack).max())
        relv = float(((got[:, pos] - v[:, pos]).abs() / v[:, pos].abs()).max())
        err = float((got[:, rest] - ref[:, rest]).abs().max() / ref[:, rest].abs().max())
        print(f"quick_gelu large |v| {mode} hint {hint} {k}: max |out| at v << 0 {float(got[:, neg].abs().max()):.2e}, |out - v| / |v| at v >> 0 "
              f"{relv:.2e}, other columns {err:.2e} (bar {EPI_BARS[mode]:.0e})")
        assert over <= 0.0, (k, over)
        assert relv <= EPI_BARS[mode], (k, relv)
        assert err <= EPI_BARS[mode], (k, err)


def test_quick_gelu_epilogue_refused_where_not_built():
    from v2a_amd import _lib as L
    a = torch.randn(256, 640, device=DEV).bfloat16()
    w = torch.randn(512, 640, device=DEV).bfloat16()
    with pytest.raises(L.V2AError, match="QUICK_GELU"):
        L.gemm([(a, 640, 640)], w, torch.empty(256, 512, device=DEV), M=256, N=512, compute=L.BF16, epilogue=L.EPI_QUICK_GELU)
    with pytest.raises(L.V2AError):
        L.gemm([(a.float(), 640, 640)], w.float(), torch.empty(256, 1024, dtype=torch.bfloat16, device=DEV), M=256, N=512,
               compute=L.F32, epilogue=L.EPI_QUICK_GELU, out_split=True, ldo=1024)


# ---- preprocessing -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "wide"])
def test_preprocessing_bit_equal_to_processor(name):
    """S = 56 and S = 336: the crop (md5 and sampled bytes) and the pixel_values planes of the patch matrix, in both modes."""
    z, meta = _fx(name)
    for cname, case in meta["cases"].items():
        for mode in ("fp32", "bf16x3"):
            enc = _encoder(dict(case, config=dict(case["config"], num_hidden_layers=1)), mode)
            S, P, T, kp = enc.S, enc.P, enc.T, enc.kp
            assert S == case["config"]["image_size"] and enc.resize == S
            for clip in case["clips"]:
                key = f"{cname}_{clip[0]}"
                fr = torch.from_numpy(_frames(clip, key, z)).to(DEV)
                n = fr.shape[0]
                crop = torch.empty(n, S, S, 3, dtype=torch.uint8, device=DEV)
                w = 2 if enc.split else 1
                patches = torch.zeros(n * T, w * kp, dtype=torch.bfloat16 if enc.split else torch.float32, device=DEV)
                enc.preprocess(fr, patches, crop)
                torch.cuda.synchronize()
                c = crop.cpu().numpy()
                assert [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in c] == list(z[key + "_crop_md5"]), key
                assert np.array_equal(c.reshape(n, -1)[:, z[key + "_crop_idx"]], z[key + "_crop_vals"]), key
                # pixel_values (F, 3, S, S) flat index -> patch matrix (row, column)
                idx = z[key + "_pix_idx"]
                ch, y, x = idx // (S * S), (idx // S) % S, idx % S
                row = 1 + (y // P) * (S // P) + x // P
                col = ch * P * P + (y % P) * P + x % P
                pm = patches.cpu().view(n, T, w * kp)
                ref = z[key + "_pix"]
                if enc.split:          # the planes of the processor's fp32 value: hi = bf16(v), lo = bf16(v - hi)
                    hi = torch.from_numpy(ref).bfloat16()
                    assert torch.equal(pm[:, row, col], hi) and torch.equal(pm[:, row, kp + col], (torch.from_numpy(ref) - hi.float()).bfloat16())
                else:
                    got = pm[:, row, col].numpy()
                    assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all(), (key, float(np.abs(got - ref).max()))
                assert float(pm[:, 0].abs().max()) == 0.0 and float(pm[:, :, 3 * P * P:kp].abs().max()) == 0.0
            del enc


# ---- the whole encoder against transformers float64 ----------------------------------------------------
def _check_model(name, modes=("fp32", "bf16x3")):
    z, meta = _fx(name)
    worst = {}
    for cname, case in meta["cases"].items():
        sd = _weights(case)
        for mode in modes:
            enc = _encoder(case, mode, sd, chunk=2)
            assert enc.ffn[0] == 9 and enc.mfma_attention == (enc.dh == 64)
            for clip in case["clips"]:
                key = f"{cname}_{clip[0]}"
                fr = torch.from_numpy(_frames(clip, key, z)).to(DEV)
                taps = {l: None for l in case["taps"]}
                got = enc.encode_chunk(fr, taps=taps).cpu().numpy().astype(np.float64)
                ref = z[key + "_embeds"]
                err = _rel(got, ref)
                tap_err = {l: _rel(taps[l][:, z[key + f"_tap{l}_rows"]].cpu().numpy(), z[key + f"_tap{l}"]) for l in case["taps"]}
                print(f"{key} [{mode}]: image_embeds {err:.2e} (bar {BARS[mode]:.0e}); taps " +
                      ", ".join(f"L{l} {e:.2e}" for l, e in tap_err.items()))
                worst[(key, mode)] = err
                # the chunked call equals the per-chunk pass
                assert np.array_equal(enc(fr).cpu().numpy(), got.astype(np.float32))
            del enc
            torch.cuda.empty_cache()
    bad = {k: v for k, v in worst.items() if v > BARS[k[1]]}
    assert not bad, bad


def test_encoder_small():
    """64-wide heads (the MFMA attention) and, `small104`, 104-wide heads (the VALU attention) with the new epilogue."""
    _check_model("small")


def test_encoder_wide_and_outlier():
    _check_model("wide")


def test_encoder_full_depth():
    _check_model("full")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_chunk_invariance(mode):
    """577 tokens: a frame's attention launch has 160 workgroups, under the count below which v2a_attention splits the keys (another sum
    order), so a chunk of one depends on the engine's floor on the frames of a launch."""
    from v2a_amd.synth import VIT_L_14_336, synthetic_video_frames
    case = dict(config=dict(VIT_L_14_336, num_hidden_layers=2), seed=3, outlier=0.0)
    fr = torch.from_numpy(synthetic_video_frames(5, 200, 300, 9))
    outs, sd = [], _weights(case)
    for chunk in (5, 2, 1):
        enc = _encoder(case, mode, sd, chunk=chunk)
        assert enc.T == 577 and enc.mfma_attention
        outs.append(enc(fr).cpu())
        del enc
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- E2TTS wiring -----------------------------------------------------------------------------------------
def test_sample_with_video_frames(tmp_path):
    from oracle import e2_cfm_oracle as O
    from v2a_amd.clip import CLIPViT2ImageEncoder
    from v2a_amd.features import feature_cache_path, resample_clip_features
    z, meta = _fx("small")
    case = meta["cases"]["small"]
    assert case["config"]["projection_dim"] == 64
    cfg = O.DiTConfig(dim=128, dim_text=64, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=16, max_seq_len=256)
    P = O.init_params(cfg, 1234)
    y0, _, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=99, piano=True)
    m = make_model(cfg, P, "fp32", device=DEV, video_encoder="clip_vit2")
    enc = m.load_image_encoder(_encoder(case, "fp32"))
    assert isinstance(enc, CLIPViT2ImageEncoder) and m.load_image_encoder(enc) is enc
    clips = case["clips"][:2]
    frames = [(_frames(c, f"small_{c[0]}", z), 0.5 + 0.25 * i) for i, c in enumerate(clips)]
    kw = dict(y0=y0, context=ctx, context_mask=cm, frames_embed=roll, steps=4, cfg_strength=2.0, remove_parallel_component=False,
              return_raw_output=True)
    cond = torch.zeros(2, 40, 16)
    got = m.sample(cond, video_frames=frames, **kw)
    te = torch.stack([resample_clip_features(enc(f).cpu(), d, 40) for f, d in frames])
    ref = m.sample(cond, text_embed=te, **kw)
    assert torch.equal(got, ref)
    # the same DiT fed the float64 embeddings of the fixture
    te64 = torch.stack([resample_clip_features(torch.from_numpy(z[f"small_{c[0]}_embeds"]).float(), d, 40) for c, (_, d) in zip(clips, frames)])
    d64 = float((m.sample(cond, text_embed=te64, **kw) - got).abs().max())
    print(f"DiT output, HIP CLIP ViT2 features vs float64 ones: {d64:.2e}")
    assert d64 <= 1e-3
    # video_paths without caches: encoded in one pass, caches written under the encoder's own name, read back on the second call
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    first = m.sample(cond, video_paths=paths, video_frames=frames, **kw)
    assert [feature_cache_path(p, "clip_vit2") for p in paths] == [str(tmp_path / f"clip{i}.generated.clip_vit2.npz") for i in range(2)]
    assert all(os.path.exists(feature_cache_path(p, "clip_vit2")) for p in paths) and not os.path.exists(feature_cache_path(paths[0]))
    assert torch.equal(first, got)
    second = m.sample(cond, video_paths=paths, **kw)
    assert torch.equal(second, first)
    # an existing cache wins over frames
    third = m.sample(cond, video_paths=paths, video_frames=[(f[:1] * 0, d) for f, d in frames], **kw)
    assert torch.equal(third, first)
    # an encoder whose projection_dim is not dim_text is refused
    wrong = meta["cases"]["small104"]
    with pytest.raises(ValueError, match="dim_text"):
        m.load_image_encoder(_encoder(wrong, "fp32"))
