"""GPU: the HIP CLIP ConvNeXt image encoder (convnext.py, csrc/convnext.hip) against transformers' float64 `ConvNextModel`
(tests/golden/clip_convnext_*.npz, scripts/make_golden_clip_convnext.py: eps 1e-6) and, at the real model's eps 1e-5, against the
float64 restatement tests/convnext_ref.py (pinned to the fixtures by tests/test_clip_convnext_refs.py); its kernels against torch
float64; chunk invariance; E2TTS(video_encoder="clip_convnext" / "mixed").sample(video_frames=...) and the caches."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
BARS = {"fp32": 2e-5, "bf16x3": 2e-4}


def _fx(name, family="clip_convnext"):
    z = np.load(os.path.join(GOLDEN, f"{family}_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _frames(clip, key, z):
    from v2a_amd.synth import synthetic_video_frames
    _, n, h, w, seed = clip
    fr = synthetic_video_frames(n, h, w, seed)
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr]
    assert md5 == list(z[key + "_frames_md5"]), f"{key}: the seeded frames differ from the ones the fixture was made from"
    return fr


def _weights(case):
    from v2a_amd.synth import random_convnext_state_dict
    return random_convnext_state_dict(case["config"], case["seed"], case["outlier"])


def _encoder(case, compute, sd=None, eps=None, **kw):
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    return CLIPConvNeXtImageEncoder(_weights(case) if sd is None else sd, DEV, config=dict(layer_norm_eps=case["eps"] if eps is None else eps),
                                    compute=compute, resize=case["resize"], crop=case["crop"], **kw)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- v2a_convnext_dwconv -----------------------------------------------------------------------------
DW_SHAPES = [(2, 2, 2, 64), (1, 4, 4, 256), (3, 8, 8, 3072), (1, 64, 64, 384), (2, 5, 9, 96)]
U = 2.0 ** -24
GAMMA_50 = 50 * U / (1 - 50 * U)           # the a-priori bound of a 50-term fp32 sum (49 products and the bias), Higham's gamma_n


def _dwconv(x, w, b):
    """x (F, H, W, C), w (C, 1, 7, 7), b (C,) on the CPU -> the kernel's output on the CPU."""
    from v2a_amd import _lib as L
    F, H, W, C = x.shape
    xd, out = x.to(DEV).contiguous(), torch.full((F, H, W, C), float("nan"), device=DEV)
    wt, bd = w.reshape(C, 49).t().contiguous().to(DEV), b.to(DEV)
    L.check(L.lib().v2a_convnext_dwconv(xd.data_ptr(), out.data_ptr(), wt.data_ptr(), bd.data_ptr(), F, H, W, C, L.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv_within_the_a_priori_bound_of_float64(shape):
    F, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(F, H, W, C, generator=g) * 2 + 0.3
    w, b = torch.randn(C, 1, 7, 7, generator=g) / 7, torch.randn(C, generator=g) * 0.5
    conv = lambda xx, ww, bb: torch.nn.functional.conv2d(xx.permute(0, 3, 1, 2), ww, bb, padding=3, groups=C).permute(0, 2, 3, 1)
    ref = conv(x.double(), w.double(), b.double())
    mag = conv(x.double().abs(), w.double().abs(), b.double().abs())          # sum |w x| + |b| per output
    got = _dwconv(x, w, b)
    assert bool(torch.isfinite(got).all()), "an output was not written"
    ratio = float(((got.double() - ref).abs() / (GAMMA_50 * mag)).max())
    print(f"dwconv {shape}: max |error| / (gamma_50 (sum |w x| + |b|)) = {ratio:.3f}")
    assert ratio <= 1.0
    # a frame's bits do not depend on the batch nor on its position in it
    if F == 3:
        for f in range(3):
            assert torch.equal(_dwconv(x[f:f + 1], w, b)[0], got[f])


# ---- LayerNorm at the block's widths, and the pooled LayerNorm -----------------------------------------------
@pytest.mark.parametrize("rows,d", [(3 * 64, 3072), (70, 384)])
def test_layernorm_in_both_layouts_against_float64(rows, d):
    """v2a_clip_layernorm as the blocks use it: rows = pixels, d = the stage's width up to 3072, into fp32 rows and into hi | lo planes."""
    from v2a_amd import _lib as L
    g = torch.Generator().manual_seed(d)
    x = torch.randn(rows, d, generator=g) * 3 + 0.5
    x[:, [5, 200, 333]] *= 60
    gam, bet = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    y = torch.empty(rows, d, device=DEV)
    ys = torch.zeros(rows, 2 * d, dtype=torch.bfloat16, device=DEV)
    lib = L.lib()
    L.check(lib.v2a_clip_layernorm(xd.data_ptr(), d, y.data_ptr(), d, L.F32, rows, d, gd.data_ptr(), bd.data_ptr(), 1e-5, L.stream_ptr()))
    L.check(lib.v2a_clip_layernorm(xd.data_ptr(), d, ys.data_ptr(), 2 * d, L.BF16_SPLIT, rows, d, gd.data_ptr(), bd.data_ptr(), 1e-5, L.stream_ptr()))
    torch.cuda.synchronize()
    ysc = ys.float().cpu().double()
    e = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    es = float((ysc[:, :d] + ysc[:, d:] - ref).abs().max() / ref.abs().max())
    print(f"layernorm rows {rows} d {d} (relative to max |y|): fp32 {e:.2e}, split planes {es:.2e}")
    assert e <= 1e-6 and es <= 1e-5


@pytest.mark.parametrize("F,pixels,C", [(3, 64, 3072), (2, 4, 512), (1, 35, 96)])
def test_pool_ln_against_float64(F, pixels, C):
    from v2a_amd import _lib as L
    g = torch.Generator().manual_seed(C + pixels)
    x = torch.randn(F, pixels, C, generator=g) * 3 + 0.5
    x[..., [5, 40, 77]] *= 60
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = torch.nn.functional.layer_norm(x.double().mean(1), (C,), gam.double(), bet.double(), 1e-5)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    out = torch.full((F, C + 8), float("nan"), device=DEV)
    L.check(L.lib().v2a_convnext_pool_ln(xd.data_ptr(), pixels * C, F, pixels, C, gd.data_ptr(), bd.data_ptr(), 1e-5, out.data_ptr(), C + 8, L.stream_ptr()))
    one = torch.empty(1, C, device=DEV)
    L.check(L.lib().v2a_convnext_pool_ln(xd[F - 1].data_ptr(), pixels * C, 1, pixels, C, gd.data_ptr(), bd.data_ptr(), 1e-5, one.data_ptr(), C, L.stream_ptr()))
    torch.cuda.synchronize()
    o = out.cpu()
    e = float((o[:, :C].double() - ref).abs().max() / ref.abs().max())
    print(f"pool_ln F {F} pixels {pixels} C {C} (relative to max |y|): {e:.2e}")
    assert e <= 1e-6 and bool(torch.isnan(o[:, C:]).all()) and torch.equal(one.cpu()[0], o[F - 1, :C])


# ---- preprocessing -----------------------------------------------------------------------------------
def test_preprocessing_bit_equal_to_pillow_and_torch():
    z, meta = _fx("small")
    for cname, case in meta["cases"].items():
        for mode in ("fp32", "bf16x3"):
            enc = _encoder(case, mode)
            S, P, T, kp = enc.S, enc.P, enc.T, enc.kp
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
                idx = z[key + "_pix_idx"]                       # flat (3, S, S) index -> patch matrix (row, column)
                ch, y, x = idx // (S * S), (idx // S) % S, idx % S
                row = 1 + (y // P) * (S // P) + x // P
                col = ch * P * P + (y % P) * P + x % P
                pm = patches.cpu().view(n, T, w * kp)
                ref = torch.from_numpy(z[key + "_pix"])
                if enc.split:          # the planes of the fp32 value: hi = bf16(v), lo = bf16(v - hi)
                    hi = ref.bfloat16()
                    assert torch.equal(pm[:, row, col], hi) and torch.equal(pm[:, row, kp + col], (ref - hi.float()).bfloat16()), key
                else:
                    assert torch.equal(pm[:, row, col], ref), key
                assert float(pm[:, 0].abs().max()) == 0.0 and float(pm[:, :, 3 * P * P:kp].abs().max()) == 0.0


# ---- the whole encoder -----------------------------------------------------------------------------------
def _tap_keys(case):
    """Fixture tap name -> encode_chunk's tap key."""
    d = case["config"]["depths"]
    keys = {"stem": "stem", "s2b0": (2, 0), "s2bL": (2, d[2] - 1)}
    keys.update({f"s{s}": (s, n - 1) for s, n in enumerate(d)})
    return keys


@functools.lru_cache(maxsize=None)
def _ref_eps5(name, cname, clip):
    """convnext_ref in float64 on the CPU at eps 1e-5 (the real model's), once per clip: (embeds, taps)."""
    import convnext_ref as R
    z, meta = _fx(name)
    case = meta["cases"][cname]
    sd = R.bare_keys(_weights(case))
    c = next(c for c in case["clips"] if c[0] == clip)
    _, pv = R.preprocess(_frames(c, f"{cname}_{clip}", z), case["resize"], case["crop"])
    taps = {k: None for k in _tap_keys(case).values()}
    with torch.no_grad():
        emb = R.forward(sd, pv.double(), 1e-5, taps)
    return emb.numpy(), {k: v.numpy() for k, v in taps.items()}


def _check_model(name):
    z, meta = _fx(name)
    worst = {}
    for cname, case in meta["cases"].items():
        sd = _weights(case)
        keys = _tap_keys(case)
        for mode in ("fp32", "bf16x3"):
            enc = _encoder(case, mode, sd, chunk=2)
            for eps in (1e-6, 1e-5):
                enc.eps = eps              # a launch argument of the LayerNorm kernels, nothing prepared depends on it
                for clip in case["clips"]:
                    key = f"{cname}_{clip[0]}"
                    fr = torch.from_numpy(_frames(clip, key, z)).to(DEV)
                    n = fr.shape[0]
                    taps = {k: None for k in keys.values()}
                    got = enc.encode_chunk(fr, taps=taps).cpu().numpy().astype(np.float64)
                    if eps == 1e-6:        # transformers' float64 ConvNextModel
                        ref = z[key + "_embeds"]
                        tap_ref = lambda t: z[key + f"_tap_{t}"]
                    else:                  # the float64 restatement at the real model's eps
                        ref, maps = _ref_eps5(name, cname, clip[0])
                        tap_ref = lambda t: maps[keys[t]].reshape(n, -1, maps[keys[t]].shape[-1])[:, z[key + f"_tap_{t}_rows"]]
                    err = _rel(got, ref)
                    tap_err = {t: _rel(taps[keys[t]].reshape(n, -1, taps[keys[t]].shape[-1])[:, z[key + f"_tap_{t}_rows"]].cpu().numpy(), tap_ref(t))
                               for t in case["taps"]}
                    print(f"{key} [{mode}, eps {eps:.0e}]: embeds {err:.2e} (bar {BARS[mode]:.0e}); taps " +
                          ", ".join(f"{t} {e:.2e}" for t, e in tap_err.items()))
                    worst[(key, mode, eps)] = err
                    assert np.array_equal(enc(fr).cpu().numpy(), got.astype(np.float32))      # the chunked call equals the per-chunk pass
            del enc
            torch.cuda.empty_cache()
    bad = {k: v for k, v in worst.items() if v > BARS[k[1]]}
    assert not bad, bad


def test_encoder_small():
    _check_model("small")


def test_encoder_wide_and_outlier():
    _check_model("wide")


def test_encoder_full_depth():
    _check_model("full")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_chunk_invariance(mode):
    from v2a_amd.synth import synthetic_video_frames
    case = dict(config=dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=128), seed=3, outlier=0.0, resize=96, crop=96, eps=1e-5)
    fr = torch.from_numpy(synthetic_video_frames(5, 120, 170, 9))
    outs, sd = [], _weights(case)
    for chunk in (5, 2, 1):
        enc = _encoder(case, mode, sd, chunk=chunk)
        outs.append(enc(fr).cpu())
        del enc
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- E2TTS wiring -----------------------------------------------------------------------------------------
def _dit(dim_text, video_encoder):
    from oracle import e2_cfm_oracle as O
    cfg = O.DiTConfig(dim=128, dim_text=dim_text, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=16,
                      max_seq_len=256)
    P = O.init_params(cfg, 1234)
    y0, _, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=99, piano=True)
    m = make_model(cfg, P, "fp32", device=DEV, video_encoder=video_encoder)
    kw = dict(y0=y0, context=ctx, context_mask=cm, frames_embed=roll, steps=4, cfg_strength=2.0, remove_parallel_component=False,
              return_raw_output=True)
    return m, kw


def test_sample_with_video_frames(tmp_path):
    from v2a_amd.features import feature_cache_path, load_clip_cache, resample_clip_features
    z, meta = _fx("small")
    case = meta["cases"]["small"]
    m, kw = _dit(case["config"]["embed_dim"], "clip_convnext")
    enc = m.load_image_encoder(_encoder(case, "fp32"))
    clips = case["clips"][:2]
    frames = [(_frames(c, f"small_{c[0]}", z), 0.5 + 0.25 * i) for i, c in enumerate(clips)]
    cond = torch.zeros(2, 40, 16)
    got = m.sample(cond, video_frames=frames, **kw)
    te = torch.stack([resample_clip_features(enc(f).cpu(), d, 40) for f, d in frames])
    assert torch.equal(got, m.sample(cond, text_embed=te, **kw))
    # video_paths without caches: encoded, caches written as .generated.clip_convnext.npz, read back on the second call
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    first = m.sample(cond, video_paths=paths, video_frames=frames, **kw)
    caches = [str(tmp_path / f"clip{i}.generated.clip_convnext.npz") for i in range(2)]
    assert caches == [feature_cache_path(p, "clip_convnext") for p in paths] and all(os.path.exists(c) for c in caches)
    assert not any(os.path.exists(feature_cache_path(p)) for p in paths)
    for c, (f, d) in zip(caches, frames):
        emb, dur = load_clip_cache(c)
        assert dur == d and torch.equal(emb.float(), enc(f).cpu())
    assert torch.equal(first, got)
    assert torch.equal(m.sample(cond, video_paths=paths, **kw), first)


def test_mixed_with_four_small_encoders(tmp_path):
    from v2a_amd.clip import CLIPImageEncoder, CLIPViT2ImageEncoder
    from v2a_amd.convnext import MIXED_ORDER, MixedImageEncoder
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    from v2a_amd.features import feature_cache_path, load_clip_cache, resample_clip_features
    from v2a_amd.synth import random_clip_vision_state_dict, random_dinov2_state_dict, synthetic_video_frames
    cv, c2, dn, cx = (_fx("small", fam)[1]["cases"]["small"] for fam in ("clip", "clip_vit2", "dinov2", "clip_convnext"))
    encs = dict(
        clip_vit=CLIPImageEncoder(random_clip_vision_state_dict(cv["config"], cv["seed"]), DEV, config=cv["config"], compute="fp32"),
        clip_vit2=CLIPViT2ImageEncoder(random_clip_vision_state_dict(c2["config"], c2["seed"]), DEV, config=c2["config"], compute="fp32"),
        clip_convnext=_encoder(cx, "fp32"),
        dinov2=DINOv2ImageEncoder(random_dinov2_state_dict(dn["config"], dn["seed"]), DEV, config=dn["config"], compute="fp32", resize=dn["resize"],
                                  crop=dn["crop"]))
    widths = [encs[k].out_dim for k in MIXED_ORDER]
    assert widths == [128, 64, 128, 192]
    m, kw = _dit(sum(widths), "mixed")
    mixed = m.load_image_encoder(encs)
    assert isinstance(mixed, MixedImageEncoder) and mixed.out_dim == 512
    frames = [(synthetic_video_frames(3, 90, 120, 40 + i), 0.5 + 0.25 * i) for i in range(2)]
    rows = [torch.cat([encs[k](f).cpu() for k in MIXED_ORDER], 1) for f, _ in frames]
    assert all(torch.equal(mixed(f).cpu(), r) for (f, _), r in zip(frames, rows))
    cond = torch.zeros(2, 40, 16)
    got = m.sample(cond, video_frames=frames, **kw)
    te = torch.stack([resample_clip_features(r, d, 40) for r, (_, d) in zip(rows, frames)])
    assert torch.equal(got, m.sample(cond, text_embed=te, **kw))
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    first = m.sample(cond, video_paths=paths, video_frames=frames, **kw)
    assert torch.equal(first, got)
    for p, r, (f, d) in zip(paths, rows, frames):
        emb, dur = load_clip_cache(feature_cache_path(p, "mixed"))
        assert feature_cache_path(p, "mixed").endswith(".generated.mixed.npz") and dur == d and torch.equal(emb, r)
        o = 0
        for k, wd in zip(MIXED_ORDER, widths):                  # the four part caches, under their own choices' names
            part, pdur = load_clip_cache(feature_cache_path(p, k))
            assert pdur == d and torch.equal(part, r[:, o:o + wd]), k
            o += wd
    assert torch.equal(m.sample(cond, video_paths=paths, **kw), first)
