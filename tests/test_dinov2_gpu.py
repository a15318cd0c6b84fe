"""GPU: the HIP DINOv2 image encoder (dinov2.py, the SWIGLU epilogue of v2a_gemm, v2a_attention without gate and clamp) against
transformers' float64 BitImageProcessor + Dinov2Model (tests/golden/dinov2_*.npz, scripts/make_golden_dinov2.py), its kernels
against torch float64, chunk invariance, and E2TTS(video_encoder="dinov2").sample(video_frames=...)."""
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
BARS = {"fp32": 2e-5, "bf16x3": 2e-4}


def _fx(name):
    z = np.load(os.path.join(GOLDEN, f"dinov2_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _frames(clip, key, z):
    from v2a_amd.synth import synthetic_video_frames
    _, n, h, w, seed = clip
    fr = synthetic_video_frames(n, h, w, seed)
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr]
    assert md5 == list(z[key + "_frames_md5"]), f"{key}: the seeded frames differ from the ones the fixture was made from"
    return fr


def _weights(case):
    from v2a_amd.synth import random_dinov2_state_dict
    return random_dinov2_state_dict(case["config"], case["seed"], case["outlier"])


def _encoder(case, compute, sd=None, **kw):
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    return DINOv2ImageEncoder(_weights(case) if sd is None else sd, DEV, config=case["config"], compute=compute, resize=case["resize"],
                              crop=case["crop"], **kw)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- preprocessing -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "wide"])
def test_preprocessing_bit_equal_to_processor(name):
    z, meta = _fx(name)
    for cname, case in meta["cases"].items():
        for mode in ("fp32", "bf16x3"):
            enc = _encoder(dict(case, config=dict(case["config"], num_hidden_layers=1)), mode)
            S, P, T, kp = enc.S, enc.P, enc.T, enc.kp
            assert (S, enc.resize) == (case["crop"], case["resize"])
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


# ---- the SWIGLU epilogue against a float64 product ------------------------------------------------------
# every kernel v2a_gemm can pick for SWIGLU: the exact-fp32 kernel (64x64 / 128x128 tiles by shape) and the split-operand shapes 1..7
SMALL_MNK, BIG_MNK = (257 * 2, 1024, 192), (257 * 4, 8192, 1536)
SWIGLU_CASES = [("fp32", 0) + SMALL_MNK, ("fp32", 0) + BIG_MNK] + [("split", h) + BIG_MNK for h in range(1, 8)] + [("split", 0) + SMALL_MNK]


@functools.lru_cache(maxsize=None)
def _swiglu_problem(M, N, K):
    """Operands and the float64 reference of one shape, made once for all the cases that use it."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.3 * torch.randn(N, generator=g)
    acc = (a.double() @ w.double().t() + b.double()).view(M, N // 32, 2, 16)        # [16 value | 16 gate] per 16 outputs
    ref = acc[:, :, 0].reshape(M, N // 2) * torch.nn.functional.silu(acc[:, :, 1].reshape(M, N // 2))
    return a, w, b, ref


@pytest.mark.parametrize("mode,hint,M,N,K", SWIGLU_CASES)
def test_swiglu_epilogue_against_float64(mode, hint, M, N, K):
    from v2a_amd import _lib as L
    a, w, b, ref = _swiglu_problem(M, N, K)
    No = N // 2
    outs = {}
    if mode == "fp32":
        out = torch.empty(M, No, device=DEV)
        L.gemm([(a.to(DEV), K, K)], w.to(DEV), out, M=M, N=N, compute=L.F32, epilogue=L.EPI_SWIGLU, bias=b.to(DEV))
        outs["fp32"] = out
    else:
        As, Ws = L.split_planes(a).to(DEV), L.split_planes(w).to(DEV)
        o32 = torch.empty(M, No, device=DEV)
        L.gemm([(As, 2 * K, K)], Ws, o32, M=M, N=N, compute=L.BF16, epilogue=L.EPI_SWIGLU, bias=b.to(DEV), a_split=True, tile_hint=hint)
        osp = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)                      # row = [hi of the N/2 | lo of them]
        L.gemm([(As, 2 * K, K)], Ws, osp, M=M, N=N, compute=L.BF16, epilogue=L.EPI_SWIGLU, bias=b.to(DEV), a_split=True, tile_hint=hint,
               out_split=True, ldo=N)
        outs["f32out"], outs["splitout"] = o32, osp
    torch.cuda.synchronize()
    errs = {}
    for k, o in outs.items():
        o = o.float().cpu().double()
        got = o[:, :No] + o[:, No:] if k == "splitout" else o
        errs[k] = float((got - ref).abs().max() / ref.abs().max())
        print(f"swiglu {mode} hint {hint} {M}x{N}x{K} {k}: {errs[k]:.2e}")
    for k, err in errs.items():
        assert err <= (2e-6 if mode == "fp32" else 2e-5), (k, err)


def test_swiglu_epilogue_refused_where_not_built():
    from v2a_amd import _lib as L
    a = torch.randn(256, 640, device=DEV).bfloat16()
    w = torch.randn(512, 640, device=DEV).bfloat16()
    with pytest.raises(L.V2AError, match="SWIGLU"):        # plain bf16 compute
        L.gemm([(a, 640, 640)], w, torch.empty(256, 256, dtype=torch.bfloat16, device=DEV), M=256, N=512, compute=L.BF16, epilogue=L.EPI_SWIGLU)
    with pytest.raises(L.V2AError, match="SWIGLU"):
        L.gemm([(a, 640, 640)], w, torch.empty(256, 256, device=DEV), M=256, N=512, compute=L.BF16, epilogue=L.EPI_SWIGLU)
    with pytest.raises(L.V2AError):                        # plane output needs split operands
        L.gemm([(a.float(), 640, 640)], w.float(), torch.empty(256, 512, dtype=torch.bfloat16, device=DEV), M=256, N=512,
               compute=L.F32, epilogue=L.EPI_SWIGLU, out_split=True, ldo=512)
    with pytest.raises(L.V2AError, match="32"):            # value / gate groups of 16
        L.gemm([(a.float(), 640, 640)], w.float()[:496], torch.empty(256, 248, device=DEV), M=256, N=496, compute=L.F32, epilogue=L.EPI_SWIGLU)


# ---- v2a_attention without gate and clamp on the packed qkv buffer ------------------------------------------
@pytest.mark.parametrize("N", [257, 17, 64])
def test_attention_no_gate_no_clamp_against_float64(N):
    from v2a_amd import _lib as L
    g = torch.Generator().manual_seed(N)
    B, H, D = 3, 24, 64
    d = H * D
    qkv = torch.randn(B * N, 3 * d, generator=g) * 1.5
    q, k, v = (qkv.double().view(B, N, 3, H, D)[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1)
    ref = (p @ v).transpose(1, 2).reshape(B * N, d)
    qd = qkv.to(DEV)
    errs = {}
    for split in (0, 1):
        out = torch.zeros(B * N, 2 * d, dtype=torch.bfloat16, device=DEV) if split else torch.empty(B * N, d, device=DEV)
        ors = out.stride(0)
        L.attention(qd.data_ptr(), qd.data_ptr() + 4 * d, qd.data_ptr() + 8 * d, None, out.data_ptr(),
                    strides=(3 * d, 3 * d, 3 * d, 0, ors, N * 3 * d, N * 3 * d, N * 3 * d, 0, N * ors), B=B, H=H, Nq=N, Nk=N,
                    scale=D ** -0.5, softclamp=0.0, dtype=L.BF16_SPLIT if split else L.F32, out_split=bool(split))
        torch.cuda.synchronize()
        o = out.float().cpu().double()
        got = o[:, :d] + o[:, d:] if split else o
        errs[split] = float((got - ref).abs().max() / ref.abs().max())
        print(f"v2a_attention gate=None softclamp=0 N={N} {'split, out_split' if split else 'f32'} (relative to max |o|): {errs[split]:.2e}")
    assert errs[0] <= 2e-5 and errs[1] <= 2e-4, errs


# ---- the whole encoder against transformers float64 ----------------------------------------------------
def _check_model(name, modes=("fp32", "bf16x3")):
    z, meta = _fx(name)
    worst = {}
    for cname, case in meta["cases"].items():
        sd = _weights(case)
        for mode in modes:
            enc = _encoder(case, mode, sd, chunk=2)
            for clip in case["clips"]:
                key = f"{cname}_{clip[0]}"
                fr = torch.from_numpy(_frames(clip, key, z)).to(DEV)
                taps = {l: None for l in case["taps"]}
                got = enc.encode_chunk(fr, taps=taps).cpu().numpy().astype(np.float64)
                ref = z[key + "_embeds"]
                err = _rel(got, ref)
                tap_err = {l: _rel(taps[l][:, z[key + f"_tap{l}_rows"]].cpu().numpy(), z[key + f"_tap{l}"]) for l in case["taps"]}
                print(f"{key} [{mode}]: pooler_output {err:.2e} (bar {BARS[mode]:.0e}); taps " +
                      ", ".join(f"L{l} {e:.2e}" for l, e in tap_err.items()))
                worst[(key, mode)] = err
                # the chunked call equals the per-chunk pass
                assert np.array_equal(enc(fr).cpu().numpy(), got.astype(np.float32))
            del enc
            torch.cuda.empty_cache()
    bad = {k: v for k, v in worst.items() if v > BARS[k[1]]}
    assert not bad, bad


def test_encoder_small_swiglu_and_gelu():
    _check_model("small")


def test_encoder_wide_and_outlier():
    _check_model("wide")


def test_encoder_full_depth():
    _check_model("full")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_chunk_invariance(mode):
    from v2a_amd.synth import DINOV2_GIANT, synthetic_video_frames
    case = dict(config=dict(DINOV2_GIANT, num_hidden_layers=2), seed=3, outlier=0.0, resize=256, crop=224)
    fr = torch.from_numpy(synthetic_video_frames(5, 200, 300, 9))
    outs, sd = [], _weights(case)
    for chunk in (5, 2, 1):
        enc = _encoder(case, mode, sd, chunk=chunk)
        outs.append(enc(fr).cpu())
        del enc
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- E2TTS wiring -----------------------------------------------------------------------------------------
def test_sample_with_video_frames(tmp_path):
    from oracle import e2_cfm_oracle as O
    from v2a_amd.features import feature_cache_path, load_clip_cache, resample_clip_features
    z, meta = _fx("small")
    case = meta["cases"]["small"]
    cfg = O.DiTConfig(dim=128, dim_text=case["config"]["hidden_size"], dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                      num_channels=16, max_seq_len=256)
    P = O.init_params(cfg, 1234)
    y0, _, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=99, piano=True)
    m = make_model(cfg, P, "fp32", device=DEV, video_encoder="dinov2")
    enc = m.load_image_encoder(_encoder(case, "fp32"))
    clips = case["clips"][:2]
    frames = [(_frames(c, f"small_{c[0]}", z), 0.5 + 0.25 * i) for i, c in enumerate(clips)]
    kw = dict(y0=y0, context=ctx, context_mask=cm, frames_embed=roll, steps=4, cfg_strength=2.0, remove_parallel_component=False,
              return_raw_output=True)
    cond = torch.zeros(2, 40, 16)
    got = m.sample(cond, video_frames=frames, **kw)
    te = torch.stack([resample_clip_features(enc(f).cpu(), d, 40) for f, d in frames])
    ref = m.sample(cond, text_embed=te, **kw)
    assert torch.equal(got, ref)
    # the same DiT fed the float64 features of the fixture
    te64 = torch.stack([resample_clip_features(torch.from_numpy(z[f"small_{c[0]}_embeds"]).float(), d, 40) for c, (_, d) in zip(clips, frames)])
    d64 = float((m.sample(cond, text_embed=te64, **kw) - got).abs().max())
    print(f"DiT output, HIP DINOv2 features vs float64 ones: {d64:.2e}")
    assert d64 <= 1e-3
    # video_paths without caches: encoded in one pass, caches written as .generated.dinov2.npz, read back on the second call
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    first = m.sample(cond, video_paths=paths, video_frames=frames, **kw)
    caches = [str(tmp_path / f"clip{i}.generated.dinov2.npz") for i in range(2)]
    assert caches == [feature_cache_path(p, "dinov2") for p in paths] and all(os.path.exists(c) for c in caches)
    assert not any(os.path.exists(feature_cache_path(p)) for p in paths)
    for c, (f, d) in zip(caches, frames):
        emb, dur = load_clip_cache(c)
        assert dur == d and torch.equal(emb.float(), enc(f).cpu())
    assert torch.equal(first, got)
    second = m.sample(cond, video_paths=paths, **kw)
    assert torch.equal(second, first)
