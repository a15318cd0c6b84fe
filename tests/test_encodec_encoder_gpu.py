"""GPU parity of the Encodec encoder (`EncodecWrapper.forward`, x3:428-432) through the C ABI.

End to end against float64 vectors of the third-party library the reference calls (tests/golden/encodec_enc_*.npz, made by
scripts/make_golden_encodec_encoder.py): max |delta| < 1e-4 on O(1) latents, the bar the decoder is held to
(tests/test_encodec_gpu.py); the library's own fp32 run sits 6e-6 - 8e-6 from its float64 run.  Per kernel against plain torch
ops: 1e-6 for the pad / ELU kernel, 2e-5 abs / rel for the fused stage-0 kernel (the decoder's per-kernel bar)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PARAM_SEED = 9753                       # of the fixtures (scripts/make_golden_encodec_encoder.py)
TAPS = ("layer1", "layer3", "layer6", "layer9", "layer12", "layer13")


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def params():
    from v2a_amd.synth import random_encodec_encoder_state_dict
    return random_encodec_encoder_state_dict(PARAM_SEED)


@pytest.fixture(scope="module")
def enc(params):
    from v2a_amd.encodec import EncodecEncoder
    return EncodecEncoder(params, DEV)


@pytest.fixture(scope="module")
def enc_composed(params):
    from v2a_amd.encodec import EncodecEncoder
    return EncodecEncoder(params, DEV, fused_stem=False)


def wave(n, seed):
    from v2a_amd.synth import synthetic_wave
    return synthetic_wave(n, seed)


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("pads", [(2, 1), (4, 3), (5, 4), (8, 7), (6, 0), (0, 0)])
@pytest.mark.parametrize("act", [True, False])
def test_elu_pad_lr_matches_torch(L, pads, act):
    pl, pr = pads
    T, C = 37, 48
    x = torch.randn(T, C, generator=_g(pl))
    xa = F.elu(x) if act else x
    ref = F.pad(xa.t()[None], (pl, pr), mode="reflect")[0].t().contiguous()
    out = torch.full((T + pl + pr + 1, C), 9.0, device=DEV)
    L.elu_pad_lr(x.to(DEV), out, T=T, C_=C, pad_left=pl, pad_right=pr, act=act)
    torch.testing.assert_close(out[:-1].cpu(), ref, atol=1e-6, rtol=1e-6)
    assert torch.all(out[-1] == 9.0)                               # nothing written past the padded signal
    with pytest.raises(L.V2AError, match="v2a_elu_pad_lr"):
        L.elu_pad_lr(x.to(DEV), out, T=T, C_=C, pad_left=T, pad_right=0)


def _stage0_reference(enc, w):
    """Layers 0 and 1 in plain torch fp32 ops on the CPU, from the engine's resolved weights: (n, 32)."""
    st = enc.stages[0]
    n = w.shape[0]
    x0 = F.conv1d(F.pad(w.view(1, 1, n), (6, 0), mode="reflect"), enc.stem["w3"], enc.stem["b_cpu"])
    h = F.conv1d(F.pad(F.elu(x0), (2, 0), mode="reflect"), st["b1"]["w3"], st["b1"]["b_cpu"])
    h = F.conv1d(F.elu(h), st["b3"]["w3"], st["b3"]["b_cpu"])
    return (F.conv1d(x0, st["sc"]["w3"], st["sc"]["b_cpu"]) + h)[0].t().contiguous()


@pytest.mark.parametrize("n", [4001, 256, 8])
def test_stage0_kernel_matches_torch_and_the_composed_path(L, enc, enc_composed, n):
    """The fused stem + C = 32 block: against torch fp32 ops, and against the same engine's generic composition
    (zero-padded K = 16 stem GEMM, v2a_elu_pad_lr, three more GEMMs).  n = 4001 leaves a partial last workgroup."""
    w = wave(n, 7)
    ref = _stage0_reference(enc, w)
    out = torch.full((n + 1, 32), 9.0, device=DEV)
    L.encodec_stage0(w.to(DEV), enc.stage0, out, n=n)
    err = float((out[:n].cpu() - ref).abs().max())
    print(f"\nstage-0 kernel (n={n}) vs torch fp32: max |d| = {err:.3e}, max |ref| = {float(ref.abs().max()):.3f}")
    torch.testing.assert_close(out[:n].cpu(), ref, atol=2e-5, rtol=2e-5)
    assert torch.all(out[n] == 9.0)                                # nothing written past row n - 1
    if n >= 8 + 2:
        composed = enc_composed._stage0(w.to(DEV), n).cpu()
        print(f"stage-0 kernel vs composed path: max |d| = {float((out[:n].cpu() - composed).abs().max()):.3e}")
        torch.testing.assert_close(out[:n].cpu(), composed, atol=2e-5, rtol=2e-5)
        torch.testing.assert_close(composed, ref, atol=2e-5, rtol=2e-5)


def _check_fixture(engine, name, label):
    g = np.load(os.path.join(GOLD, f"encodec_enc_{name}.npz"))
    meta = json.loads(str(g["meta"]))
    n = meta["n"]
    taps = {}
    z = engine.encoder(wave(n, meta["input_seed"]).view(1, 1, n), taps)
    assert z.is_cuda and z.dtype == torch.float32 and tuple(z.shape) == (1,) + tuple(g["shape"]) == (1, 128, meta["frames"])
    z = z[0].cpu().numpy().astype(np.float64)
    errs = {}
    for k in TAPS:
        a = taps[k].cpu().numpy().astype(np.float64)
        assert tuple(g[f"{k}_shape"]) == a.shape, k
        errs[k] = float(np.abs(a[tuple(g[f"{k}_idx"].T)] - g[f"{k}_val"]).max())
    errs["latent"] = float(np.abs(z - g["z"]).max()) if "z" in g else float(np.abs(z[tuple(g["z_idx"].T)] - g["z_val"]).max())
    print(f"\nencodec encoder [{label}] n={n} -> {meta['frames']} frames (right pads {meta['right_pads']}) vs float64 library vectors: "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-4, (k, v)
    if "z" not in g:
        assert np.abs(z).mean() == pytest.approx(g["stats"][1], rel=1e-4)
    return errs


@pytest.mark.parametrize("name", ["small", "full", "ragged"])
def test_encoder_matches_float64_library_vectors(enc, name):
    """small: 2 333 samples, right pads 1, 1, 3, 5; full: the 10 s clip, no right pad; ragged: 196 161 samples, right pads 1, 3,
    4, 7 -- the largest each strided layer can take.  Latent and every tap inside 1e-4."""
    _check_fixture(enc, name, "fused stem")


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_composed_stem_matches_float64_library_vectors(enc_composed, name):
    _check_fixture(enc_composed, name, "composed stem")


def test_batch_list_forward_and_legacy_names(params, enc):
    """A batch of two equals each clip alone, bit for bit; encode_list takes ragged lengths; forward uses channel 0 of a
    (channels, n) input; the hub checkpoint's `encoder.`-prefixed weight_g / weight_v names load."""
    from v2a_amd.encodec import EncodecEncoder
    a, b = wave(5000, 1), wave(5000, 2)
    both = enc.encoder(torch.stack([a, b])[:, None])
    assert both.shape == (2, 128, 16)
    assert torch.equal(both[0], enc.encoder(a.view(1, 1, -1))[0]) and torch.equal(both[1], enc.encoder(b.view(1, 1, -1))[0])
    assert not torch.equal(both[0], both[1])
    long, ragged = wave(240000, 3), wave(196161, 4)
    zs = enc.encode_list([long, ragged])
    assert [tuple(z.shape) for z in zs] == [(128, 750), (128, 614)]
    assert torch.equal(zs[0], enc.encoder(long.view(1, 1, -1))[0]) and torch.equal(zs[1], enc.encoder(ragged.view(1, 1, -1))[0])
    stereo = torch.stack([a, b])
    f = enc(stereo)
    assert f.shape == (1, 128, 16) and torch.equal(f[0], both[0]) and torch.equal(enc.forward(stereo), f)
    legacy = {"encoder." + k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v
              for k, v in params.items()}
    legacy["decoder.layers.0.conv.bias"] = torch.zeros(3)          # ignored
    assert torch.equal(EncodecEncoder(legacy, DEV).encoder(a.view(1, 1, -1)), both[:1])
    with pytest.raises(ValueError, match="at least 7"):
        enc.encoder(torch.zeros(1, 1, 1920))
    z7 = enc.encoder(wave(1921, 5).view(1, 1, -1))                 # the shortest accepted input
    assert z7.shape == (1, 128, 7) and bool(torch.isfinite(z7).all())


@pytest.mark.parametrize("n", [6400, 4001])
def test_round_trip_through_both_engines_matches_the_library(params, enc, n):
    """decoder(encoder(w)) has 320 * ceil(n / 320) samples and equals the library's fp32 decoder(encoder(w)) within 2e-4: two engines
    at 1e-4 each."""
    from transformers import EncodecConfig, EncodecModel
    from v2a_amd.encodec import EncodecDecoder
    from v2a_amd.synth import random_encodec_decoder_state_dict
    dsd = random_encodec_decoder_state_dict(2468)
    model = EncodecModel(EncodecConfig()).eval()
    model.encoder.load_state_dict(params, strict=True)
    model.decoder.load_state_dict(dsd, strict=True)
    w = wave(n, 11).view(1, 1, n)
    with torch.no_grad():
        zref = model.encoder(w)
        ref = model.decoder(zref)
    z = enc.encoder(w)
    got = EncodecDecoder(dsd, DEV).decoder(z)
    assert got.shape == ref.shape == (1, 1, 320 * -(-n // 320))
    ez, ew = float((z.cpu() - zref).abs().max()), float((got.cpu() - ref).abs().max())
    print(f"\nround trip n={n}: latent max |d| = {ez:.3e}, waveform max |d| = {ew:.3e} (max |wav| = {float(ref.abs().max()):.3f})")
    assert ez < 1e-4 and ew < 2e-4


def test_sample_takes_a_raw_wave_prompt(params, enc):
    """E2TTS(if_cond_proj_in=True, mel_spec_module=adapter).sample(cond=wave (2, nw)) == the call with the pre-encoded latent (x3:2157-2160),
    through the mel_spec_module argument and through load_audio_encoder."""
    from conftest import make_model
    from oracle import e2_cfm_oracle as O
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=128,
                      max_seq_len=256, cond_proj_in=True)
    P = O.init_params(cfg, 77)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=5, piano=True)
    nw = 8 * 320 - 100                                             # 8 latent frames of prompt, 40 frames generated
    waves = torch.stack([wave(nw, 21), wave(nw, 22)])
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, lens=torch.tensor([8, 8]),
              duration=torch.tensor([40, 33]), steps=4, cfg_strength=2.0, remove_parallel_component=False, return_raw_output=True)
    latent = enc.encoder(waves[:, None]).permute(0, 2, 1).contiguous()             # (2, 8, 128)
    assert latent.shape == (2, 8, 128)
    m = make_model(cfg, P, "fp32", mel_spec_module=lambda w: enc.encoder(w.unsqueeze(1)))
    ref = m.sample(latent, **kw).cpu()
    got = m.sample(waves, **kw).cpu()
    assert got.shape == (2, 40, 128) and torch.equal(got, ref)
    assert torch.equal(got[:, :8], latent.cpu())                   # x3:2260-2261: the prompt frames come back unchanged
    m2 = make_model(cfg, P, "fp32")
    with pytest.raises(NotImplementedError, match="mel_spec_module"):
        m2.sample(waves, **kw)
    assert isinstance(m2.load_audio_encoder(params), type(enc))
    assert torch.equal(m2.sample(waves, **kw).cpu(), ref)
