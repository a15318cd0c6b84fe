"""GPU: the HiFi-GAN vocoder (v2a_amd.HiFiGAN: csrc/hifigan.hip around the exact-fp32 v2a_gemm) against float64 -- the reference module's
own run where tests/golden/hifigan.npz holds it whole (wave, pre-tanh), tests/hifigan_ref.py, which that fixture pins, for the taps;
its bit-level promises; the three kernels alone; `E2TTS.sample(return_raw_output=False)` through `load_vocoder`.

Accuracy.  The bar of a tap is 4 x the fixture's error scale for it: the largest |reference fp32 - reference float64| over the
configuration's cases, the reference being the module of src/audioldm/hifigan/models.py on torch's CPU.  The factor 4 is the allowance
of tests/test_vocos_gpu.py: another summation order, another tanh.  The ratio max |x - x64| / scale is printed for every tap.
Measured on an MI355X (K_CHUNK = 512; profiles/hifigan.txt has every tap): 0.10 - 1.61 over every case, path and tap, the largest at
conv_pre of the full configuration at T = 16 (1.61), then up1 of the reduced one at T = 11 (1.51).

v2a_hifigan_conv alone is held to the textbook bound of its own summation: a chain of n fp32 additions of products errs by at most
gamma_n sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24; an output is C products per tap chain, k - 1 additions of the taps' sums, the
bias and the residual, and the fp32 product x * 0.1f of the leaky ReLU differs from the float64 one by less than 2 u of itself, so
n = C + k + 4 covers it, applied to sum |W| |lrelu x| + |bias| + |resid| evaluated in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
KW = {"full": {}, "small": dict(upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)}
CASES = {"full": ("t1", "t4", "t16", "ragged"), "small": ("t3", "t11")}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN, allow_pickle=False))


_engines: dict = {}
_ref64: dict = {}


def engine(cfg, fused):
    from v2a_amd import HiFiGAN
    if (cfg, fused) not in _engines:
        _engines[cfg, fused] = HiFiGAN(R.state_dict(cfg), DEV, fused=fused, **KW[cfg])
    return _engines[cfg, fused]


def ref64(cfg, tag):
    """float64 taps of one single-clip item, computed once and shared."""
    if (cfg, tag) not in _ref64:
        mel = dict(R.items(cfg))[tag]
        _ref64[cfg, tag] = R.generator(R.state_dict(cfg), mel, R.CONFIGS[cfg], torch.float64)
    return _ref64[cfg, tag]


def tap_ratios(voc, cfg, case, gold) -> dict:
    """One decode of a case with taps -> tap name -> max |x - x64| / the fixture's error scale, the largest over the case's clips
    (scripts/hifigan_probe.py prints the same table)."""
    taps = {}
    if case == "ragged":
        waves = voc.decode(R.ragged_mel(), lens=R.RAGGED_LENS, taps=taps)
        tags = [f"ragged{i}" for i in range(len(R.RAGGED_LENS))]
    else:
        waves = voc.decode(dict(R.items(cfg))[case], taps=taps)
        tags = [case]
    worst = {}
    for i, tag in enumerate(tags):
        want = ref64(cfg, tag)
        n = want["wave"].shape[1]
        assert tuple(waves[i].shape) == (n,) == gold[f"{cfg}_{tag}_wave"].shape
        assert torch.equal(waves[i], taps["wave"][i, :n])
        for name in R.tap_names(R.CONFIGS[cfg]):
            w64 = want[name][0]
            got = taps[name][i].double().cpu()[..., :w64.shape[-1]]
            assert got.shape == w64.shape, (tag, name)
            worst[name] = max(worst.get(name, 0.0), float((got - w64).abs().max()) / float(gold[f"{cfg}_scale_{name}"]))
        for name in ("wave", "pre"):                                               # the reference module's own float64, held whole
            err = float(np.abs(taps[name][i, :n].double().cpu().numpy() - gold[f"{cfg}_{tag}_{name}"]).max())
            worst[name] = max(worst[name], err / float(gold[f"{cfg}_scale_{name}"]))
    return worst


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("cfg,case", [(c, k) for c in CASES for k in CASES[c]])
def test_every_tap_within_four_error_scales_of_float64(gold, cfg, case, fused):
    worst = tap_ratios(engine(cfg, fused), cfg, case, gold)
    print(f"\nhifigan {cfg} {case} fused={fused}: max |x - x64| / error scale per tap: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = {k: round(v, 2) for k, v in worst.items() if not v <= FACTOR}
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False])
def test_a_clip_does_not_depend_on_its_batch_or_the_run(fused):
    voc = engine("full", fused)
    mel = R.ragged_mel()
    first = [w.clone() for w in voc.decode(mel, lens=R.RAGGED_LENS)]
    again = voc.decode(mel, lens=R.RAGGED_LENS)
    for i, n in enumerate(R.RAGGED_LENS):
        assert first[i].shape == (160 * n + 32,) and torch.equal(first[i], again[i]), i
        alone = voc.decode(mel[i:i + 1, :, :n])
        assert alone.shape == (1, 160 * n + 32) and torch.equal(alone[0], first[i]), i
    whole = voc.decode(mel)                                                        # no lens: every clip has T frames
    assert whole.shape == (3, 2592) and torch.equal(whole[1], first[1])
    big = torch.full((3, 2600), 7.0, device=DEV)
    out = big[:, 4:2596]
    assert voc.decode(mel, out=out) is out and torch.equal(out, whole)
    assert bool((big[:, :4] == 7).all()) and bool((big[:, 2596:] == 7).all())
    with pytest.raises(ValueError, match="out must be"):
        voc.decode(mel, out=torch.empty(3, 2591, device=DEV))


def _conv_case(C, k, d, seed):
    g = torch.Generator().manual_seed(seed)
    lens = (1, R_TILE - 1, R_TILE, R_TILE + 1, 2 * R_TILE + 25)
    T = max(lens)
    x = torch.randn(len(lens), T, C, generator=g)
    w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    bias = torch.randn(C, generator=g) * 0.1
    resid = torch.randn(len(lens), T, C, generator=g)
    return lens, T, x, w, bias, resid


R_TILE = 128


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_conv_kernel_alone(C, k, d, resid):
    """Five clips of 1, tile - 1, tile, tile + 1 and 2 tiles + 25 frames in ONE launch, each against float64 as if it were alone."""
    from v2a_amd import _lib as L, hifigan as H
    assert H.TILE == R_TILE
    lens, T, x, w, bias, res = _conv_case(C, k, d, 1000 * C + 10 * k + d)
    pitch = T + 3
    xg = torch.zeros(len(lens), pitch, C, device=DEV)
    xg[:, :T] = x.to(DEV)
    xg[:, T:] = 9.0                                                                # rows behind T and behind lens hold values the kernel must not read
    rg = torch.zeros(len(lens), pitch, C, device=DEV)
    rg[:, :T] = res.to(DEV)
    out = torch.full((len(lens), pitch, C), -5.0, device=DEV)
    wp, bg = H.pack_conv_fragments(w).to(DEV), bias.to(DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    L.check(L.lib().v2a_hifigan_conv(xg.data_ptr(), C, pitch, len(lens), T, C, lens_dev.data_ptr(), wp.data_ptr(), bg.data_ptr(), k, d, 0.1,
                                     rg.data_ptr() if resid else 0, C, out.data_ptr(), C, L.stream_ptr()))
    got = out.cpu()
    u, n_chain = 2.0 ** -24, C + k + 4
    gamma = n_chain * u / (1 - n_chain * u)
    for i, n in enumerate(lens):
        xi, ri = x[i, :n].t()[None].double(), res[i, :n].t()[None].double() if resid else None
        want = R.conv1d(xi, w.double(), bias.double(), d, 0.1, ri)[0].t()
        mag = F.conv1d(F.leaky_relu(xi, 0.1).abs(), w.double().abs(), bias.double().abs(), dilation=d, padding=(k - 1) * d // 2)
        bound = gamma * ((mag + ri.abs()) if resid else mag)[0].t()
        err = (got[i, :n].double() - want).abs()
        assert bool((err <= bound).all()), (i, n, float((err / bound).max()))
        assert bool((got[i, n:] == -5.0).all()), (i, n)                            # nothing behind the clip's own length is written


@pytest.mark.parametrize("slope", [0.1, 0.01])
@pytest.mark.parametrize("C", [32, 1024])
@pytest.mark.parametrize("nsrc", [1, 2, 3])
def test_act_pad_equals_torch_fp32_bit_for_bit(nsrc, C, slope):
    from v2a_amd import _lib as L
    g = torch.Generator().manual_seed(nsrc * 7 + C)
    lens, T, halo, src_pitch = (5, 9, 1), 9, 4, 11
    out_pitch = T + 2 * halo + 3
    srcs = [torch.randn(len(lens), src_pitch, C, generator=g) for _ in range(nsrc)]
    dev = [s.to(DEV) for s in srcs]
    out = torch.full((len(lens), out_pitch, C), 3.0, device=DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ptr = [t.data_ptr() for t in dev] + [0] * (3 - nsrc)
    L.check(L.lib().v2a_hifigan_act_pad(ptr[0], ptr[1], ptr[2], src_pitch, C, len(lens), T, C, lens_dev.data_ptr(), float(nsrc), slope, out.data_ptr(),
                                        out_pitch, halo, L.stream_ptr()))
    got = out.cpu()
    total = srcs[0]
    for s in srcs[1:]:
        total = total + s                                                          # (s0 + s1) + s2
    want = F.leaky_relu(total / nsrc if nsrc > 1 else total, slope)
    for i, n in enumerate(lens):
        assert torch.equal(got[i, halo:halo + n], want[i, :n]), i
        assert bool((got[i, :halo] == 0).all()) and bool((got[i, halo + n:] == 0).all()), i      # the halo and everything behind the clip: exactly zero


def test_post_int16_truncates_its_own_wave(gold):
    voc = engine("full", True)
    mel = dict(R.items("full"))["t16"]
    wave = voc.decode(mel)
    pcm = voc.decode_to_waveform(mel.permute(0, 2, 1)[:, None])
    assert pcm.dtype == torch.int16 and pcm.shape == wave.shape == (1, 2592)
    assert np.array_equal(pcm.cpu().numpy(), (wave.cpu().numpy() * 32768).astype("int16"))
    assert int(np.abs(pcm.cpu().numpy()[0].astype(np.int32) - gold["full_t16_pcm"].astype(np.int32)).max()) <= 1
    err = float(np.abs(wave[0].double().cpu().numpy() - gold["full_t16_wave"]).max())
    assert err <= FACTOR * float(gold["full_scale_wave"]), err
    ragged = voc.decode_to_waveform(R.ragged_mel().permute(0, 2, 1)[:, None], lens=R.RAGGED_LENS)
    assert [tuple(r.shape) for r in ragged] == [(832,), (2592,), (1472,)]
    for i, n in enumerate(R.RAGGED_LENS):
        assert int(np.abs(ragged[i].cpu().numpy().astype(np.int32) - gold[f"full_ragged{i}_pcm"].astype(np.int32)).max()) <= 1, i


def test_post_saturates_at_full_scale():
    """tanh rounds to +-1 from |pre| of about 9: the product +-32768 is stored as 32767 / -32768."""
    from v2a_amd import _lib as L
    C, T = 32, 6
    a = torch.zeros(1, T, C, device=DEV)
    a[0, :, 0] = torch.tensor([40.0, -40.0, 0.0, 0.25, -0.25, 1e-6], device=DEV)
    w = torch.zeros(7, C, device=DEV)
    w[3, 0] = 1.0                                                                  # the centre tap of channel 0: pre = a[t][0]
    bias = torch.zeros(1, device=DEV)
    wave, pre = torch.zeros(1, T, device=DEV), torch.zeros(1, T, device=DEV)
    pcm = torch.zeros(1, T, dtype=torch.int16, device=DEV)
    L.check(L.lib().v2a_hifigan_post(a.data_ptr(), T, 1, T, C, 0, w.data_ptr(), bias.data_ptr(), wave.data_ptr(), pcm.data_ptr(), pre.data_ptr(), T,
                                     L.stream_ptr()))
    assert torch.equal(pre, a[:, :, 0])
    assert pcm[0, :3].cpu().tolist() == [32767, -32768, 0] and int(pcm[0, 3]) == -int(pcm[0, 4]) and int(pcm[0, 5]) == 0
    assert np.array_equal(pcm.cpu().numpy()[:, 2:], (wave.cpu().numpy()[:, 2:] * 32768).astype("int16"))


def test_sample_decodes_through_the_loaded_hifigan():
    """E2TTS(num_channels=64).sample(return_raw_output=False) after load_vocoder(HiFiGAN): element i = decode(raw[i, :duration[i]].T[None])[0]
    bit for bit, 160 duration[i] + 32 samples."""
    from conftest import make_model
    from oracle import e2_cfm_oracle as O
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=64, max_seq_len=64)
    P = O.init_params(cfg, 4242)
    b, n = 2, 12
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, b, n, nc=5, seed=11, piano=True)
    voc = engine("full", True)
    m = make_model(cfg, P, "fp32")
    duration = torch.tensor([n, n - 5])
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, steps=2, cfg_strength=2.0, remove_parallel_component=False,
              lens=duration, duration=duration)
    cond = torch.zeros(b, n, 64)
    raw = m.sample(cond, return_raw_output=True, **kw)
    assert m.load_vocoder(voc) is voc and m.vocos is voc
    audio = m.sample(cond, return_raw_output=False, **kw)
    assert isinstance(audio, list) and len(audio) == b
    for k in range(b):
        dk = int(duration[k])
        want = voc.decode(raw[k, :dk].transpose(0, 1)[None])[0]
        assert audio[k].shape == (160 * dk + 32,) and torch.equal(audio[k], want), k
        assert bool(torch.isfinite(audio[k]).all()) and float(audio[k].abs().max()) <= 1.0
