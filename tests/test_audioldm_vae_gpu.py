"""GPU: the AudioLDM VAE decoder (v2a_amd.AudioLDMVaeDecoder / VaeVocoder: csrc/audioldm_vae.hip around the exact-fp32 v2a_gemm) -- the
six kernels alone through the C ABI against float64, the engine against the reference module's own float64 run
(tests/golden/audioldm_vae.npz: the mel whole, 64 sampled entries of every other tap), its bit-level promises, and
`E2TTS.sample(return_raw_output=False)` through `load_vocoder`.

Accuracy of the engine.  The bar of a tap is 4 x the fixture's error scale for it: the largest |reference fp32 - reference float64| over
the cases of its configuration and regime, the reference being the module of src/audioldm/variational_autoencoder/modules.py on torch's
CPU.  The factor 4 is the allowance of tests/test_vocos_gpu.py and tests/test_hifigan_gpu.py: another summation order, another exp.  The
ratio max |x - x64| / scale is printed for every tap.

Accuracy of the kernels alone, u = 2^-24, each bound applied to float64 evaluations of the same fp32 inputs:
  * gn_act_pad: y = ((x - mean) rstd) gamma + beta with mean and rstd rounded from double once: the rounding of mean costs |mean| u
    in x - mean, then four rounded operations: |err y| <= u (rstd |gamma| |mean| + 4 |t gamma| + |y|), t = (x - mean) rstd; the double
    statistics add nothing visible (a variance of 1 under a mean of 100 loses 13 of 53 bits).  swish(y) = y / (1 + expf(-y)): |swish'| <= 1.1
    carries the error of y, expf (1 ulp), the addition and the division add 4 u |swish|.  A 1 % margin covers the second-order terms.
  * softmax: v = scale s is one rounded product (|v| u), v - max another (|v - max| u), and exp turns an absolute error of its argument
    into a relative one of its value, plus 2 u for expf; the sum is at most 11 additions deep (n / 256 per thread, 6 butterfly steps,
    2 tree steps), the division one more: |p - p64| <= (2 max_j (|v_j| + |v_j - max| + 2) + 13) u p64, and |sum_j p_j - 1| <= 16 u.
  * stage_in: a chain of zc fmas from the bias: gamma_(zc + 1) sum |terms|.
  * upsample_pad, the layout of stage_in (identity weight) and conv_out (its documented fma chain, evaluated on the host through exact
    float64 products) are compared bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import audioldm_vae_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
U = 2.0 ** -24
CASES = {"full": tuple(f"l{l}" for l in R.FULL_L) + ("ragged",), "small": tuple(f"l{l}" for l in R.SMALL_L)}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN, allow_pickle=False))


_engines: dict = {}


def engine(cfg, regime, k_chunk=512):
    from v2a_amd import AudioLDMVaeDecoder
    key = (cfg, regime, k_chunk)
    if key not in _engines:
        _engines[key] = AudioLDMVaeDecoder(R.state_dict(cfg, regime), DEV, k_chunk=k_chunk)
    return _engines[key]


def L():
    from v2a_amd import _lib
    return _lib


# ---- (a) kernel by kernel -------------------------------------------------------------------------------------------------------

def _flat_map(x, lens, Wp, pitch):
    """x (b, H, W, C) -> a flat map of row pitch Wp and `pitch` rows per clip whose every other element is NaN: nothing but the clips' own
    pixels may be read."""
    b, H, W, C = x.shape
    m = torch.full((b, pitch, C), float("nan"))
    v = m[:, :H * Wp].view(b, H, Wp, C)
    for i, n in enumerate(lens):
        v[i, :n, :W] = x[i, :n]
    return m.to(DEV)


def _gn_case(C, H, W, seed, mean):
    g = torch.Generator().manual_seed(seed)
    lens = (H, max(1, H // 2), 0)
    x = torch.randn(len(lens), H, W, C, generator=g) * (1 + torch.arange(C) % 3) + mean + torch.randn(C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    return lens, x, gamma, beta


@pytest.mark.parametrize("border", [1, 0])
@pytest.mark.parametrize("mean", [0.0, 100.0])
@pytest.mark.parametrize("H,W", [(1, 16), (5, 16), (32, 16), (20, 64)])            # 16 and 80 pixels: below the tile of 512; 512: one tile; 1280: 2.5
@pytest.mark.parametrize("C", [32, 64, 512])
def test_group_norm_kernels_alone(C, H, W, mean, border):
    _lib = L()
    lens, x, gamma, beta = _gn_case(C, H, W, 7 * C + H + W, mean)
    b, Wp = len(lens), W + 2
    pitch = (H + 2) * Wp + 5
    tiles = (H * W + 511) // 512 + 1                                               # one more than needed: it must come back zero
    src = _flat_map(x, lens, Wp, pitch)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    part = torch.full((b, tiles, 32, 2), -1.0, dtype=torch.float64, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)                                           # named: alive until the kernels have run
    _lib.check(_lib.lib().v2a_vae_gn_stats(src.data_ptr(), pitch, Wp, b, H, W, C, lens_dev.data_ptr(), part.data_ptr(), tiles, _lib.stream_ptr()))
    cpg = C // 32
    x64 = x.double()
    for i, n in enumerate(lens):
        px = x64[i, :n].reshape(n * W, 32, cpg)
        for t in range(tiles):
            sel = px[t * 512:(t + 1) * 512]
            got = part[i, t].cpu()
            if sel.numel() == 0:
                assert bool((got == 0).all()), (i, t)                              # a tile without a pixel of the clip: exactly zero
                continue
            s, ss = sel.sum((0, 2)), (sel * sel).sum((0, 2))
            gam = 2 * sel.shape[0] * cpg * 2.0 ** -53                              # two double sums of that many terms, in different orders
            assert bool(((got[:, 0] - s).abs() <= gam * sel.abs().sum((0, 2))).all()) and bool(((got[:, 1] - ss).abs() <= gam * ss).all()), (i, t)
    for swish in (0, 1):
        Wd, Hd = W + 2 * border, H + 2 * border
        out_pitch = Hd * Wd + 3
        out = torch.full((b, out_pitch, C), 7.0, device=DEV)
        _lib.check(_lib.lib().v2a_vae_gn_act_pad(src.data_ptr(), pitch, Wp, b, H, W, C, lens_dev.data_ptr(), part.data_ptr(), tiles, gd.data_ptr(),
                                                 bd.data_ptr(), 1e-6, swish, out.data_ptr(), out_pitch, border, _lib.stream_ptr()))
        got = out.cpu()
        assert bool(torch.isfinite(got).all())
        for i, n in enumerate(lens):
            grid = got[i, :Hd * Wd].view(Hd, Wd, C)
            inner = grid[border:border + n, border:border + W]
            mask = torch.ones(Hd, Wd, dtype=torch.bool)
            mask[border:border + n, border:border + W] = False
            assert bool((grid[mask] == 0).all()) and bool((got[i, Hd * Wd:] == 0).all()), (i, swish)      # border, rows behind lens, the tail: exactly 0
            if n == 0:
                continue
            px = x64[i, :n].reshape(n * W, 32, cpg)
            m = px.mean((0, 2), keepdim=True)
            r = 1.0 / torch.sqrt((px * px).mean((0, 2), keepdim=True) - m * m + 1e-6)
            g64, b64 = gamma.double().view(32, cpg), beta.double().view(32, cpg)
            t = (px - m) * r
            y = t * g64 + b64
            bound = U * (r * g64.abs() * m.abs() + 4 * (t * g64).abs() + y.abs())
            want = y
            if swish:
                want = y * torch.sigmoid(y)
                bound = 1.1 * bound + 4 * U * want.abs()
            err = (inner.reshape(n * W, 32, cpg).double() - want).abs()
            assert bool((err <= 1.01 * bound).all()), (i, swish, float((err / bound).max()))


@pytest.mark.parametrize("C,H,W", [(32, 1, 16), (64, 5, 16), (512, 3, 32)])
def test_upsample_pad_equals_nearest_interpolation_bit_for_bit(C, H, W):
    _lib = L()
    g = torch.Generator().manual_seed(C + H)
    lens = (H, max(1, H - 1), 0)
    b, Wp = len(lens), W + 2
    x = torch.randn(b, H, W, C, generator=g)
    pitch = (H + 2) * Wp
    src = _flat_map(x, lens, Wp, pitch)
    H2, W2 = 2 * H, 2 * W
    out_pitch = (H2 + 2) * (W2 + 2) + 2
    out = torch.full((b, out_pitch, C), 7.0, device=DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().v2a_vae_upsample_pad(src.data_ptr(), pitch, Wp, b, H, W, C, lens_dev.data_ptr(), out.data_ptr(), out_pitch, _lib.stream_ptr()))
    got = out.cpu()
    for i, n in enumerate(lens):
        want = torch.zeros(H2 + 2, W2 + 2, C)
        if n:
            want[1:2 * n + 1, 1:W2 + 1] = F.interpolate(x[i, :n].permute(2, 0, 1)[None], scale_factor=2.0, mode="nearest")[0].permute(1, 2, 0)
        assert torch.equal(got[i, :(H2 + 2) * (W2 + 2)].view(H2 + 2, W2 + 2, C), want), i
        assert bool((got[i, (H2 + 2) * (W2 + 2):] == 0).all()), i


@pytest.mark.parametrize("n", [16, 80, 656])
def test_softmax_alone(n):
    _lib = L()
    g = torch.Generator().manual_seed(n)
    rows, ld, scale = 5, n + 16, float(np.float32(512 ** -0.5))
    s = torch.randn(rows, ld, generator=g) * 40
    s[0, :n] = torch.where(torch.rand(n, generator=g) < 0.5, 80.0, -80.0) / scale     # logits of +-80
    s[1, :n] = -80.0 / scale
    s[1, n // 2] = 80.0 / scale                                                        # one winner 160 above the rest
    s[2, :n] = 0.0
    s[:, n:] = float("nan")                                                            # the padding is written, never read
    dev = s.to(DEV)
    _lib.check(_lib.lib().v2a_vae_softmax(dev.data_ptr(), ld, rows, n, scale, _lib.stream_ptr()))
    got = dev.cpu()
    assert bool((got[:, n:] == 0).all())
    v = s[:, :n].double() * float(np.float32(scale))
    want = torch.softmax(v, 1)
    vmax = v.max(1, keepdim=True).values
    rel = (2 * (v.abs() + (v - vmax).abs() + 2).max(1, keepdim=True).values + 13) * U
    err = (got[:, :n].double() - want).abs()
    assert bool((err <= rel * want + 1e-37).all()), float((err / (rel * want + 1e-37)).max())
    assert float((got[:, :n].double().sum(1) - 1).abs().max()) <= 16 * U
    assert torch.equal(got[2, :n], torch.full((n,), 1.0 / n))                          # equal logits: e = 1, sum = n exactly, one rounded division


@pytest.mark.parametrize("mode", ["emb", "z"])
def test_stage_in_layout_and_chain(mode):
    _lib = L()
    g = torch.Generator().manual_seed(3)
    b, l, zc, W, cpad = 3, 6, 8, 16, 16
    lens = (6, 2, 0)
    emb = torch.randn(b, zc * W, l, generator=g)
    z = R.to_z(emb).contiguous()                                                       # (b, zc, l, W): the torch reshape
    src, strides = (emb, (zc * W * l, W * l, 1, l)) if mode == "emb" else (z, (zc * l * W, l * W, W, 1))
    pitch = (l + 2) * (W + 2) + 1
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for w, bias in ((torch.eye(zc), torch.zeros(zc)), (torch.randn(zc, zc, generator=g), torch.randn(zc, generator=g))):
        out = torch.full((b, pitch, cpad), 7.0, device=DEV)
        sd, wd, bd = src.to(DEV), w.to(DEV), bias.to(DEV)                          # named: alive until the kernel has run
        _lib.check(_lib.lib().v2a_vae_stage_in(sd.data_ptr(), *strides, b, l, W, zc, lens_dev.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                               out.data_ptr(), cpad, pitch, _lib.stream_ptr()))
        got = out.cpu()
        identity = bool((w == torch.eye(zc)).all())
        for i, n in enumerate(lens):
            grid = got[i, :(l + 2) * (W + 2)].view(l + 2, W + 2, cpad)
            zi = z[i, :, :n].permute(1, 2, 0)                                          # (n, W, zc)
            want = torch.zeros(l + 2, W + 2, cpad, dtype=torch.float64)
            want[1:n + 1, 1:W + 1, :zc] = zi.double() @ w.double().t() + bias.double()
            mask = torch.ones(l + 2, W + 2, cpad, dtype=torch.bool)
            mask[1:n + 1, 1:W + 1, :zc] = False
            assert bool((grid[mask] == 0).all()) and bool((got[i, (l + 2) * (W + 2):] == 0).all()), i      # border, padded channels, rows behind lens
            if identity:
                assert torch.equal(grid[1:n + 1, 1:W + 1, :zc], zi), i                 # the layout, bit for bit
            else:
                mag = zi.double().abs() @ w.double().abs().t() + bias.double().abs()
                gam = (zc + 1) * U / (1 - (zc + 1) * U)
                assert bool(((grid[1:n + 1, 1:W + 1, :zc].double() - want[1:n + 1, 1:W + 1, :zc]).abs() <= gam * mag).all()), i


def _fma_chain_f32(a_rows, w, bias):
    """acc = bias; acc = fl32(w[k] * a[:, k] + acc) for k ascending: the product of two fp32 numbers is exact in float64, the sum is
    rounded to float64 and then to fp32."""
    acc = np.full(a_rows.shape[0], np.float32(bias), dtype=np.float32)
    a64, w64 = a_rows.astype(np.float64), w.astype(np.float64)
    for k in range(w.shape[0]):
        acc = (w64[k] * a64[:, k] + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("C,H,W", [(32, 5, 16), (128, 3, 64)])
def test_conv_out_equals_its_documented_fma_chain_bit_for_bit(C, H, W):
    _lib = L()
    g = torch.Generator().manual_seed(C)
    lens = (H, max(1, H - 2), 0)
    b, Wp = len(lens), W + 2
    pitch = (H + 2) * Wp + 4
    a = torch.zeros(b, pitch, C)
    a[:, :(H + 2) * Wp].view(b, H + 2, Wp, C)[:, 1:H + 1, 1:W + 1] = torch.randn(b, H, W, C, generator=g)
    w, bias = torch.randn(9 * C, generator=g) / (9 * C) ** 0.5, torch.randn(1, generator=g)
    out = torch.full((b, H, W), 7.0, device=DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)                                # named: alive until the kernel has run
    _lib.check(_lib.lib().v2a_vae_conv_out(ad.data_ptr(), pitch, b, H, W, C, lens_dev.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                           out.data_ptr(), _lib.stream_ptr()))
    got = out.cpu().numpy()
    for i, n in enumerate(lens):
        assert bool((got[i, n:] == 0).all()), i
        if n == 0:
            continue
        grid = a[i, :(H + 2) * Wp].view(H + 2, Wp, C)
        # the window of pixel (y, x) in (ky, kx, c) order: bordered rows y + ky, pixels x .. x + 2
        rows = torch.stack([torch.cat([grid[y + ky, x:x + 3].reshape(-1) for ky in range(3)]) for y in range(n) for x in range(W)]).numpy()
        want = _fma_chain_f32(rows, w.numpy(), float(bias)).reshape(n, W)
        assert np.array_equal(got[i, :n], want), (i, float(np.abs(got[i, :n] - want).max()))


# ---- (b) the engine against the reference module -----------------------------------------------------------------------------

def tap_ratios(dec, cfg, regime, case, gold) -> dict:
    """One decode of a case with taps -> tap name -> max |x - x64| / the fixture's error scale, the largest over the case's clips
    (scripts/audioldm_vae_probe.py prints the same table)."""
    names = R.tap_names(R.CONFIGS[cfg])
    scale = dict(zip(names, gold[f"{cfg}_{regime}_scale"]))
    taps = {}
    if case == "ragged":
        from v2a_amd import AudioLDMVaeDecoder
        if (cfg, regime, "ragged") not in _engines:
            _engines[cfg, regime, "ragged"] = AudioLDMVaeDecoder(R.state_dict(cfg, regime), DEV, scale_factor=R.RAGGED_SCALE)
        d = _engines[cfg, regime, "ragged"]
        mel = d.decode_latents(R.ragged_emb(), lens=R.RAGGED_LENS, taps=taps)
        tags = [f"ragged{i}" for i in range(len(R.RAGGED_LENS))]
    else:
        mel = dec.decode_latents(dict((t, e) for t, e, _ in R.items(cfg))[case], taps=taps)
        tags = [case]
    assert torch.equal(mel, taps["mel"])
    worst = {}
    for i, tag in enumerate(tags):
        key = f"{cfg}_{regime}_{tag}"
        want = gold[key + "_mel"]
        got = taps["mel"][i, 0, :want.shape[0]].double().cpu().numpy()
        assert got.shape == want.shape, key
        worst["mel"] = max(worst.get("mel", 0.0), float(np.abs(got - want).max()) / scale["mel"])
        assert bool((taps["mel"][i, 0, want.shape[0]:] == 0).all()), key                 # rows behind the clip's own length are zero
        for t, name in enumerate(names[:-1]):
            shape, idx = tuple(gold[key + "_tap_shape"][t]), gold[key + "_tap_idx"][t].astype(np.int64)
            a = taps[name][i:i + 1, :, :shape[2]]
            assert tuple(a.shape) == shape, (key, name)
            v = a.double().cpu().numpy()[tuple(idx.T)]
            worst[name] = max(worst.get(name, 0.0), float(np.abs(v - gold[key + "_tap_val"][t]).max()) / scale[name])
    return worst


@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("cfg,case", [(c, k) for c in CASES for k in CASES[c]])
def test_every_tap_within_four_error_scales_of_float64(gold, cfg, case, regime):
    worst = tap_ratios(engine(cfg, regime), cfg, regime, case, gold)
    print(f"\naudioldm_vae {cfg} {regime} {case}: max |x - x64| / error scale per tap: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = {k: round(v, 2) for k, v in worst.items() if not v <= FACTOR}
    assert not bad, bad


# ---- (c) promises ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_a_clip_does_not_depend_on_its_batch_or_the_run(regime):
    dec = engine("full", regime)
    emb = R.ragged_emb()
    first = dec.decode_latents(emb, lens=R.RAGGED_LENS).clone()
    again = dec.decode_latents(emb, lens=R.RAGGED_LENS)
    assert first.shape == (3, 1, 64, 64) and torch.equal(first, again)
    for i, n in enumerate(R.RAGGED_LENS):
        alone = dec.decode_latents(emb[i:i + 1, :, :n])
        assert alone.shape == (1, 1, 4 * n, 64) and torch.equal(alone[0], first[i, :, :4 * n]), i
        assert bool((first[i, :, 4 * n:] == 0).all()), i
    z = R.to_z(emb).contiguous()
    assert torch.equal(dec.decode_first_stage(z, lens=R.RAGGED_LENS), first)          # the reshape inside stage_in is the torch one


@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("case", CASES["small"])
def test_tiny_k_chunk_stays_within_the_same_bar(gold, case, regime):
    """k_chunk = 64: every RESID chain of the engine runs with more than one launch (the 3x3 convolutions in 5 and 9, the 1x1 ones and
    the attention's in 1 .. 3)."""
    worst = tap_ratios(engine("small", regime, 64), "small", regime, case, gold)
    print(f"\naudioldm_vae small {regime} {case} k_chunk=64: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    bad = {k: round(v, 2) for k, v in worst.items() if not v <= FACTOR}
    assert not bad, bad


def _vocoder():
    import hifigan_ref as HR
    from v2a_amd import HiFiGAN, VaeVocoder
    if "voc" not in _engines:
        _engines["voc"] = VaeVocoder(engine("full", "plain"), HiFiGAN(HR.state_dict("full"), DEV))
    return _engines["voc"]


def test_vae_vocoder_equals_its_two_halves_and_the_composed_float64_reference():
    import hifigan_ref as HR
    voc = _vocoder()
    l = 3
    emb = dict((t, e) for t, e, _ in R.items("small"))["l3"]                           # (1, 128, 3): latents are the same for every configuration
    wave = voc.decode(emb)
    assert wave.shape == (1, 640 * l + 32) and wave.dtype == torch.float32
    mel = voc.decoder.decode_latents(emb)                                              # (1, 1, 12, 64)
    assert torch.equal(wave, voc.hifigan.decode(mel[:, 0].transpose(1, 2)))
    pcm = voc.decode_to_waveform(emb)
    assert pcm.dtype == torch.int16 and np.array_equal(pcm.cpu().numpy(), (wave.cpu().numpy() * 32768).astype("int16"))
    ref = {}
    for dt in (torch.float64, torch.float32):                                          # the two restatements, composed, in both precisions
        m = R.decoder(R.state_dict("full", "plain"), R.to_z(emb), R.CONFIGS["full"], 1.0, dt)["mel"]
        ref[dt] = HR.generator(HR.state_dict("full"), m[:, 0].transpose(1, 2), HR.CONFIGS["full"], dt)["wave"]
    scale = float((ref[torch.float32].double() - ref[torch.float64]).abs().max())
    err = float((wave.double().cpu() - ref[torch.float64]).abs().max())
    print(f"\nVaeVocoder l = {l}: max |wave - wave64| = {err:.3e} = {err / scale:.2f} x the composed reference's own fp32 error {scale:.3e}")
    assert err <= FACTOR * scale
    ragged = voc.decode(R.ragged_emb(), lens=R.RAGGED_LENS)
    assert [tuple(w.shape) for w in ragged] == [(640 * n + 32,) for n in R.RAGGED_LENS]
    for i, n in enumerate(R.RAGGED_LENS):
        assert torch.equal(ragged[i], voc.decode(R.ragged_emb()[i:i + 1, :, :n])[0]), i


def test_sample_decodes_through_the_loaded_vae_vocoder():
    """E2TTS(num_channels=128).sample(return_raw_output=False) after load_vocoder(VaeVocoder): element i = decode(raw[i, :duration[i]].T[None])[0]
    bit for bit, 640 duration[i] + 32 samples."""
    from conftest import make_model
    from oracle import e2_cfm_oracle as O
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=128, max_seq_len=64)
    P = O.init_params(cfg, 4243)
    b, n = 2, 6
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, b, n, nc=5, seed=12, piano=True)
    voc = _vocoder()
    m = make_model(cfg, P, "fp32")
    duration = torch.tensor([n, n - 2])
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, steps=2, cfg_strength=2.0, remove_parallel_component=False,
              lens=duration, duration=duration)
    cond = torch.zeros(b, n, 128)
    raw = m.sample(cond, return_raw_output=True, **kw)
    assert m.load_vocoder(voc) is voc and m.vocos is voc
    audio = m.sample(cond, return_raw_output=False, **kw)
    assert isinstance(audio, list) and len(audio) == b
    for k in range(b):
        dk = int(duration[k])
        want = voc.decode(raw[k, :dk].transpose(0, 1)[None])[0]
        assert audio[k].shape == (640 * dk + 32,) and torch.equal(audio[k], want), k
        assert bool(torch.isfinite(audio[k]).all()) and float(audio[k].abs().max()) <= 1.0
