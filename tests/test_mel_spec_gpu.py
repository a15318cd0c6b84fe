"""GPU: the log-mel front end (v2a_amd.MelSpec: v2a_mel_pad, one exact-fp32 v2a_gemm over overlapping rows, v2a_mel_from_dft) against
float64, its bit-level promises, and the raw-wave paths of E2TTS through it.

Reference, on the CPU in float64 at test time: S = torch.stft(x.double(), ...) (divided by sqrt(sum(w^2)) when normalize),
mel64 = fb64.T @ |S|**power with fb64 = mel_filterbank(...) (tests/test_mel_spec_refs.py pins both tables), log64 = log(max(mel64, 1e-5)).

Accuracy.  With u = 2^-24 and ||x_t w||_2 the 2-norm of the windowed frame, the error scale of mel value m of frame t is
    power 1:  S[m, t] = u (sqrt(n_fft) sum_k fb[k, m] ||x_t w||_2 + mel64[m, t])
    power 2:  S[m, t] = u (2 sqrt(n_fft) (fb.T @ |S|)[m, t] ||x_t w||_2 + mel64[m, t])
-- a bin's re and im carry about u sqrt(n_fft) ||x_t w||_2 of summation error, a magnitude no more, a power 2 |S| times that, and the
second term covers the fp32 rounding of the weights and of the mel chain.  r = max |mel - mel64| / S.  The yardstick is r_cpu32, the same
ratio for torch's CPU fp32 evaluation from the same fp32 tables (fp32 matmul of the frames by the basis, magnitude, fp32 matmul by the
filterbank); the assertion is r_gpu <= 4 r_cpu32: the margin covers another summation order and another square root, and is far below
what an indexing, window or padding mistake gives (r of 1e3 and more).  The log output is held to
    |log_gpu - log64| <= |mel_gpu - mel64| / min(max(mel_gpu, eps), max(mel64, eps)) + 2 ulp(log64)
for every entry: the clamp is 1-Lipschitz and log has slope 1 / x.

Each wave batch has three rows: two of seeded noise under a random envelope and a tonal one, 0.9 sin(0.37 n) + 1e-4 noise, whose quiet
bands lie beside a loud one.  nw = 33 at (64, 16) is the shortest wave a reflect pad of 32 allows (T = 3, fewer rows than any tile); the
(2048, 512) case is the one whose bins of 16 frames pass 64 KB of LDS.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
U = 2.0 ** -24

# (n_fft, hop, win, n_mels, sr, nw, power, norm, normalize, center)
CASES = [
    (64, 16, 64, 10, 24000, 101, 1, None, False, True),
    (64, 16, 64, 10, 24000, 33, 1, None, False, True),
    (64, 16, 48, 10, 16000, 257, 2, "slaney", True, True),
    (256, 64, 200, 40, 24000, 1000, 2, None, False, False),
    (1024, 256, 1024, 100, 24000, 513, 1, None, False, True),
    (1024, 256, 1024, 100, 24000, 2400, 1, None, False, True),
    (1024, 256, 1024, 100, 24000, 24007, 1, None, False, True),
    (2048, 512, 2048, 128, 44100, 3000, 2, None, False, True),
]


def make_waves(nw, seed):
    """(3, nw) fp32: two rows of noise under a random envelope, one tonal row with quiet bands beside a loud one."""
    g = torch.Generator().manual_seed(seed)
    knots = torch.rand(2, 1, max(2, nw // 97 + 2), generator=g)
    env = F.interpolate(knots, size=nw, mode="linear", align_corners=True)[:, 0]
    noise = torch.randn(2, nw, generator=g) * env
    n = torch.arange(nw, dtype=torch.float64)
    tonal = (0.9 * torch.sin(0.37 * n)).float() + 1e-4 * torch.randn(nw, generator=g)
    return torch.cat([noise, tonal[None]], 0).contiguous()


def module(case, device=DEV):
    from v2a_amd import MelSpec
    n_fft, hop, win, n_mels, sr, _, power, norm, normalize, center = case
    return MelSpec(filter_length=n_fft, hop_length=hop, win_length=win, n_mel_channels=n_mels, sampling_rate=sr, normalize=normalize,
                   power=power, norm=norm, center=center, device=device)


def reference64(case, x):
    """-> dict(mel64 (b, n_mels, T), log64, scale S, r_cpu32) for waves x (b, nw) fp32."""
    from v2a_amd.mel import mel_filterbank, stft_window
    n_fft, hop, win, n_mels, sr, _, power, norm, normalize, center = case
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    S = torch.stft(x.double(), n_fft, hop, win, window=w, center=center, pad_mode="reflect", return_complex=True)
    weff = stft_window(n_fft, win)
    if normalize:
        S, weff = S / w.pow(2).sum().sqrt(), weff / w.pow(2).sum().sqrt()
    mag = S.abs()                                                                  # (b, bins, T)
    fb64 = mel_filterbank(n_fft // 2 + 1, n_mels, sr, norm=norm)                   # (bins, n_mels)
    mel64 = torch.einsum("km,bkt->bmt", fb64, mag ** power)
    xp = F.pad(x[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0] if center else x
    frames = xp.unfold(1, n_fft, hop)                                              # (b, T, n_fft) fp32
    fnorm = (frames.double() * weff).norm(dim=-1)[:, None, :]                      # (b, 1, T)
    if power == 1:
        scale = U * (math.sqrt(n_fft) * fb64.sum(0)[None, :, None] * fnorm + mel64)
    else:
        scale = U * (2.0 * math.sqrt(n_fft) * torch.einsum("km,bkt->bmt", fb64, mag) * fnorm + mel64)
    # the yardstick: torch's CPU fp32 evaluation from the fp32 tables the device gets
    ms = module(case, "cpu")
    basis32 = ms.host_tables()[0]
    nb = ms.n_bins
    Y = frames @ basis32[:2 * nb, :n_fft].T                                        # (b, T, 2 bins): re, im interleaved
    p32 = Y[..., 0::2] ** 2 + Y[..., 1::2] ** 2
    p32 = p32.sqrt() if power == 1 else p32
    mel32 = (p32 @ fb64.float()).permute(0, 2, 1)
    return dict(mel64=mel64, log64=mel64.clamp(min=EPS).log(), scale=scale, r_cpu32=ratio(mel32, mel64, scale))


def ratio(mel, mel64, scale):
    err = (mel.double() - mel64).abs()
    r = torch.where(scale > 0, err / scale.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(r.max())


def ulp32(v):
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32)).astype(np.float64))


_REFS = {}


def case_data(i):
    """Waves and float64 reference of case i, computed once and shared."""
    if i not in _REFS:
        x = make_waves(CASES[i][5], 1000 + i)
        _REFS[i] = (x, reference64(CASES[i], x))
    return _REFS[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%d_win%d_mels%d_nw%d_p%d" % (c[0], c[1], c[2], c[3], c[5], c[6]) for c in CASES])
def test_mel_against_float64(i):
    case = CASES[i]
    n_fft, hop, win, n_mels, sr, nw, power, norm, normalize, center = case
    x, ref = case_data(i)
    ms = module(case)
    T = 1 + nw // hop if center else 1 + (nw - n_fft) // hop
    mel = ms.mel(x.to(DEV) if i % 2 else x)                           # waves on the device and on the host
    lg = ms(x.to(DEV) if i % 2 else x)
    assert mel.shape == lg.shape == (3, n_mels, T) == tuple(ref["mel64"].shape) and mel.dtype == lg.dtype == torch.float32 and lg.is_cuda
    mel, lg = mel.cpu(), lg.cpu()
    r_gpu = ratio(mel, ref["mel64"], ref["scale"])
    print(f"\nmel n_fft={n_fft} hop={hop} win={win} n_mels={n_mels} sr={sr} nw={nw} power={power} norm={norm} normalize={normalize} "
          f"center={center}: T={T} r_gpu={r_gpu:.3f} r_cpu32={ref['r_cpu32']:.3f} max mel64={float(ref['mel64'].max()):.3e}")
    assert torch.isfinite(mel).all() and torch.isfinite(lg).all()
    assert r_gpu <= 4.0 * ref["r_cpu32"]
    dmel = (mel.double() - ref["mel64"]).abs()
    bound = dmel / torch.minimum(mel.double().clamp(min=EPS), ref["mel64"].clamp(min=EPS)) + 2.0 * ulp32(ref["log64"])
    dlog = (lg.double() - ref["log64"]).abs()
    worst = float((dlog - bound).max())
    print(f"    log: max |d| = {float(dlog.max()):.3e}, max (|d| - bound) = {worst:.3e}, entries at the floor: {int((ref['mel64'] < EPS).sum())}")
    assert bool((dlog <= bound).all())


@pytest.mark.parametrize("i", [2, 5], ids=["64x16", "1024x256"])
def test_row_of_a_batch_equals_the_single_row_call(i):
    x, _ = case_data(i)
    ms = module(CASES[i])
    full, full_mel = ms(x), ms.mel(x)
    for r in range(3):
        assert torch.equal(ms(x[r:r + 1]), full[r:r + 1]) and torch.equal(ms.mel(x[r:r + 1]), full_mel[r:r + 1])
    assert torch.equal(ms(torch.cat([x, x.flip(0)])), torch.cat([full, full.flip(0)]))


@pytest.mark.parametrize("i,k", [(2, 9), (0, 4), (5, 5), (6, 40)], ids=["64x16_k9", "64x16_k4", "1024x256_k5", "1024x256_k40"])
def test_frames_do_not_depend_on_the_clip_length(i, k):
    """The frames of x[:, :k hop] that the cut does not touch -- those that end at or before sample k hop, t <= k - n_fft / (2 hop) -- equal
    the frames of the whole wave bit for bit: other tiles, another M of the GEMM, another grid."""
    case = CASES[i]
    n_fft, hop = case[0], case[1]
    x, _ = case_data(i)
    ms = module(case)
    assert k * hop < x.shape[1]
    full, cut = ms.mel(x), ms.mel(x[:, :k * hop])
    keep = k - n_fft // (2 * hop) + 1
    assert keep >= 1 and cut.shape[-1] == k + 1
    assert torch.equal(cut[..., :keep], full[..., :keep])
    assert not torch.equal(cut[..., keep:], full[..., keep:k + 1])                 # the reflected end is another signal


def test_two_runs_same_bits_and_channel_axis():
    x, _ = case_data(5)
    ms = module(CASES[5])
    a = ms(x)
    b = ms(x.to(DEV))
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    assert torch.equal(ms(x[:, None, :]), a) and torch.equal(ms.mel(x[:, None, :].to(DEV)), ms.mel(x))
    assert torch.equal(module(CASES[5])(x), a)                                     # another module, other buffers
    with pytest.raises(ValueError):
        ms(x[:, None, None, :])


@pytest.mark.parametrize("i", [1, 3, 5], ids=["64x16_center", "256x64_nocenter", "1024x256_center"])
def test_silence_is_exactly_the_floor(i):
    case = CASES[i]
    ms = module(case)
    out = ms(torch.zeros(2, case[5]))
    floor = np.float32(np.log(np.float64(np.float32(EPS))))                        # the double log of the fp32 floor, rounded once
    assert out.shape[0] == 2 and torch.equal(out.cpu(), torch.full(out.shape, float(floor)))
    assert float(ms.mel(torch.zeros(2, case[5])).abs().max()) == 0.0


@pytest.mark.parametrize("i", [1, 2, 5], ids=["64x16_T3", "64x16_T17", "1024x256_T10"])
def test_nothing_outside_the_output_is_written(i):
    """The destination as a view into a canary-filled buffer, with a row stride and a batch stride of its own."""
    case = CASES[i]
    x, _ = case_data(i)
    ms = module(case)
    want = ms(x)
    b, n_mels, T = want.shape
    buf = torch.full((b + 1, n_mels + 3, T + 7), 12345.0, device=DEV)
    view = buf[:b, 1:1 + n_mels, 3:3 + T]
    got = ms(x, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, want)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:b, 1:1 + n_mels, 3:3 + T] = False
    assert bool((buf[mask] == 12345.0).all())
    with pytest.raises(ValueError, match="out must be"):
        ms(x, out=buf[:b, :n_mels, :T + 1])


@pytest.fixture(scope="module")
def wiring():
    from oracle import e2_cfm_oracle as O
    from v2a_amd import MelSpec
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=16,
                      max_seq_len=256, cond_proj_in=True)
    P = O.init_params(cfg, 78)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=6, piano=True)
    ms = MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=16, device=DEV)
    return dict(cfg=cfg, P=P, y0=y0, text=text, roll=roll, ctx=ctx, cm=cm, ms=ms)


def test_sample_takes_a_raw_wave_prompt_through_melspec(wiring):
    """x3:2157-2160: sample(cond=<raw wave (b, nw)>) == sample(cond=mel_spec(wave).permute(0, 2, 1)), bit for bit, through the
    mel_spec_module argument and through load_mel_spec."""
    from conftest import make_model
    c, ms = wiring, wiring["ms"]
    waves = make_waves(7 * 16 + 9, 31)[:2]                             # 8 mel frames of prompt, 40 frames generated
    kw = dict(y0=c["y0"], text_embed=c["text"], context=c["ctx"], context_mask=c["cm"], frames_embed=c["roll"], lens=torch.tensor([8, 8]),
              duration=torch.tensor([40, 33]), steps=4, cfg_strength=2.0, remove_parallel_component=False, return_raw_output=True)
    latent = ms(waves).permute(0, 2, 1)
    assert latent.shape == (2, 8, 16)
    m = make_model(c["cfg"], c["P"], "fp32", mel_spec_module=ms)
    ref = m.sample(latent, **kw).cpu()
    got = m.sample(waves, **kw).cpu()
    assert got.shape == (2, 40, 16) and torch.equal(got, ref)
    assert torch.equal(got[:, :8], latent.cpu())                       # x3:2260-2261: the prompt frames come back unchanged
    m2 = make_model(c["cfg"], c["P"], "fp32")
    with pytest.raises(NotImplementedError, match="mel_spec_module"):
        m2.sample(waves, **kw)
    built = m2.load_mel_spec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=16)
    assert m2.mel_spec is built and built.dev == m2.device
    assert torch.equal(m2.sample(waves, **kw).cpu(), ref)


def test_forward_val_takes_a_raw_wave_through_melspec(wiring):
    """x3:2328-2331: forward(<raw wave>, val=True, x0=...) == the call on the mel frames, bit for bit."""
    from conftest import make_model
    c, ms = wiring, wiring["ms"]
    waves = make_waves(39 * 16 + 5, 32)[:2]                            # 40 mel frames
    m = make_model(c["cfg"], c["P"], "fp32", audiocond_drop_prob=0.3, mel_spec_module=ms)
    kw = dict(text_embed=c["text"], times=torch.tensor([0.3, 0.8]), lens=torch.tensor([40, 31]), val=True, x0=c["y0"], context=c["ctx"],
              context_mask=c["cm"])
    latent = ms(waves).permute(0, 2, 1)
    assert latent.shape == (2, 40, 16)
    ref, got = m.forward(latent, **kw), m.forward(waves, **kw)
    for a, b in zip((ref.loss, ref.cond, ref.pred_flow, ref.pred_data), (got.loss, got.cond, got.pred_flow, got.pred_data)):
        assert torch.equal(a.cpu(), b.cpu())
    assert torch.isfinite(got.pred_flow).all() and float(got.loss) > 0
