"""GPU: the wave front end (v2a_amd.WaveFrontEnd, csrc/wave.hip) and what is built on it (E2TTS.encode_audio, CLI --wav).

Resampler: against a float64 `conv1d` with the same fp32-rounded table, so that the kernel alone is measured.  The bar is not a
measurement: for every output, |y_j - ref_j| <= (K + 1) * 2^-24 * sum_k |xpad[q o + k] * table[p][k]|, the a-priori bound of a K-term
fp32 sum taken in any order, evaluated by the test in float64 from the inputs.
Normalise: bit for bit against torch's CPU fp32 `(x - m) / (peak + 1e-8) * 0.5` with m = fl32(float64 mean); the waves are chosen so
that the float64 mean lies further than 1e-6 of an fp32 spacing from a rounding boundary, which the test asserts first.
torchaudio is not installed where these tests were written: the references are float64 evaluations of the restatement in
tests/test_wave_front_end_host.py."""
import ctypes
import dataclasses
import json
import math
import sys
import types

import numpy as np
import pytest
import torch

import v2a_amd
from v2a_amd import _lib as L
from v2a_amd.synth import random_encodec_decoder_state_dict, random_encodec_encoder_state_dict, synthetic_wave
from v2a_amd.wave import MAX_PARTS, resampled_length, sinc_resample_table
from test_wave_front_end_host import RATES, resample64, resample_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
FULL = {44100: 441000, 22050: 220500}                              # the 10 s clips


@pytest.fixture(scope="module")
def fe():
    return v2a_amd.WaveFrontEnd(DEV)


def lengths(rate, o):
    return sorted({v for v in (1, 37, o - 1, o, o + 1, 10 * o + 13) if v >= 1}) + ([FULL[rate]] if rate in FULL else [])


def raw_resample(x, table, width, o, n, slack=64):
    """One v2a_wave_resample launch into a NaN-filled destination of out_len + slack samples -> (destination, out_len, parts, n_parts)."""
    out_len = resampled_length(x.shape[0], o, n)
    y = torch.full((out_len + slack,), float("nan"), device=DEV)
    parts = torch.full((MAX_PARTS * 2,), float("nan"), dtype=torch.float64, device=DEV)
    n_parts = ctypes.c_int32(0)
    L.check(L.lib().v2a_wave_resample(x.data_ptr(), x.shape[0], table.data_ptr(), o, n, table.shape[1], width, y.data_ptr(), out_len,
                                      parts.data_ptr(), ctypes.byref(n_parts), L.stream_ptr()))
    return y, out_len, parts, n_parts.value


def bits(t):
    return t.cpu().view(torch.int32)


# ---- resampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_resampler_against_float64_within_the_summation_bound(fe, rate):
    table, width, o, n = sinc_resample_table(rate, 24000)
    K = table.shape[1]
    tdev = fe.table(rate)[0]
    assert torch.equal(tdev.cpu(), table)
    worst = 0.0
    for i, length in enumerate(lengths(rate, o)):
        x = synthetic_wave(length, 100 + i, rate)
        y, out_len, parts, n_parts = raw_resample(x.to(DEV), tdev, width, o, n)
        y = y.cpu()
        assert out_len == math.ceil(n * length / o)
        assert bool(torch.isnan(y[out_len:]).all()) and not bool(torch.isnan(y[:out_len]).any())      # nothing past the end, all before it
        ref, scale = resample64(x, table, width, o, n), resample_bound(x, table, width, o, n)
        bound = (K + 1) * U * scale
        err = (y[:out_len].double() - ref).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (rate, length, ratio)
        # the public call gives the same bits, and the partials hold the sum, minimum and maximum of this output
        got = fe.resample(x, rate)
        assert got.shape == (out_len,) and got.device.type == "cuda" and torch.equal(bits(got), bits(y[:out_len]))
        p = parts.cpu()[:2 * n_parts]
        mnmx = p.view(torch.float32).view(-1, 4)[:, 2:]
        assert 1 <= n_parts <= MAX_PARTS and float(mnmx[:, 0].min()) == float(y[:out_len].min()) and float(mnmx[:, 1].max()) == float(y[:out_len].max())
        assert abs(float(p[0::2].sum()) - float(y[:out_len].double().sum())) <= 1e-12 * float(y[:out_len].double().abs().sum()) + 1e-300
    print(f"resample {rate} Hz -> 24000 Hz ({n} x {K} table): worst |y - ref64| / ((K + 1) 2^-24 sum |x t|) = {worst:.4f}")


@pytest.mark.parametrize("rate,length", [(44100, 441000), (11025, 110250), (48000, 30001)])
def test_a_sample_does_not_depend_on_the_tiling(fe, rate, length):
    """The same samples as the prefix of a wave twice as long (twice the tiles: past V2A_WAVE_MAX_PARTS workgroups loop), and the same
    samples o later (every output n further, in another tile at another place): bit-equal wherever the window holds the same data.
    44 100 Hz: table in LDS; 11 025 Hz: table read from global memory."""
    table, width, o, n = fe.table(rate)
    a = synthetic_wave(length, 7, rate)
    b = torch.cat([a, synthetic_wave(length, 8, rate)])
    ya, yb = fe.resample(a, rate), fe.resample(b, rate)
    # output j = q n + p reads x[q o - width .. q o + width + o - 1]: inside the prefix while q o + width + o - 1 <= length - 1
    q_ok = (length - width - o) // o
    shared = (q_ok + 1) * n
    assert 0.99 * ya.shape[0] < shared <= ya.shape[0] and yb.shape[0] > 1.99 * shared
    assert torch.equal(bits(ya[:shared]), bits(yb[:shared]))
    assert not torch.equal(bits(ya[shared:]), bits(yb[shared:ya.shape[0]]))                      # behind it the longer wave has data
    ys = fe.resample(a[o:], rate)                                                               # q' = q - 1
    q_first = -(-width // o)                                                                    # windows of the shifted wave without front padding
    assert torch.equal(bits(ys[q_first * n:shared - n]), bits(ya[(q_first + 1) * n:shared]))


def test_two_runs_give_the_same_bits(fe):
    for rate in (44100, 11025, 24000):
        x = synthetic_wave(50001, 3, rate)
        outs = []
        for _ in range(2):
            outs.append((bits(fe(x, rate)), fe.last_stats))
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and all(math.isfinite(v) for v in outs[0][1])


# ---- normalise -----------------------------------------------------------------------------------------------------------
def mean32_checked(x):
    """fl32 of the exact mean of x, after asserting that the mean is further than 1e-6 fp32 spacings from a rounding boundary."""
    m64 = math.fsum(x.double().tolist()) / x.shape[0]
    m32 = np.float32(m64)
    lo, hi = np.nextafter(m32, np.float32(-np.inf)), np.nextafter(m32, np.float32(np.inf))
    spacing = min(float(hi) - float(m32), float(m32) - float(lo))
    dist = min(abs(m64 - (float(lo) + float(m32)) / 2), abs(m64 - (float(hi) + float(m32)) / 2))
    assert dist > 1e-6 * spacing, f"precondition: the float64 mean {m64!r} is {dist / spacing:.2e} spacings from a rounding boundary; take another seed"
    return torch.tensor(m32)


def normalize_cpu(x, n_out=None):
    """(out, m, peak): torch's CPU fp32 `normalize_wav` with m = fl32(float64 mean), cut or zero-padded to n_out."""
    m = mean32_checked(x)
    xm = x - m
    peak = xm.abs().max()
    out = xm / (peak + 1e-8) * 0.5
    n_out = x.shape[0] if n_out is None else n_out
    return torch.nn.functional.pad(out[:n_out], (0, max(0, n_out - x.shape[0]))), float(m), float(peak)


WAVES = {
    "one sample": lambda: synthetic_wave(1, 11),
    "37 samples": lambda: synthetic_wave(37, 12),
    "5 000 samples": lambda: synthetic_wave(5000, 13),
    "10 s": lambda: synthetic_wave(240000, 14),
    "past 256 partials": lambda: synthetic_wave(600001, 15),
    "DC offset": lambda: 0.5 * synthetic_wave(24000, 16) + 0.3,
    "negative peak": lambda: -synthetic_wave(24001, 17).abs() * 0.7,
}


@pytest.mark.parametrize("name", list(WAVES))
def test_normalize_equals_the_cpu_fp32_evaluation_bit_for_bit(fe, name):
    x = WAVES[name]()
    if name == "DC offset":
        assert abs(float(x.double().mean()) - 0.3) < 0.02
    n = x.shape[0]
    for n_out in (None, max(1, n // 2), n, n + 77):
        want, m, peak = normalize_cpu(x, n_out)
        got = fe.normalize(x, n_out=n_out)
        assert got.shape == want.shape and got.dtype == torch.float32 and got.device.type == "cuda"
        assert fe.last_stats == (m, peak), (fe.last_stats, (m, peak))
        assert torch.equal(bits(got), bits(want))
    # a NaN-filled destination with room behind n_out: nothing is written there
    xd = x.to(DEV)
    parts, n_parts = torch.empty(MAX_PARTS * 2, dtype=torch.float64, device=DEV), ctypes.c_int32(0)
    L.check(L.lib().v2a_wave_stats(xd.data_ptr(), n, parts.data_ptr(), ctypes.byref(n_parts), L.stream_ptr()))
    assert n_parts.value == min(MAX_PARTS, -(-n // 2048))
    dst, stats = torch.full((n + 100,), float("nan"), device=DEV), torch.empty(2, device=DEV)
    L.check(L.lib().v2a_wave_normalize(xd.data_ptr(), n, parts.data_ptr(), n_parts.value, dst.data_ptr(), n + 50, stats.data_ptr(), L.stream_ptr()))
    want, m, peak = normalize_cpu(x, n + 50)
    assert torch.equal(bits(dst[:n + 50]), bits(want)) and bool(torch.isnan(dst[n + 50:]).all()) and stats.tolist() == [m, peak]
    print(f"normalize [{name}]: n = {n}, m = {m:.9e}, peak = {peak:.9e}, {n_parts.value} partials: bit-equal to the CPU fp32 evaluation")


def test_normalize_of_silence_is_silence(fe):
    for n, n_out in ((1, None), (5000, None), (5000, 6000), (5000, 100)):
        got = fe.normalize(torch.zeros(n), n_out=n_out).cpu()
        assert got.shape == (n if n_out is None else n_out,) and not bool(torch.isnan(got).any()) and bool((got == 0).all())
        assert fe.last_stats == (0.0, 0.0)


def test_target_rate_skips_the_resampler(fe):
    """orig_freq == 24 000: without normalize the wave comes back bit for bit; with it the stats kernel feeds the same normalisation."""
    stereo = torch.stack([synthetic_wave(30011, 21), synthetic_wave(30011, 22)])
    x = stereo[0]
    assert torch.equal(bits(fe(stereo, 24000, normalize=False)), bits(x)) and torch.equal(bits(fe.resample(x, 24000)), bits(x))
    assert torch.equal(bits(fe(x, 24000, normalize=False, max_samples=6400)), bits(x[:6400]))
    want, m, peak = normalize_cpu(x)
    assert torch.equal(bits(fe(stereo, 24000)), bits(want)) and fe.last_stats == (m, peak)
    assert torch.equal(bits(fe(x, 24000, max_samples=6400)), bits(want[:6400])) and fe.last_stats == (m, peak)
    assert torch.equal(bits(fe(x, 24000, max_samples=10 ** 9)), bits(want))


@pytest.mark.parametrize("rate", [44100, 11025, 48000])
def test_resampled_wave_is_normalised_from_the_partials_of_the_same_launch(fe, rate):
    """__call__ = resample, then normalize on the partials the resampler wrote: equal to normalising the resampled wave on the CPU."""
    x = synthetic_wave(rate + 17, 31, rate) * 0.6 + 0.05
    y = fe.resample(x, rate).cpu()
    want, m, peak = normalize_cpu(y)
    got = fe(x, rate)
    assert torch.equal(bits(got), bits(want)) and fe.last_stats == (m, peak)
    assert torch.equal(bits(fe(x, rate, max_samples=6400)), bits(want[:6400])) and fe.last_stats == (m, peak)      # the whole wave's statistics
    assert torch.equal(bits(fe(x, rate, normalize=False)), bits(y))


# ---- composition ----------------------------------------------------------------------------------------------------------
def _audio_model(**kw):
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          max_seq_len=256, if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=128, sampling_rate=24000, device="cuda:0", **kw)


def test_encode_audio_is_the_front_end_then_the_encoder(fe):
    m = _audio_model()
    enc = m.load_audio_encoder(random_encodec_encoder_state_dict(1))
    waves = [torch.stack([synthetic_wave(30000, 41, 44100), synthetic_wave(30000, 42, 44100)]), synthetic_wave(9000, 43, 22050),
             synthetic_wave(5000, 44, 24000)]
    rates = [44100, 22050, 24000]
    fronts = [fe(w, r) for w, r in zip(waves, rates)]
    assert [f.shape[0] for f in fronts] == [16327, 9796, 5000]
    want = [z.clone() for z in enc.encode_list(fronts)]
    lat, lens = m.encode_audio(waves, rates)
    assert lens.tolist() == [52, 31, 16] and lens.dtype == torch.long and lat.shape == (3, 52, 128) and lat.device.type == "cuda"
    for i, z in enumerate(want):
        assert torch.equal(bits(lat[i, :lens[i]]), bits(z.t().contiguous())) and bool((lat[i, lens[i]:] == 0).all())
    # max_frames: cut at max_frames * 320 samples of the normalised wave, before the encoder
    want = [z.clone() for z in enc.encode_list([f[:20 * 320] for f in fronts])]
    lat, lens = m.encode_audio(waves, rates, max_frames=20)
    assert lens.tolist() == [20, 20, 16] and lat.shape == (3, 20, 128)
    for i, z in enumerate(want):
        assert torch.equal(bits(lat[i, :lens[i]]), bits(z.t().contiguous())) and bool((lat[i, lens[i]:] == 0).all())
    # normalize=False: the resampled wave as it is; one rate for all
    raw = [fe(w, 44100, normalize=False) for w in waves[:2]]
    want = [z.clone() for z in enc.encode_list(raw)]
    lat, lens = m.encode_audio(waves[:2], 44100, normalize=False)
    assert lens.tolist() == [z.shape[1] for z in want]
    for i, z in enumerate(want):
        assert torch.equal(bits(lat[i, :lens[i]]), bits(z.t().contiguous()))


def test_cli_validate_from_wav_equals_validate_from_the_latents(tmp_path, small, capsys, monkeypatch):
    """CLI --validate --wav --encodec with `<video>.wav` at 44 100 Hz (read through a fake soundfile) prints the JSON that --validate
    prints from the `.latent.npy` written from `encode_audio` of the same waves; an existing `.latent.npy` wins over the `.wav`."""
    from test_validation_gpu import _model, build_cases                 # the tiny model of the validation tests, by import only
    from v2a_amd import cli
    c = build_cases(dict(small, cfg=dataclasses.replace(small["cfg"], num_channels=128)))["plain"]
    cfg = c["cfg"]
    ck, es = tmp_path / "small.pt", tmp_path / "encodec.pt"
    torch.save({"model_state_dict": c["P"]}, ck)
    esd = {"encoder." + k: v for k, v in random_encodec_encoder_state_dict(2).items()}
    esd.update({"decoder." + k: v for k, v in random_encodec_decoder_state_dict(2).items()})
    torch.save(esd, es)
    waves = {}
    g = torch.Generator().manual_seed(5)
    dirs = {}
    for tag in ("wav", "lat"):
        (tmp_path / tag).mkdir()
        vids = [str(tmp_path / tag / f"clip{i}.mp4") for i in range(3)]
        dirs[tag] = vids
        (tmp_path / tag / "list.scp").write_text("".join(f"{v}\tsound {i}\n" for i, v in enumerate(vids)))
    for i in range(3):
        emb, t5 = torch.randn(13 + i, cfg.dim_text, generator=g), (0.2 * torch.randn(4 + i, cfg.dim, generator=g)).numpy()
        stereo = np.stack([synthetic_wave(20000 + 3000 * i, 50 + i, 44100).numpy(), synthetic_wave(20000 + 3000 * i, 60 + i, 44100).numpy()], 1)
        for tag in ("wav", "lat"):
            v = dirs[tag][i]
            v2a_amd.save_clip_cache(v2a_amd.feature_cache_path(v), emb, 0.5 + 0.01 * i)              # 37, 38, 38 frames
            np.savez(v.replace(".mp4", ".t5.npz"), t5)
        waves[dirs["wav"][i].replace(".mp4", ".wav")] = stereo
        open(dirs["wav"][i].replace(".mp4", ".wav"), "wb").close()
    monkeypatch.setitem(sys.modules, "torchaudio", None)
    monkeypatch.setitem(sys.modules, "soundfile", types.SimpleNamespace(read=lambda path, dtype, always_2d: (waves[path], 44100)))
    mc = dict(dim=cfg.dim, dim_text=cfg.dim_text, dim_frames=cfg.dim_frames, depth=cfg.depth, heads=cfg.heads, dim_head=cfg.dim_head,
              frames_heads=cfg.frames_heads, num_registers=cfg.num_registers, max_seq_len=cfg.max_seq_len, num_channels=cfg.num_channels)

    def run(tag, *flags):
        written = cli.main([str(ck), "0", str(tmp_path / tag / "list.scp"), "0", "3", str(tmp_path / "out"), "--batch", "2", "--frames", "40",
                            "--dtype", "fp32", "--model-config", json.dumps(mc), "--validate", *flags])
        assert written == []
        return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]

    # the latents of the same waves, written next to the second set of videos: encode_audio cut at each batch's n frames
    m = _model(c, "fp32")
    m.load_audio_encoder(esd)
    for b0 in (0, 2):
        reqs = cli.build_requests(cli.read_scp(str(tmp_path / "lat" / "list.scp"), b0, b0 + 2), False, 40)
        n = v2a_amd.collate_clips(reqs, cfg.num_channels)[1]["text_embed"].shape[1]
        for i in range(b0, min(b0 + 2, 3)):
            z, zl = m.encode_audio([torch.from_numpy(waves[dirs["wav"][i].replace(".mp4", ".wav")][:, 0].copy())], [44100], max_frames=n)
            assert 20 <= int(zl[0]) <= n
            np.save(dirs["lat"][i].replace(".mp4", ".latent.npy"), z[0, :int(zl[0])].cpu().numpy())
    from_wav = run("wav", "--wav", "--encodec", str(es))
    from_lat = run("lat")
    assert len(from_wav) == 2 and from_wav == from_lat and json.loads(from_wav[0])["loss"] > 0
    # an existing .latent.npy wins: other latents next to clip0 change the first line, and only the first
    np.save(dirs["wav"][0].replace(".mp4", ".latent.npy"), torch.randn(30, cfg.num_channels, generator=g).numpy())
    again = run("wav", "--wav", "--encodec", str(es))
    assert again[0] != from_wav[0] and again[1] == from_wav[1]
    with pytest.raises(FileNotFoundError):                              # without --wav the .wav is not looked at
        run("wav")
