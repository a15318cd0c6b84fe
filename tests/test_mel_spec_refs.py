"""CPU: what pins the two host tables of the log-mel front end (v2a_amd/mel.py) without torchaudio.

* `mel_filterbank` (torchaudio's `melscale_fbanks`, HTK scale) against `transformers.audio_utils.mel_filter_bank(norm=None | "slaney",
  mel_scale="htk")`: exactly for the default setting (513 bins, 100 channels, 24 kHz) and the small one of the GPU tests (33, 10,
  24 kHz), to 1e-12 elsewhere.
* `stft_basis`: the framed evaluation -- reflect pad, unfold, float64 matmul with the basis -- against `torch.stft` in float64, to 1e-9
  of the largest value, with win_length < n_fft, normalize=True and center=False among the cases.
* `transformers.audio_utils.spectrogram` with the same window and filterbank against fb.T @ |S|**power from `torch.stft`, to 1e-6 of
  the largest value (it runs numpy's FFT in float64 and returns fp64 here; measured 1.1e-8).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from v2a_amd.mel import MelSpec, filterbank_bands, mel_filterbank, stft_basis, stft_window      # fails at import without the feature


def stft64(x, n_fft, hop, win, normalize, center):
    """torch.stft in float64 as torchaudio's Spectrogram calls it -> complex (b, n_fft / 2 + 1, T)."""
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    S = torch.stft(x.double(), n_fft, hop, win, window=w, center=center, pad_mode="reflect", return_complex=True)
    return S / w.pow(2).sum().sqrt() if normalize else S


def frames64(x, n_fft, hop, center):
    """(b, nw) -> (b, T, n_fft) float64 frames as torch.stft cuts them."""
    x = x.double()
    if center:
        x = F.pad(x[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    return x.unfold(1, n_fft, hop)


@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("n_freqs,n_mels,sr,exact", [(513, 100, 24000, True), (33, 10, 24000, True), (33, 10, 16000, False),
                                                     (129, 40, 24000, False), (1025, 128, 44100, False), (201, 80, 22050, False)])
def test_filterbank_equals_transformers(n_freqs, n_mels, sr, exact, norm):
    au = pytest.importorskip("transformers.audio_utils")
    ref = torch.from_numpy(au.mel_filter_bank(n_freqs, n_mels, 0.0, float(sr // 2), sr, norm=norm, mel_scale="htk"))
    fb = mel_filterbank(n_freqs, n_mels, sr, norm=norm)
    assert fb.dtype == torch.float64 and fb.shape == ref.shape == (n_freqs, n_mels)
    d = float((fb - ref).abs().max())
    print(f"mel_filterbank({n_freqs}, {n_mels}, {sr}, norm={norm}): max |d| vs transformers = {d:.3e}")
    assert d == 0.0 if exact else d <= 1e-12
    assert float(fb.min()) >= 0.0 and float(fb.max()) > 0.0


def test_filterbank_band_form_is_the_filterbank():
    """Every filter has one contiguous support; (first, count, weights) rebuilds the fp32 table exactly, empty filters included."""
    for n_freqs, n_mels, sr in [(513, 100, 24000), (33, 10, 24000), (33, 40, 24000)]:       # the last has filters without a bin
        fb = mel_filterbank(n_freqs, n_mels, sr).float()
        bands, weights = filterbank_bands(fb)
        assert bands.dtype == torch.int32 and bands.shape == (n_mels, 2) and weights.shape == (n_mels, max(1, int(bands[:, 1].max())))
        back = torch.zeros_like(fb)
        for m in range(n_mels):
            first, count = int(bands[m, 0]), int(bands[m, 1])
            assert 0 <= first and first + count <= n_freqs
            back[first:first + count, m] = weights[m, :count]
            assert float(weights[m, count:].abs().sum()) == 0.0
        assert torch.equal(back, fb)
    assert int((bands[:, 1] == 0).sum()) > 0


def test_window_is_centred_as_torch_stft_centres_it():
    w = stft_window(64, 48)
    assert torch.equal(w[8:56], torch.hann_window(48, periodic=True, dtype=torch.float64)) and float(w[:8].abs().sum() + w[56:].abs().sum()) == 0.0
    assert torch.equal(stft_window(64, 64), torch.hann_window(64, periodic=True, dtype=torch.float64))


@pytest.mark.parametrize("n_fft,hop,win,normalize,center,nw", [
    (64, 16, 64, False, True, 101), (64, 16, 48, True, True, 257), (64, 16, 48, False, False, 257), (256, 64, 200, False, False, 1000),
    (256, 64, 200, True, True, 1000), (1024, 256, 1024, False, True, 2400), (1024, 256, 600, True, False, 2400)])
def test_framed_basis_equals_torch_stft(n_fft, hop, win, normalize, center, nw):
    x = torch.randn(3, nw, generator=torch.Generator().manual_seed(nw + n_fft), dtype=torch.float64)
    S = stft64(x, n_fft, hop, win, normalize, center)
    basis = stft_basis(n_fft, win, normalize)
    nb = n_fft // 2 + 1
    assert basis.dtype == torch.float64 and basis.shape == (2 * nb, n_fft)
    Y = frames64(x, n_fft, hop, center) @ basis.T                     # (b, T, re | im)
    got = torch.complex(Y[..., :nb], Y[..., nb:]).permute(0, 2, 1)
    assert got.shape == S.shape
    d = float((got - S).abs().max() / S.abs().max())
    print(f"framed basis n_fft={n_fft} hop={hop} win={win} normalize={normalize} center={center}: max |d| / max |S| = {d:.3e}")
    assert d <= 1e-9


@pytest.mark.parametrize("n_fft,hop,win,n_mels,sr,nw,power,norm", [(1024, 256, 1024, 100, 24000, 2400, 1, None), (64, 16, 48, 10, 16000, 257, 2, "slaney"),
                                                                   (256, 64, 200, 40, 24000, 1000, 2, None)])
def test_transformers_spectrogram_agrees(n_fft, hop, win, n_mels, sr, nw, power, norm):
    au = pytest.importorskip("transformers.audio_utils")
    x = torch.randn(nw, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    fb = mel_filterbank(n_fft // 2 + 1, n_mels, sr, norm=norm)
    mel64 = fb.T @ stft64(x[None], n_fft, hop, win, False, True)[0].abs() ** power
    # transformers pads the window itself when frame_length < fft_length -- on the right, not centred -- so it gets torch's centred one
    got = au.spectrogram(x.numpy(), stft_window(n_fft, win).numpy(), frame_length=n_fft, hop_length=hop, fft_length=n_fft, power=float(power),
                         center=True, pad_mode="reflect", mel_filters=fb.numpy(), mel_floor=0.0, dtype=np.float64)
    got = torch.from_numpy(np.asarray(got, dtype=np.float64))
    assert got.shape == mel64.shape
    d = float((got - mel64).abs().max() / mel64.abs().max())
    print(f"transformers.spectrogram n_fft={n_fft} power={power}: max |d| / max = {d:.3e}")
    assert d <= 1e-6


def test_device_tables_are_the_float64_tables_rounded_once():
    """host_tables(): re of bin k in row 2k, im in row 2k + 1, zero rows and zero columns up to the GEMM's alignment; the band weights are the
    fp32 rounding of the float64 filterbank."""
    ms = MelSpec(filter_length=72, hop_length=12, win_length=60, n_mel_channels=9, sampling_rate=16000, normalize=True, norm="slaney", device="cpu")
    basis, bands, weights = ms.host_tables()
    nb = 37
    assert (ms.n_bins, ms.k_pad, ms.n_pad) == (nb, 80, 76) and basis.shape == (76, 80) and basis.dtype == torch.float32
    b64 = stft_basis(72, 60, True)
    assert torch.equal(basis[0:2 * nb:2, :72], b64[:nb].float()) and torch.equal(basis[1:2 * nb:2, :72], b64[nb:].float())
    assert float(basis[:, 72:].abs().sum()) == 0.0 and float(basis[2 * nb:].abs().sum()) == 0.0
    fb = mel_filterbank(nb, 9, 16000, norm="slaney").float()
    for m in range(9):
        first, count = int(bands[m, 0]), int(bands[m, 1])
        assert torch.equal(weights[m, :count], fb[first:first + count, m])
