"""CPU: host side of the log-mel front end (v2a_amd.MelSpec, csrc/mel.hip) -- every refusal of the class, the host-side validation of
the two entry points (an error code and a message, no GPU touched), the frame count, `E2TTS.load_mel_spec`, and the exports."""
import ctypes

import pytest
import torch

import v2a_amd
from v2a_amd.mel import MelSpec, mel_filterbank, stft_basis      # fails at import without the feature


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    return _lib


def test_exports():
    assert v2a_amd.MelSpec is MelSpec and v2a_amd.mel_filterbank is mel_filterbank and v2a_amd.stft_basis is stft_basis
    assert "MelSpec" in v2a_amd.__all__
    from v2a_amd import _lib
    for name in ("v2a_mel_pad", "v2a_mel_from_dft"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.lib().v2a_abi_version() == 9


def test_reference_keywords_and_attributes():
    ms = MelSpec(device="cpu")
    assert (ms.n_fft, ms.hop, ms.win_length, ms.n_mel_channels, ms.sampling_rate, ms.normalize, ms.power, ms.norm, ms.center) == \
        (1024, 256, 1024, 100, 24000, False, 1, None, True)
    ms = MelSpec(filter_length=64, hop_length=16, win_length=48, n_mel_channels=10, sampling_rate=16000, normalize=True, power=2, norm="slaney",
                 center=False, device="cpu")
    assert (ms.n_mel_channels, ms.sampling_rate, ms.n_bins, ms.pad) == (10, 16000, 33, 0)


@pytest.mark.parametrize("kw,match", [
    (dict(win_length=1025), "win_length"), (dict(filter_length=64, win_length=65), "win_length"), (dict(win_length=0), "win_length"),
    (dict(hop_length=255), "hop_length"), (dict(hop_length=2), "hop_length"), (dict(hop_length=0), "hop_length"),
    (dict(power=3), "power"), (dict(power=0), "power"), (dict(power=1.5), "power"), (dict(power=None), "power"),
    (dict(norm="htk"), "norm"), (dict(norm=True), "norm"),
    (dict(filter_length=63, win_length=32), "filter_length"), (dict(filter_length=2, win_length=2), "filter_length"),
    (dict(filter_length=4096), "filter_length"), (dict(n_mel_channels=0), "n_mel_channels")])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        MelSpec(device="cpu", **kw)


def test_input_refusals_come_before_any_device_work():
    ms = MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=10, device="cpu")
    for bad in (torch.zeros(100), torch.zeros(2, 2, 100), torch.zeros(2, 1, 1, 100), torch.zeros(0, 100)):
        with pytest.raises(ValueError, match=r"\(b, nw\) or \(b, 1, nw\)"):
            ms(bad)
    with pytest.raises(ValueError, match="floating point"):
        ms(torch.zeros(2, 100, dtype=torch.int16))
    with pytest.raises(ValueError, match="center=True reflects 32"):
        ms(torch.zeros(2, 32))                                         # a reflect pad needs pad < length
    with pytest.raises(ValueError, match="center=True reflects 32"):
        ms.mel(torch.zeros(2, 1, 7))
    nc = MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=10, center=False, device="cpu")
    with pytest.raises(ValueError, match="center=False needs at least"):
        nc(torch.zeros(2, 63))


def test_frame_counts():
    """T = 1 + nw // hop (center=True), 1 + (nw - n_fft) // hop (center=False): torch.stft's own counts."""
    for n_fft, hop, nws in [(64, 16, (33, 47, 48, 101, 257)), (1024, 256, (513, 2400, 24007, 240000)), (256, 64, (1000, 256, 319, 320))]:
        c, nc = MelSpec(n_fft, hop, n_fft, 10, device="cpu"), MelSpec(n_fft, hop, n_fft, 10, center=False, device="cpu")
        w = torch.hann_window(n_fft, periodic=True)
        for nw in nws:
            assert c.frames(nw) == 1 + nw // hop
            if nw <= 24007:
                assert c.frames(nw) == torch.stft(torch.zeros(nw), n_fft, hop, window=w, center=True, return_complex=True).shape[-1]
            if nw >= n_fft:
                assert nc.frames(nw) == 1 + (nw - n_fft) // hop == torch.stft(torch.zeros(nw), n_fft, hop, window=w, center=False,
                                                                                return_complex=True).shape[-1]
    assert MelSpec(device="cpu").frames(240000) == 938


def _pad(L, **kw):
    a = dict(x=4096, ldx=100, B=2, nw=100, pad=32, out=8192, pitch=176)
    a.update(kw)
    return L.v2a_mel_pad(a["x"], a["ldx"], a["B"], a["nw"], a["pad"], a["out"], a["pitch"], None)


def test_mel_pad_validates_on_the_host(lib):
    L = lib.lib()
    for kw, word in [(dict(x=None), "null"), (dict(out=None), "null"), (dict(out=4096), "aliased"), (dict(B=0), "B=0"), (dict(nw=0), "nw=0"),
                     (dict(pad=100), "pad=100"), (dict(pad=-1), "pad=-1"), (dict(ldx=99), "ldx=99"), (dict(pitch=163), "pitch=163"),
                     (dict(x=4098), "alignment")]:
        assert _pad(L, **kw) == -1, kw
        assert word.encode() in L.v2a_last_error(), (kw, L.v2a_last_error())


def _mel(L, table=((0, 2), (1, 3), (30, 3)), **kw):
    host = (ctypes.c_int32 * (2 * len(table)))(*[v for b in table for v in b])
    a = dict(dft=4096, ld_dft=68, rpc=12, n_chunks=1, chunk_stride=0, B=2, T=7, n_fft=64, hop=16, n_mels=len(table), bands_host=ctypes.addressof(host), bands=8192,
             weights=12288, wpitch=3, power=1, eps=1e-5, out=16384, obs=3 * 7, ors=7)
    a.update(kw)
    return L.v2a_mel_from_dft(a["dft"], a["ld_dft"], a["rpc"], a["n_chunks"], a["chunk_stride"], a["B"], a["T"], a["n_fft"], a["hop"], a["n_mels"], a["bands_host"], a["bands"],
                              a["weights"], a["wpitch"], a["power"], a["eps"], a["out"], a["obs"], a["ors"], None)


def test_mel_from_dft_validates_on_the_host(lib):
    L = lib.lib()
    for kw, word in [(dict(dft=None), "null"), (dict(bands_host=None), "null"), (dict(bands=None), "null"), (dict(weights=None), "null"),
                     (dict(out=None), "null"),
                     (dict(n_fft=63), "n_fft=63"), (dict(n_fft=2), "n_fft=2"), (dict(n_fft=4096), "n_fft=4096"),
                     (dict(hop=0), "hop=0"), (dict(hop=18), "hop=18"), (dict(hop=-4), "hop=-4"),
                     (dict(n_mels=0), "n_mels=0"), (dict(power=0), "power=0"), (dict(power=3), "power=3"),
                     (dict(wpitch=0), "wpitch=0"), (dict(wpitch=34), "wpitch=34"),
                     (dict(table=((0, 2), (31, 3))), "band 1"), (dict(table=((-1, 2),)), "band 0"), (dict(table=((0, 4),)), "band 0"),
                     (dict(table=((0, 2), (3, -1))), "band 1"), (dict(table=((33, 1),)), "band 0"),
                     (dict(T=0), "T=0"), (dict(T=13), "rows_per_clip"), (dict(ld_dft=64), "ld_dft=64"), (dict(ld_dft=67), "ld_dft=67"), (dict(B=0), "B=0"),
                     (dict(n_chunks=0), "n_chunks=0"), (dict(n_chunks=17), "n_chunks=17"), (dict(n_chunks=2, chunk_stride=19 * 68 - 2), "chunk_stride"),
                     (dict(n_chunks=2, chunk_stride=19 * 68 + 1), "chunk_stride"), (dict(ors=6), "out_row_stride=6"), (dict(obs=20), "out_batch_stride=20"), (dict(dft=4100), "alignment")]:
        assert _mel(L, **kw) == -1, kw
        assert word.encode() in L.v2a_last_error(), (kw, L.v2a_last_error())
    # empty bands anywhere up to the last bin pass the band check: the refusal is the next one (nothing is ever launched from here)
    assert _mel(L, table=((33, 0), (0, 0), (30, 3)), T=0) == -1 and b"T=0" in L.v2a_last_error()


def _small_model(**kw):
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          max_seq_len=256, if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=True, device="cpu", **kw)


def test_load_mel_spec():
    m = _small_model()
    assert m.mel_spec is None
    with pytest.raises(ValueError, match="n_mel_channels=100 but the model has num_channels=16"):
        m.load_mel_spec()
    with pytest.raises(ValueError, match="n_mel_channels=10"):
        m.load_mel_spec(MelSpec(64, 16, 64, 10, device="cpu"))
    assert m.mel_spec is None
    with pytest.raises(TypeError):
        m.load_mel_spec(lambda w: w)
    with pytest.raises(ValueError, match="hop_length"):
        m.load_mel_spec(filter_length=64, hop_length=10, win_length=64, n_mel_channels=16)
    ms = m.load_mel_spec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=16)
    assert isinstance(ms, MelSpec) and m.mel_spec is ms and ms.dev == m.device and (ms.n_fft, ms.hop) == (64, 16)
    mine = MelSpec(64, 16, 48, 16, device="cpu")
    assert m.load_mel_spec(mine) is mine and m.mel_spec is mine
    assert _small_model(mel_spec_module=mine).mel_spec is mine           # the constructor argument, as before
    with pytest.raises(ValueError, match="center=True reflects"):       # a raw wave reaches the module: its refusal comes back
        m.sample(torch.zeros(2, 20))
