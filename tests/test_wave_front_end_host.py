"""CPU: host side of the wave front end (v2a_amd.WaveFrontEnd, csrc/wave.hip) -- the filter table against a float64 restatement of
torchaudio's `sinc_interp_hann` kernel written here, that restatement against an analytic sine (an anchor that shares no formula
with it), the table cap, the three C-ABI symbols and their argument checks, the `--wav` rules of the CLI and the source selection
of `--validate`.

torchaudio is not installed where these tests were written, so no vector of the library pins the resampler: `table64` below is
the library's published algorithm restated, and everything is measured against float64 evaluations of it."""
import ctypes
import glob
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from v2a_amd.wave import WaveFrontEnd, resample_geometry, resampled_length, sinc_resample_table, table_in_lds      # fails at import without the feature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 44100, 32000, 22050, 16000, 11025, 8000)
# (o, n, width, K) at new_freq = 24 000, lowpass_filter_width = 6, rolloff = 0.99, by hand from the formula
GEOMETRY = {48000: (2, 1, 13, 28), 44100: (147, 80, 12, 171), 32000: (4, 3, 9, 22), 22050: (147, 160, 7, 161), 16000: (2, 3, 7, 16),
            11025: (147, 320, 7, 161), 8000: (1, 3, 7, 15)}


def table64(orig_freq, new_freq=24000, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio `_get_sinc_resample_kernel(..., resampling_method="sinc_interp_hann")` in float64 -> (kernel (n, K), width, o, n)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base_freq)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels *= window * scale
    return kernels[:, 0], width, o, n


def resample64(x, table, width, o, n):
    """torchaudio `_apply_sinc_resample_kernel` in float64 on a 1-D wave: pad, conv1d of stride o, phases interleaved, cut."""
    L = x.shape[0]
    xp = F.pad(x.double()[None, None], (width, width + o))
    y = F.conv1d(xp, table.double()[:, None, :], stride=o)                 # (1, n, q)
    return y[0].t().reshape(-1)[:-(-n * L // o)]


def resample_bound(x, table, width, o, n):
    """sum_k |xpad[q o + k] * table[p][k]| per output, in float64: the scale of the a-priori error bound of a K-term fp32 sum."""
    return resample64(x.abs(), table.abs(), width, o, n)


@pytest.mark.parametrize("rate", RATES)
def test_table_against_the_float64_restatement(rate):
    table, width, o, n = sinc_resample_table(rate, 24000)
    ref, rwidth, ro, rn = table64(rate)
    assert (o, n, width, table.shape[1]) == GEOMETRY[rate] == resample_geometry(rate, 24000)
    assert (width, o, n) == (rwidth, ro, rn) and table.dtype == torch.float32 and tuple(table.shape) == tuple(ref.shape) == (n, 2 * width + o)
    ref32 = ref.float()
    ulp = torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))) - ref32.abs()
    over = float(((table - ref32).abs() / ulp).max())
    print(f"{rate} Hz: table ({n}, {table.shape[1]}), max |table - fl32(table64)| = {over:.2f} fp32 spacings")
    assert over <= 1.0
    for L in (1, 37, o - 1, o, o + 1, 10 * o + 13):
        if L >= 1:
            assert resampled_length(L, o, n) == math.ceil(n * L / o) == resample64(torch.zeros(L), ref, width, o, n).shape[0]


@pytest.mark.parametrize("rate", [44100, 22050, 11025, 8000])
def test_restatement_resamples_a_sine_to_the_analytic_sine(rate):
    """A 440 Hz unit sine of 1 s: the float64 restatement against sin(2 pi 440 j / 24000), 200 samples away from both ends.  A phase
    sign or a stride that the restatement and the implementation got wrong together would show here (they share the formula)."""
    ref, width, o, n = table64(rate)
    x = torch.sin(2 * math.pi * 440.0 * torch.arange(rate, dtype=torch.float64) / rate)
    y = resample64(x, ref, width, o, n)
    assert y.shape[0] == 24000
    want = torch.sin(2 * math.pi * 440.0 * torch.arange(24000, dtype=torch.float64) / 24000)
    err = float((y - want)[200:-200].abs().max())
    # the same through the implementation's table: the indexing the kernel uses, y[q n + p] = sum_k xpad[q o + k] table[p][k]
    table = sinc_resample_table(rate, 24000)[0].double()
    xp = F.pad(x, (width, width + o))
    j = torch.arange(200, 24000 - 200)
    win = xp[((j // n) * o)[:, None] + torch.arange(table.shape[1])[None, :]]
    err_impl = float(((win * table[j % n]).sum(1) - want[200:-200]).abs().max())
    print(f"{rate} Hz: 440 Hz sine, max |resampled - analytic| = {err:.2e} (restatement), {err_impl:.2e} (sinc_resample_table, indexed by hand)")
    assert err <= 1e-3 and err_impl <= 1e-3


def test_both_table_paths_are_reached_by_the_tested_rates():
    """48 / 44.1 / 22.05 kHz tables (112 B, 53 KB, 101 KB) sit in LDS beside the window; 11.025 kHz (201 KB) is read from global memory."""
    lds = {r: table_in_lds(*[GEOMETRY[r][i] for i in (0, 1, 3)]) for r in RATES}
    assert lds == {48000: True, 44100: True, 32000: True, 22050: True, 16000: True, 11025: False, 8000: True}


def test_table_cap_raises_before_anything_is_allocated_or_launched(monkeypatch):
    from v2a_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(ValueError, match=r"44101 Hz -> 24000 Hz"):
        sinc_resample_table(44101, 24000)
    fe = WaveFrontEnd("cpu")
    not_a_wave = object()                                          # torch.as_tensor(object()) raises another error: never reached
    for call in (lambda: fe.resample(not_a_wave, 44101), lambda: fe(not_a_wave, 44101), lambda: fe.table(44101)):
        with pytest.raises(ValueError, match=r"44101 Hz -> 24000 Hz"):
            call()
    assert fe._tables == {}
    with pytest.raises(ValueError, match="positive"):
        sinc_resample_table(0, 24000)


def test_new_symbols_are_declared_exported_and_check_arguments():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ("v2a_wave_resample", "v2a_wave_stats", "v2a_wave_normalize"):
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 9 and _lib.lib().v2a_abi_version() == 9
    L = _lib.lib()
    np_ = ctypes.c_int32(0)
    ok = dict(x=4096, L=1000, table=8192, o=147, n=80, K=171, width=12, y=16384, out_len=545, parts=32768)

    def resample(**kw):
        a = dict(ok, **kw)
        return L.v2a_wave_resample(a["x"], a["L"], a["table"], a["o"], a["n"], a["K"], a["width"], a["y"], a["out_len"], a["parts"],
                                   ctypes.byref(np_), None)
    assert resample(x=None) == -1 and b"null" in L.v2a_last_error()
    assert resample(K=170) == -1 and b"K=170" in L.v2a_last_error()                       # K != 2 width + o
    assert resample(out_len=544) == -1 and b"out_len=544" in L.v2a_last_error()           # ceil(80 * 1000 / 147) = 545
    assert resample(out_len=546) == -1 and b"out_len=546" in L.v2a_last_error()
    assert resample(L=0, out_len=0) == -1 and b"L=0" in L.v2a_last_error()
    assert resample(o=9000, K=9024, n=1, out_len=1) == -1 and b"K=9024" in L.v2a_last_error()      # past the LDS window
    assert resample(y=16386) == -1 and b"alignment" in L.v2a_last_error()
    assert L.v2a_wave_stats(None, 10, 32768, ctypes.byref(np_), None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_wave_stats(4096, 0, 32768, ctypes.byref(np_), None) == -1 and b"n=0" in L.v2a_last_error()
    assert L.v2a_wave_normalize(4096, 10, 32768, 1, None, 10, 65536, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_wave_normalize(4096, 10, 32768, 0, 16384, 10, 65536, None) == -1 and b"n_parts=0" in L.v2a_last_error()
    assert L.v2a_wave_normalize(4096, 10, 32768, 257, 16384, 10, 65536, None) == -1 and b"n_parts=257" in L.v2a_last_error()
    assert L.v2a_wave_normalize(4096, 10, 32768, 1, 16384, 0, 65536, None) == -1 and b"n_out=0" in L.v2a_last_error()
    assert np_.value == 0                                                                 # nothing was launched, nothing reported


def test_wave_device_assembly_has_no_scratch():
    """The rule of test_isa_guard.py (whose source list is fixed) for csrc/wave.hip: four kernels, no spill, no scratch."""
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    paths = glob.glob(os.path.join(build, "wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert paths, "no device assembly for wave.hip: csrc/build.sh must compile it with -save-temps=obj"
    blocks = open(paths[0]).read().split("- .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert sum("wave_resample" in n for n in names) == 2 and sum("wave_stats" in n or "wave_normalize" in n for n in names) == 2, names
    for b, n in zip(blocks, names):
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n


def test_cli_wav_flag_and_reader(tmp_path, monkeypatch):
    """--wav: refused without --encodec; read_wave returns the first channel and the file's own rate through soundfile when
    torchaudio is absent, and says so when neither is installed; read_audio_prompt still refuses every rate but 24 000 Hz."""
    from v2a_amd import cli
    base = ["ck", "0", "scp", "0", "1", "out"]
    assert cli.build_parser().parse_args(base).wav is False
    assert cli.build_parser().parse_args(base + ["--wav", "--encodec", "e.pt"]).wav is True
    with pytest.raises(SystemExit):
        cli.main(base + ["--wav"])
    with pytest.raises(SystemExit):
        cli.main(base + ["--wav", "--validate"])
    monkeypatch.setitem(sys.modules, "torchaudio", None)           # import torchaudio -> ImportError
    monkeypatch.setitem(sys.modules, "soundfile", None)
    with pytest.raises(RuntimeError, match="torchaudio or soundfile"):
        cli.read_wave(str(tmp_path / "a.wav"))
    data = np.arange(2 * 5000, dtype=np.float32).reshape(5000, 2) / 10000
    seen = []

    def read(path, dtype, always_2d):
        seen.append((path, dtype, always_2d))
        return data, 44100
    monkeypatch.setitem(sys.modules, "soundfile", types.SimpleNamespace(read=read))
    w, rate = cli.read_wave(str(tmp_path / "a.wav"))
    assert rate == 44100 and w.shape == (5000,) and w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(data[:, 0].copy()))
    assert seen == [(str(tmp_path / "a.wav"), "float32", True)]
    with pytest.raises(ValueError, match="44100 Hz"):
        cli.read_audio_prompt(str(tmp_path / "a.mp4"), 0.1)


def test_latent_npy_wins_over_wav_in_validation(tmp_path):
    from v2a_amd import cli
    vids = [str(tmp_path / f"clip{i}.mp4") for i in range(4)]
    for i in (0, 1):
        np.save(vids[i].replace(".mp4", ".latent.npy"), np.zeros((3, 4), np.float32))
    for i in (1, 2):
        open(vids[i].replace(".mp4", ".wav"), "wb").close()
    lat, wav = [v.replace(".mp4", ".latent.npy") for v in vids], [v.replace(".mp4", ".wav") for v in vids]
    assert cli.validation_sources(vids, wav=True) == [("latent", lat[0]), ("latent", lat[1]), ("wav", wav[2]), ("latent", lat[3])]
    assert cli.validation_sources(vids, wav=False) == [("latent", p) for p in lat]           # without --wav nothing changes
    assert cli.validation_sources(vids) == cli.validation_sources(vids, wav=False)


def test_encode_audio_without_an_encoder_raises():
    import v2a_amd
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                       max_seq_len=256, if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=128, device="cpu")
    with pytest.raises(RuntimeError, match="load_audio_encoder"):
        m.encode_audio([torch.zeros(4000)], [44100])
    assert v2a_amd.WaveFrontEnd is WaveFrontEnd and v2a_amd.sinc_resample_table is sinc_resample_table


def test_cli_wave_prompt_is_cut_after_the_front_end(tmp_path, monkeypatch):
    """--wav --audio-prompt-seconds: `<video>.wav` at its own rate goes through the model's front end and the first S seconds of the
    24 kHz result are the prompt; a result shorter than S seconds is refused."""
    from v2a_amd import cli
    data = np.linspace(-1, 1, 2 * 50000, dtype=np.float32).reshape(50000, 2)
    monkeypatch.setitem(sys.modules, "torchaudio", None)
    monkeypatch.setitem(sys.modules, "soundfile", types.SimpleNamespace(read=lambda path, dtype, always_2d: (data, 44100)))
    seen = []

    def front(wav, rate):
        seen.append((tuple(wav.shape), rate))
        return torch.arange(27211, dtype=torch.float32)             # ceil(80 * 50000 / 147) samples at 24 kHz
    model = types.SimpleNamespace(wave_front_end=lambda: front)
    w = cli.wave_prompt(model, str(tmp_path / "a.mp4"), 1.0)
    assert seen == [((50000,), 44100)] and torch.equal(w, torch.arange(24000, dtype=torch.float32))
    with pytest.raises(ValueError, match="needs 36000"):
        cli.wave_prompt(model, str(tmp_path / "a.mp4"), 1.5)
