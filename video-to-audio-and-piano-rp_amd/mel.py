"""The log-mel front end of the reference, on the device: `MelSpec` (e2_tts_crossatt3.py:375-417), the module its callers import next
to `EncodecWrapper` (predict.py:49, app.py:49) and the other `mel_spec_module` of `E2TTS`:

    mel = torchaudio.transforms.MelSpectrogram(sample_rate, n_fft, win_length, hop_length, n_mels, power, center, normalized, norm)(wave)
    mel = mel.clamp(min=1e-5).log()                                     # x3:293-294

torchaudio is not a dependency.  Its two tables are restated here on the host in float64 and rounded to fp32 once, on the way to the
device: `mel_filterbank` is `torchaudio.functional.melscale_fbanks` (HTK scale), `stft_basis` the windowed real DFT that `torch.stft`
evaluates with an FFT.  Window, normalisation and mel norm are all in those tables; the launches of a call -- v2a_mel_pad, the
exact-fp32 v2a_gemm over overlapping rows (lda = hop, K = n_fft in chunks of K_CHUNK samples, one launch and one partial DFT per
chunk), v2a_mel_from_dft (csrc/mel.hip) -- know the sizes and `power` alone.
DESIGN 1b says what pins the restatement (torch.stft in float64, transformers' mel_filter_bank) and where the tables differ."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

MAX_FFT = 2048                   # V2A_MEL_MAX_FFT: bins of 16 frames a workgroup of v2a_mel_from_dft holds in LDS
LOG_EPS = 1e-5                   # x3:293: log(t, eps=1e-5)
CACHE_MAX = 8                    # (b, nw) work-buffer sets kept per module
K_CHUNK = 256                    # samples of a frame one GEMM launch sums: the exact-fp32 GEMM adds its K products in one chain


def mel_filterbank(n_freqs: int, n_mels: int, sample_rate: int, f_min: float = 0.0, f_max=None, norm=None) -> torch.Tensor:
    """torchaudio's `melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm, mel_scale="htk")` in float64 -> (n_freqs, n_mels):
    bin frequencies linspace(0, sample_rate // 2, n_freqs), n_mels + 2 points equally spaced in HTK mel 2595 log10(1 + f / 700),
    triangles max(0, min(down, up)), and with norm="slaney" filter m scaled by 2 / (f[m + 2] - f[m]).  f_max: sample_rate // 2, as
    MelSpectrogram sets it.  torchaudio evaluates the same formulas in fp32; MelSpec rounds this table to fp32 once."""
    n_freqs, n_mels = int(n_freqs), int(n_mels)
    if norm not in (None, "slaney"):
        raise ValueError(f'norm must be None or "slaney", got {norm!r}')
    if n_freqs < 2 or n_mels < 1:
        raise ValueError(f"mel_filterbank: n_freqs={n_freqs} (>= 2), n_mels={n_mels} (>= 1)")
    f_max = float(int(sample_rate) // 2) if f_max is None else float(f_max)
    if not 0.0 <= float(f_min) <= f_max:
        raise ValueError(f"mel_filterbank: f_min={f_min} f_max={f_max}")
    all_freqs = np.linspace(0, int(sample_rate) // 2, n_freqs)
    m_min = 2595.0 * np.log10(1.0 + (float(f_min) / 700.0))
    m_max = 2595.0 * np.log10(1.0 + (f_max / 700.0))
    f_pts = 700.0 * (np.power(10, np.linspace(m_min, m_max, n_mels + 2) / 2595.0) - 1.0)
    f_diff = np.diff(f_pts)
    slopes = f_pts[None, :] - all_freqs[:, None]                     # (n_freqs, n_mels + 2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(np.zeros(1), np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    return torch.from_numpy(np.ascontiguousarray(fb))


def stft_window(n_fft: int, win_length: int) -> torch.Tensor:
    """The periodic Hann window of win_length in float64, zero-padded on both sides to n_fft as torch.stft centres it."""
    n_fft, win_length = int(n_fft), int(win_length)
    if not 1 <= win_length <= n_fft:
        raise ValueError(f"win_length={win_length} must lie in 1 .. filter_length={n_fft}")
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    return w


def stft_basis(n_fft: int, win_length: int, normalized: bool = False) -> torch.Tensor:
    """The windowed real DFT basis in float64, (2 * (n_fft / 2 + 1), n_fft): row k = cos(2 pi k j / n_fft) w[j] and row
    n_fft / 2 + 1 + k = -sin(2 pi k j / n_fft) w[j], so basis @ frame = re | im of torch.stft's bins k = 0 .. n_fft / 2.  The phase
    k j is reduced mod n_fft in integers before the cosine.  normalized: divided by sqrt(sum(w^2)), torchaudio's "window" normalisation."""
    n_fft = int(n_fft)
    if n_fft < 4 or n_fft % 2:
        raise ValueError(f"filter_length={n_fft} must be even and at least 4")
    w = stft_window(n_fft, win_length)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    j = torch.arange(n_fft, dtype=torch.int64)[None, :]
    ang = ((k * j) % n_fft).to(torch.float64) * (2.0 * math.pi / n_fft)
    basis = torch.cat([torch.cos(ang) * w, -torch.sin(ang) * w], 0)
    if normalized:
        basis = basis / w.pow(2).sum().sqrt()
    return basis


def filterbank_bands(fb: torch.Tensor):
    """(n_freqs, n_mels) fp32 filterbank -> (bands int32 (n_mels, 2) = first bin and bin count of every channel, weights fp32
    (n_mels, wpitch)): the band form v2a_mel_from_dft reads.  A triangular filter has one contiguous support; the band runs from its
    first to its last non-zero weight (an empty filter: count 0)."""
    fb = fb.to(torch.float32)
    n_freqs, n_mels = fb.shape
    bands = torch.zeros(n_mels, 2, dtype=torch.int32)
    for m in range(n_mels):
        nz = torch.nonzero(fb[:, m]).flatten()
        if nz.numel():
            bands[m, 0], bands[m, 1] = int(nz[0]), int(nz[-1]) - int(nz[0]) + 1
    wpitch = max(1, int(bands[:, 1].max()))
    weights = torch.zeros(n_mels, wpitch, dtype=torch.float32)
    for m in range(n_mels):
        first, count = int(bands[m, 0]), int(bands[m, 1])
        weights[m, :count] = fb[first:first + count, m]
    return bands.contiguous(), weights.contiguous()


class MelSpec:
    """The reference's `MelSpec` with its keywords and defaults, plus `device`.  `__call__` / `forward(inp)`: (b, nw) or (b, 1, nw) float
    waves on the host or the device -> (b, n_mel_channels, T) fp32 log-mel on `device`, T = 1 + nw // hop_length (center=True) or
    1 + (nw - filter_length) // hop_length (center=False).  `mel(inp)`: the same without the log.  All rows share nw, as in the
    reference.  ValueError for what torch or the kernels would refuse; tables go to the device on first use."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=100, sampling_rate=24_000, normalize=False,
                 power=1, norm=None, center=True, device="cuda:0"):
        self.n_fft, self.hop, self.win_length = int(filter_length), int(hop_length), int(win_length)
        self.n_mel_channels, self.sampling_rate = int(n_mel_channels), int(sampling_rate)
        self.normalize, self.norm, self.center = bool(normalize), norm, bool(center)
        self.dev = torch.device(device)
        if self.n_fft < 4 or self.n_fft % 2 or self.n_fft > MAX_FFT:
            raise ValueError(f"filter_length={filter_length} must be even and lie in 4 .. {MAX_FFT}")
        if not 1 <= self.win_length <= self.n_fft:
            raise ValueError(f"win_length={win_length} must lie in 1 .. filter_length={filter_length}")
        if self.hop < 1 or self.hop % 4:
            raise ValueError(f"hop_length={hop_length} must be a positive multiple of 4 (the row stride of the exact-fp32 GEMM)")
        if power not in (1, 2):
            raise ValueError(f"power={power!r} must be 1 or 2")
        if norm not in (None, "slaney"):
            raise ValueError(f'norm must be None or "slaney", got {norm!r}')
        if self.n_mel_channels < 1 or self.sampling_rate < 2:
            raise ValueError(f"n_mel_channels={n_mel_channels}, sampling_rate={sampling_rate}")
        self.power = int(power)
        self.n_bins = self.n_fft // 2 + 1
        self.pad = self.n_fft // 2 if self.center else 0
        self.k_pad = -(-self.n_fft // 16) * 16                      # K of the fp32 GEMM: whole K tiles of 16, the basis zero behind n_fft
        self.n_pad = -(-2 * self.n_bins // 4) * 4                   # N and ldo of the GEMM: 16-byte rows
        self.n_chunks = -(-self.k_pad // K_CHUNK)                   # partial DFTs of a frame, added in chunk order by v2a_mel_from_dft
        self._tables = None
        self._cache: dict = {}

    def frames(self, nw: int) -> int:
        """T of a wave of nw samples; ValueError where torch.stft would refuse it."""
        nw = int(nw)
        if self.center and nw <= self.pad:
            raise ValueError(f"center=True reflects {self.pad} samples on both sides: a wave needs more than that, got {nw}")
        if not self.center and nw < self.n_fft:
            raise ValueError(f"center=False needs at least filter_length={self.n_fft} samples, got {nw}")
        return 1 + (nw + 2 * self.pad - self.n_fft) // self.hop

    def host_tables(self):
        """(basis fp32 (n_pad, k_pad) with re of bin k in row 2k and im in row 2k + 1, bands int32 (n_mels, 2), weights fp32
        (n_mels, wpitch)): the float64 tables rounded once, in the layouts the kernels read."""
        b64 = stft_basis(self.n_fft, self.win_length, self.normalize)
        basis = torch.zeros(self.n_pad, self.k_pad, dtype=torch.float32)
        basis[0:2 * self.n_bins:2, :self.n_fft] = b64[:self.n_bins].to(torch.float32)
        basis[1:2 * self.n_bins:2, :self.n_fft] = b64[self.n_bins:].to(torch.float32)
        fb = mel_filterbank(self.n_bins, self.n_mel_channels, self.sampling_rate, norm=self.norm).to(torch.float32)
        return (basis,) + filterbank_bands(fb)

    def _device_tables(self):
        if self._tables is None:
            basis, bands, weights = self.host_tables()
            L.lib()                                                  # fail loudly without the HIP library, before the copies
            self._tables = (basis.to(self.dev), bands, bands.to(self.dev), weights.to(self.dev))
        return self._tables

    def _wave(self, inp) -> torch.Tensor:
        inp = torch.as_tensor(inp)
        if inp.ndim == 3:
            if inp.shape[1] != 1:
                raise ValueError(f"a wave batch is (b, nw) or (b, 1, nw), got {tuple(inp.shape)}")
            inp = inp[:, 0]
        if inp.ndim != 2 or inp.shape[0] < 1:
            raise ValueError(f"a wave batch is (b, nw) or (b, 1, nw), got {tuple(inp.shape)}")
        if not inp.is_floating_point():
            raise ValueError(f"waves are floating point, got {inp.dtype}")
        return inp

    def _buffers(self, b: int, nw: int, T: int):
        key = (b, nw)
        if key not in self._cache:
            lp = nw + 2 * self.pad
            pitch = -(-lp // self.hop) * self.hop
            rows = (b - 1) * (pitch // self.hop) + T                 # GEMM rows; those between two clips are computed and never read
            if rows >= 1 << 31 or b > 65535:
                raise ValueError(f"{b} waves of {nw} samples make {rows} frames: more than one launch takes")
            if len(self._cache) >= CACHE_MAX:
                self._cache.pop(next(iter(self._cache)))
            # zeroed once: the pad kernel writes lp samples per clip, the GEMM's last rows read up to k_pad samples behind them
            padded = torch.zeros(b * pitch + self.k_pad, dtype=torch.float32, device=self.dev)
            dft = torch.empty(self.n_chunks, rows, self.n_pad, dtype=torch.float32, device=self.dev)
            self._cache[key] = (padded, dft, pitch, rows)
        return self._cache[key]

    @torch.no_grad()
    def _run(self, inp, eps: float, out=None) -> torch.Tensor:
        inp = self._wave(inp)
        b, nw = int(inp.shape[0]), int(inp.shape[1])
        T = self.frames(nw)
        self._device_tables()
        x = inp.to(self.dev, torch.float32).contiguous()
        if out is not None and (out.shape != (b, self.n_mel_channels, T) or out.dtype != torch.float32 or out.device != x.device
                                or out.stride(2) != 1):
            raise ValueError(f"out must be a ({b}, {self.n_mel_channels}, {T}) fp32 tensor on {x.device} with unit stride along time")
        padded, dft, pitch, rows = self._buffers(b, nw, T)
        if out is None:
            out = torch.empty(b, self.n_mel_channels, T, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            self._stage_pad(x, padded, pitch)
            self._stage_dft(padded, dft, rows)
            self._stage_mel(dft, pitch, b, T, eps, out)
        return out

    # the three stages of a call, one method each (scripts/mel_spec_probe.py times them apart)
    def _stage_pad(self, x, padded, pitch):
        b, nw = x.shape
        L._launch("mel_pad", 0.0, 4.0 * b * (2 * nw + 2 * self.pad),
                  lambda: L.lib().v2a_mel_pad(x.data_ptr(), nw, b, nw, self.pad, padded.data_ptr(), pitch, L.stream_ptr()))

    def _stage_dft(self, padded, dft, rows):
        basis = self._device_tables()[0]
        for c in range(self.n_chunks):                               # chunk c of every frame: A and W moved by the chunk, lda = hop
            k0, k1 = c * K_CHUNK, min((c + 1) * K_CHUNK, self.k_pad)
            L.gemm([(padded[k0:], self.hop, k1 - k0)], basis[:, k0:], dft[c], M=rows, N=self.n_pad, compute=L.F32, ldo=self.n_pad)

    def _stage_mel(self, dft, pitch, b, T, eps, out):
        _, bands_host, bands, weights = self._device_tables()
        L._launch("mel_from_dft", b * T * (3.0 * self.n_bins + 2.0 * int(bands_host[:, 1].sum())),
                  4.0 * b * T * (2 * self.n_bins * self.n_chunks + self.n_mel_channels),
                  lambda: L.lib().v2a_mel_from_dft(dft.data_ptr(), self.n_pad, pitch // self.hop, self.n_chunks, dft.stride(0), b, T, self.n_fft,
                                                   self.hop, self.n_mel_channels, bands_host.data_ptr(), bands.data_ptr(), weights.data_ptr(),
                                                   weights.shape[1], self.power, float(eps), out.data_ptr(), out.stride(0), out.stride(1),
                                                   L.stream_ptr()))

    def forward(self, inp, out=None) -> torch.Tensor:
        """log(clamp(mel, 1e-5)); `out`: an fp32 (b, n_mel_channels, T) destination on the device, any batch and row strides."""
        return self._run(inp, LOG_EPS, out)

    __call__ = forward

    def mel(self, inp, out=None) -> torch.Tensor:
        """The mel spectrogram itself, without the log."""
        return self._run(inp, -1.0, out)
