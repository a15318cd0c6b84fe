"""The wave front end of the reference's data path, on the device: what turns the first channel of an audio file at any rate into
the wave the Encodec encoder reads (trainer_multigpus_alldatas3.py:1047-1050 and 1427-1431):

    waveform = waveform[0:1, :]
    waveform = torchaudio.functional.resample(waveform, sr, 24000)      # if sr != 24000
    waveform = torch_tools.normalize_wav(waveform)                      # torch_tools.py:53-56
    waveform = waveform[:, :val_length * hop_size]                      # validation only (:1133)

The filter table is built here on the host, once per rate pair; the FIR, the reductions and the normalisation are the three kernels
of csrc/wave.hip.  torchaudio is not a dependency: the table restates the `sinc_interp_hann` kernel of its documentation and source
(`_get_sinc_resample_kernel`), evaluated in float64 and rounded once to fp32 -- the `dtype=None` reading that `transforms.Resample`
uses (DESIGN 1b says how far the other reading, the same formula evaluated in fp32, lies)."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L

TABLE_MAX = 1 << 22              # V2A_WAVE_TABLE_MAX: entries of the largest table built (16 MiB of fp32, 32 MiB while in float64)
WINDOW_MAX = 8192                # taps of one phase the kernel's LDS window holds (csrc/wave.hip: WAVE_WINDOW_MAX)
TILE_OUT = 1024                  # outputs a workgroup aims at per tile (csrc/wave.hip: WAVE_TILE_OUT)
LDS_BYTES = 128 * 1024           # V2A_WAVE_LDS_BYTES: window + table of a workgroup
MAX_PARTS = 256                  # V2A_WAVE_MAX_PARTS
PART_BYTES = 16                  # { double sum; float min; float max; }


def resample_geometry(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(o, n, width, K): the reduced rates, the half width of the filter in input samples and the taps of one phase."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"sample rates must be positive, got {orig_freq} -> {new_freq} Hz")
    if lowpass_filter_width <= 0:
        raise ValueError("lowpass_filter_width must be positive")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    return o, n, width, 2 * width + o


def table_in_lds(o: int, n: int, K: int) -> bool:
    """Whether v2a_wave_resample stages the table in LDS (the host side of csrc/wave.hip restated): a workgroup takes
    Q = max(1, 1024 // n) consecutive q, fewer if their window (Q - 1) * o + K would pass WINDOW_MAX floats, and the table goes
    beside that window when both fit LDS_BYTES."""
    Q = min(max(1, TILE_OUT // n), (WINDOW_MAX - K) // o + 1)
    return 4 * ((Q - 1) * o + K + n * K) <= LDS_BYTES


def resampled_length(length: int, o: int, n: int) -> int:
    """Samples of the resampled wave: ceil(n * length / o)."""
    return -(-n * int(length) // o)


def sinc_resample_table(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """torchaudio's `sinc_interp_hann` resampling kernel -> (table fp32 (P, K), width, o, n), P = n phases of K = 2 * width + o taps.

    Output j = q * n + p of a wave x is sum_k xpad[q * o + k] * table[p][k], xpad = x with `width` zeros in front and `width + o`
    behind.  A rate pair whose table would hold more than TABLE_MAX entries, or more than WINDOW_MAX taps per phase, is refused with
    a ValueError before anything is allocated (44 101 -> 24 000 Hz would need about 1e9 entries)."""
    o, n, width, K = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    if n * K > TABLE_MAX or K > WINDOW_MAX:
        raise ValueError(f"resampling {orig_freq} Hz -> {new_freq} Hz needs a filter table of {n} phases x {K} taps = {n * K} entries; "
                         f"at most {TABLE_MAX} entries and {WINDOW_MAX} taps are built (the rates share too small a common divisor)")
    lpw = float(lowpass_filter_width)
    base = min(o, n) * rolloff
    idx = torch.arange(-width, width + o, dtype=torch.float64) / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx[None, :]) * base
    t = t.clamp(-lpw, lpw)
    win = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    table = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * win * (base / o)
    return table.to(torch.float32).contiguous(), width, o, n


class WaveFrontEnd:
    """First channel -> `new_freq` Hz -> `normalize_wav`, on `device`, without a visit to the host.

    resample(wave, orig_freq), normalize(wave) and __call__(wave, orig_freq, normalize=True, max_samples=None) return 1-D fp32
    tensors on the device; a 2-D (channels, n) input stands for its channel 0, as in the reference.  Tables are built once per rate
    and kept on the device.  `last_stats` is (mean, peak) of the last normalisation -- reading it is the only host synchronisation."""

    def __init__(self, device="cuda:0", new_freq: int = 24000, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.dev = torch.device(device)
        self.new_freq, self.lowpass_filter_width, self.rolloff = int(new_freq), int(lowpass_filter_width), float(rolloff)
        self._tables: dict = {}
        self._stats = None

    def table(self, orig_freq: int):
        """(table on the device, width, o, n) of orig_freq -> new_freq; ValueError for a pair whose table is too large."""
        key = int(orig_freq)
        if key not in self._tables:
            t, width, o, n = sinc_resample_table(key, self.new_freq, self.lowpass_filter_width, self.rolloff)
            L.lib()                                                  # fail loudly without the HIP library, before the copy
            self._tables[key] = (t.to(self.dev), width, o, n)
        return self._tables[key]

    def _wave(self, wave) -> torch.Tensor:
        wave = torch.as_tensor(wave)
        if wave.ndim == 2:
            wave = wave[0]
        if wave.ndim != 1 or wave.shape[0] < 1:
            raise ValueError(f"a wave is (n,) or (channels, n) with n >= 1, got {tuple(wave.shape)}")
        return wave.to(self.dev, torch.float32).contiguous()

    def _parts(self):
        return torch.empty(MAX_PARTS * PART_BYTES // 8, dtype=torch.float64, device=self.dev), C.c_int32(0)

    def _resample(self, x, orig_freq):
        """x (L,) on the device -> (y, parts, n_parts); the table is looked up (and a refused pair raises) before any allocation."""
        table, width, o, n = self.table(orig_freq)
        y = torch.empty(resampled_length(x.shape[0], o, n), dtype=torch.float32, device=self.dev)
        parts, n_parts = self._parts()
        with torch.cuda.device(self.dev):
            L._launch("wave_resample", 2.0 * y.shape[0] * table.shape[1], 4.0 * (x.shape[0] + y.shape[0] + table.numel()),
                      lambda: L.lib().v2a_wave_resample(x.data_ptr(), x.shape[0], table.data_ptr(), o, n, table.shape[1], width, y.data_ptr(),
                                                        y.shape[0], parts.data_ptr(), C.byref(n_parts), L.stream_ptr()))
        return y, parts, n_parts.value

    def _normalize(self, x, parts, n_parts, n_out):
        out = torch.empty(x.shape[0] if n_out is None else int(n_out), dtype=torch.float32, device=self.dev)
        if out.shape[0] < 1:
            raise ValueError(f"normalize: a destination of {out.shape[0]} samples")
        stats = torch.empty(2, dtype=torch.float32, device=self.dev)
        if parts is None:
            parts, np_ = self._parts()
            with torch.cuda.device(self.dev):
                L._launch("wave_stats", 0.0, 4.0 * x.shape[0],
                          lambda: L.lib().v2a_wave_stats(x.data_ptr(), x.shape[0], parts.data_ptr(), C.byref(np_), L.stream_ptr()))
            n_parts = np_.value
        with torch.cuda.device(self.dev):
            L._launch("wave_normalize", 3.0 * out.shape[0], 4.0 * (min(x.shape[0], out.shape[0]) + out.shape[0]),
                      lambda: L.lib().v2a_wave_normalize(x.data_ptr(), x.shape[0], parts.data_ptr(), n_parts, out.data_ptr(), out.shape[0],
                                                         stats.data_ptr(), L.stream_ptr()))
        self._stats = stats
        return out

    @property
    def last_stats(self):
        """(mean, peak) of the last normalised wave as Python floats (fp32 values), None before the first."""
        return None if self._stats is None else tuple(self._stats.tolist())

    @torch.no_grad()
    def resample(self, wave, orig_freq: int) -> torch.Tensor:
        """`torchaudio.functional.resample(wave, orig_freq, new_freq)` of channel 0; orig_freq == new_freq returns the wave as it is."""
        if int(orig_freq) == self.new_freq:
            return self._wave(wave)
        self.table(orig_freq)                                        # a refused rate pair raises before the wave is copied
        return self._resample(self._wave(wave), orig_freq)[0]

    @torch.no_grad()
    def normalize(self, wave, n_out=None) -> torch.Tensor:
        """`normalize_wav` (torch_tools.py:53-56) of channel 0; n_out: the length of the result, the normalised wave cut there or
        followed by zeros (mean and peak are the whole wave's either way, as the reference normalises before it cuts)."""
        return self._normalize(self._wave(wave), None, 0, n_out)

    @torch.no_grad()
    def __call__(self, wave, orig_freq: int, normalize: bool = True, max_samples=None) -> torch.Tensor:
        """The whole front end.  max_samples: keep at most that many samples of the result (the validation set's
        `[:, :val_length * hop_size]`), taken after the normalisation."""
        if int(orig_freq) != self.new_freq:
            self.table(orig_freq)                                    # a refused rate pair raises before the wave is copied
        x = self._wave(wave)
        parts, n_parts = None, 0
        if int(orig_freq) != self.new_freq:
            x, parts, n_parts = self._resample(x, orig_freq)
        keep = x.shape[0] if max_samples is None else max(1, min(x.shape[0], int(max_samples)))
        return self._normalize(x, parts, n_parts, keep) if normalize else x[:keep]
