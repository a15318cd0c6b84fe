"""The Vocos vocoder on the device: mel frames -> wave, the `vocos` of a model whose latents are log-mel frames.  The reference builds it
with `Vocos.from_pretrained('charactr/vocos-mel-24khz')` (e2_tts_crossatt.py:1324, e2_tts_crossatt6.py:1469) and calls
`self.vocos.decode(mel)` per clip (x3:2275-2287); that checkpoint reads exactly the frames `MelSpec` makes (100 mels, n_fft 1024, hop 256,
centre padding).  This is the mel variant with padding="center":

    x = LayerNorm(Conv1d(C, dim, 7, padding=3)(features))                                  backbone.embed, backbone.norm
    x = x + gamma * pwconv2(GELU(pwconv1(LayerNorm(dwconv7(x)))))                          backbone.convnext.{i}
    m | p = head.out(LayerNorm(x))                                                         backbone.final_layer_norm, head.out
    S = min(exp(m), 100) (cos p + i sin p);  wave = torch.istft(S, n_fft, hop, window=hann, center=True)

The `vocos` package is not a dependency.  The launches of a call (csrc/vocos.hip, include/v2a_cfm.h): v2a_vocos_stage_in, the embed
convolution as an exact-fp32 v2a_gemm over overlapping rows, v2a_clip_layernorm, per block v2a_vocos_dwconv_ln, v2a_gemm (pwconv1),
v2a_vocos_gelu, v2a_gemm (pwconv2) and v2a_vocos_scale_residual, v2a_clip_layernorm, the head GEMM, v2a_vocos_spectrum, the inverse DFT as
v2a_gemm against `istft_basis`, v2a_vocos_overlap_add.  Every GEMM runs in K chunks of K_CHUNK columns (`_gemm_chain`): the exact-fp32
GEMM adds its K products in one fp32 chain, and with K = 1536 in one chain a block of the 24 kHz network came out 4.5 times further from
float64 than torch's CPU fp32, past the 4 the tests allow; chunk c adds to the sum of the chunks before it through the RESID epilogue,
so the partials are added in chunk order.  One arithmetic mode, fp32 throughout.
DESIGN 1b says what pins this restatement (a float64 restatement in torch that ends in torch.istft)."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib as L

LN_EPS = 1e-6
MAX_DIM, MAX_FFT, MAX_FRAMES = 2048, 4096, 1 << 24         # V2A_VOCOS_MAX_DIM, V2A_VOCOS_MAX_FFT, V2A_VOCOS_MAX_FRAMES
K_CHUNK = 256                    # K of one GEMM launch, as MelSpec cuts its K: longer chains of the exact-fp32 GEMM lose accuracy
CACHE_MAX = 8                    # (b, T) work-buffer sets kept per module
ENVELOPE_MIN = 1e-11             # torch.istft refuses a window envelope that falls below this


def expected_state_dict_shapes(C: int = 100, dim: int = 512, hidden: int = 1536, depth: int = 8, n_fft: int = 1024) -> dict:
    """Key -> shape of the tensors `Vocos` reads, as `Vocos.from_pretrained` stores them (`feature_extractor.*` and
    `head.istft.window` may be present and are ignored).  The defaults are charactr/vocos-mel-24khz."""
    s = {"backbone.embed.weight": (dim, C, 7), "backbone.embed.bias": (dim,), "backbone.norm.weight": (dim,), "backbone.norm.bias": (dim,)}
    for i in range(depth):
        p = f"backbone.convnext.{i}."
        s.update({p + "dwconv.weight": (dim, 1, 7), p + "dwconv.bias": (dim,), p + "norm.weight": (dim,), p + "norm.bias": (dim,),
                  p + "pwconv1.weight": (hidden, dim), p + "pwconv1.bias": (hidden,), p + "pwconv2.weight": (dim, hidden),
                  p + "pwconv2.bias": (dim,), p + "gamma": (dim,)})
    s.update({"backbone.final_layer_norm.weight": (dim,), "backbone.final_layer_norm.bias": (dim,),
              "head.out.weight": (n_fft + 2, dim), "head.out.bias": (n_fft + 2,)})
    return s


def istft_basis(n_fft: int) -> torch.Tensor:
    """The windowed inverse real DFT in float64, (n_fft, 2 * (n_fft / 2 + 1)): column 2k = c_k cos(2 pi k n / n_fft) w[n] / n_fft and
    column 2k + 1 = -c_k sin(2 pi k n / n_fft) w[n] / n_fft with c_0 = c_{n_fft/2} = 1 and c_k = 2 between, w the periodic Hann window,
    so basis @ (re, im interleaved) = irfft(S) * w.  The sine columns of the DC and Nyquist bins are exactly zero: a C2R transform
    ignores those imaginary parts.  The phase k n is reduced mod n_fft in integers before the cosine."""
    n_fft = int(n_fft)
    if n_fft < 4 or n_fft % 4:
        raise ValueError(f"n_fft={n_fft} must be a multiple of 4 and at least 4")
    nb = n_fft // 2 + 1
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    n = torch.arange(n_fft, dtype=torch.int64)[:, None]
    k = torch.arange(nb, dtype=torch.int64)[None, :]
    ang = ((k * n) % n_fft).to(torch.float64) * (2.0 * math.pi / n_fft)
    coef = torch.full((nb,), 2.0, dtype=torch.float64)
    coef[0] = coef[-1] = 1.0
    scale = (w / n_fft)[:, None] * coef[None, :]
    sin = -torch.sin(ang) * scale
    sin[:, 0] = 0.0
    sin[:, -1] = 0.0
    basis = torch.empty(n_fft, 2 * nb, dtype=torch.float64)
    basis[:, 0::2] = torch.cos(ang) * scale
    basis[:, 1::2] = sin
    return basis


def window_envelope(n_fft: int, hop: int, T: int) -> np.ndarray:
    """sum_t w^2[n + n_fft / 2 - t hop] over the T frames that cover sample n, n < (T - 1) hop, in float64: the divisor of torch.istft."""
    wsq = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).pow(2).numpy()
    full = np.zeros((T - 1) * hop + n_fft)
    for t in range(T):
        full[t * hop:t * hop + n_fft] += wsq
    return full[n_fft // 2:n_fft // 2 + (T - 1) * hop]


def overlap_add_numpy(frames: np.ndarray, hop: int) -> np.ndarray:
    """The gather form v2a_vocos_overlap_add evaluates, on the host: frames (T, n_fft) = irfft(S[:, t]) * w -> (T - 1) hop samples,
    y[n] = sum_t frames[t][p - t hop] / sum_t w^2[p - t hop] with p = n + n_fft / 2, ascending t, in the dtype of `frames`."""
    T, n_fft = frames.shape
    wsq = (torch.hann_window(n_fft, periodic=True, dtype=torch.float64).pow(2)).numpy().astype(frames.dtype)
    out = np.zeros((T - 1) * hop, dtype=frames.dtype)
    for n in range(out.shape[0]):
        p = n + n_fft // 2
        tlo = 0 if p - n_fft + 1 <= 0 else (p - n_fft + hop) // hop
        acc = env = frames.dtype.type(0)
        for t in range(tlo, min(p // hop, T - 1) + 1):
            acc = acc + frames[t, p - t * hop]
            env = env + wsq[p - t * hop]
        out[n] = acc / env
    return out


class Vocos:
    """`Vocos(state_dict, device="cuda:0", hop_length=None)`: C, dim, hidden, depth and n_fft are read from the shapes; hop_length
    defaults to n_fft // 4.  `decode(features)`: (b, C, T) or (C, T) fp32 on the host or the device -> (b, (T - 1) hop) fp32 on the
    device.  ValueError for what the kernels or torch.istft would refuse, NotImplementedError for the adaptive-norm (Encodec-feature)
    variant; weights and tables go to the device on first use."""

    def __init__(self, state_dict, device="cuda:0", hop_length=None):
        if not isinstance(state_dict, dict):
            raise TypeError(f"Vocos: a state dict, got {type(state_dict).__name__}")
        sd = {k: v for k, v in state_dict.items() if not k.startswith("feature_extractor.")}
        if any(k.endswith("norm.scale.weight") or k.endswith("norm.shift.weight") for k in sd):
            raise NotImplementedError("Vocos: adaptive-norm keys (norm.scale.weight): the Encodec-feature variant with padding=\"same\" is not built")
        for key in ("backbone.embed.weight", "head.out.weight"):
            if key not in sd:
                raise ValueError(f"Vocos: missing key {key}")
        ew, hw = sd["backbone.embed.weight"], sd["head.out.weight"]
        if ew.ndim != 3 or ew.shape[2] != 7:
            raise ValueError(f"Vocos: backbone.embed.weight has shape {tuple(ew.shape)}, expected (dim, C, 7)")
        if hw.ndim != 2:
            raise ValueError(f"Vocos: head.out.weight has shape {tuple(hw.shape)}, expected (n_fft + 2, dim)")
        self.dim, self.C, self.n_fft = int(ew.shape[0]), int(ew.shape[1]), int(hw.shape[0]) - 2
        depth = 0
        while f"backbone.convnext.{depth}.pwconv1.weight" in sd:
            depth += 1
        if depth < 1:
            raise ValueError("Vocos: missing key backbone.convnext.0.pwconv1.weight")
        self.depth = depth
        pw = sd["backbone.convnext.0.pwconv1.weight"]
        if pw.ndim != 2:
            raise ValueError(f"Vocos: backbone.convnext.0.pwconv1.weight has shape {tuple(pw.shape)}, expected (hidden, dim)")
        self.hidden = int(pw.shape[0])
        if self.dim % 16 or self.hidden % 16 or self.dim < 16 or self.hidden < 16:
            raise ValueError(f"Vocos: dim={self.dim} and hidden={self.hidden} must be multiples of 16 (the K granularity of the exact-fp32 GEMM)")
        if self.dim > MAX_DIM:
            raise ValueError(f"Vocos: dim={self.dim} is more than the {MAX_DIM} channels a tile of v2a_vocos_dwconv_ln holds")
        if self.n_fft < 4 or self.n_fft % 4 or self.n_fft > MAX_FFT:
            raise ValueError(f"Vocos: head.out.weight has {self.n_fft + 2} rows: n_fft={self.n_fft} must be a multiple of 4 in 4 .. {MAX_FFT}")
        for key, shape in expected_state_dict_shapes(self.C, self.dim, self.hidden, self.depth, self.n_fft).items():
            if key not in sd:
                raise ValueError(f"Vocos: missing key {key}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"Vocos: {key} has shape {tuple(sd[key].shape)}, expected {shape}")
        self.hop = self.n_fft // 4 if hop_length is None else int(hop_length)
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"Vocos: hop_length={self.hop} must lie in 1 .. n_fft={self.n_fft}")
        # every way the frames of a clip of T >= 2 frames can cover a sample occurs at some T <= ceil(n_fft / hop) + 2
        for T in range(2, -(-self.n_fft // self.hop) + 3):
            low = float(np.abs(window_envelope(self.n_fft, self.hop, T)).min())
            if not low > ENVELOPE_MIN:
                raise ValueError(f"Vocos: hop_length={self.hop} with a Hann window of {self.n_fft}: the window envelope falls to {low:.3e} "
                                 f"(clips of {T} frames), torch.istft refuses less than {ENVELOPE_MIN}")
        self.dev = torch.device(device)
        self.n_bins = self.n_fft // 2 + 1
        self.c_pad = -(-self.C // 16) * 16                              # K of the embed GEMM is 7 c_pad: whole K tiles of 16
        self.n_logits = -(-(self.n_fft + 2) // 4) * 4                   # N and ldo of the head GEMM: 16-byte rows
        self.k_spec = -(-2 * self.n_bins // 16) * 16                    # K of the inverse DFT: (re, im) pairs, zero behind them
        self._sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items() if k in expected_state_dict_shapes(self.C, self.dim, self.hidden, self.depth, self.n_fft)}
        self._w = None
        self._cache: dict = {}

    @classmethod
    def from_pretrained(cls, path, device="cuda:0"):
        """A local directory with `config.yaml` and `pytorch_model.bin`, as the hub stores charactr/vocos-mel-24khz: hop and padding
        come from the config's head (`init_args`: n_fft, hop_length, padding).  Nothing is ever fetched."""
        import yaml
        path = str(path)
        cfg_path, bin_path = os.path.join(path, "config.yaml"), os.path.join(path, "pytorch_model.bin")
        if not os.path.isdir(path) or not os.path.isfile(cfg_path) or not os.path.isfile(bin_path):
            raise FileNotFoundError(f"Vocos.from_pretrained: {path} is not a local directory with config.yaml and pytorch_model.bin "
                                    "(nothing is downloaded)")
        with open(cfg_path) as f:
            cfg = yaml.safe_load(f) or {}
        head = (cfg.get("head") or {}).get("init_args") or {}
        padding = head.get("padding", "same")                            # ISTFTHead's default
        if padding != "center":
            raise NotImplementedError(f"Vocos.from_pretrained: head padding={padding!r}; only padding=\"center\" (the mel variant) is built")
        sd = torch.load(bin_path, map_location="cpu")
        voc = cls(sd, device=device, hop_length=head.get("hop_length"))
        if "n_fft" in head and int(head["n_fft"]) != voc.n_fft:
            raise ValueError(f"Vocos.from_pretrained: config n_fft={head['n_fft']} but head.out.weight gives n_fft={voc.n_fft}")
        return voc

    def host_tables(self):
        """(basis fp32 (n_fft, k_spec): `istft_basis` rounded once, zero behind the 2 (n_fft / 2 + 1) columns; wsq fp32 (n_fft): w^2 of the
        periodic Hann window, rounded once): the tables the inverse-DFT GEMM and v2a_vocos_overlap_add read."""
        basis = torch.zeros(self.n_fft, self.k_spec, dtype=torch.float32)
        basis[:, :2 * self.n_bins] = istft_basis(self.n_fft).to(torch.float32)
        wsq = torch.hann_window(self.n_fft, periodic=True, dtype=torch.float64).pow(2).to(torch.float32)
        return basis, wsq

    def _weights(self):
        if self._w is None:
            L.lib()                                                      # fail loudly without the HIP library, before the copies
            sd, dev = self._sd, self.dev
            put = lambda t: t.contiguous().to(dev)
            ew = torch.zeros(self.dim, 7, self.c_pad)                    # W[d][j * c_pad + c] = embed.weight[d][c][j]
            ew[:, :, :self.C] = sd["backbone.embed.weight"].permute(0, 2, 1)
            hw = torch.zeros(self.n_logits, self.dim)
            hw[:self.n_fft + 2] = sd["head.out.weight"]
            hb = torch.zeros(self.n_logits)
            hb[:self.n_fft + 2] = sd["head.out.bias"]
            blocks = []
            for i in range(self.depth):
                p = f"backbone.convnext.{i}."
                blocks.append(dict(dw=put(sd[p + "dwconv.weight"][:, 0].t()), db=put(sd[p + "dwconv.bias"]),          # taps (7, dim)
                                   ng=put(sd[p + "norm.weight"]), nb=put(sd[p + "norm.bias"]),
                                   w1=put(sd[p + "pwconv1.weight"]), b1=put(sd[p + "pwconv1.bias"]),
                                   w2=put(sd[p + "pwconv2.weight"]), b2=put(sd[p + "pwconv2.bias"]), gamma=put(sd[p + "gamma"])))
            basis, wsq = self.host_tables()
            self._w = dict(ew=put(ew.reshape(self.dim, 7 * self.c_pad)), eb=put(sd["backbone.embed.bias"]),
                           ng=put(sd["backbone.norm.weight"]), nb=put(sd["backbone.norm.bias"]), blocks=blocks,
                           fg=put(sd["backbone.final_layer_norm.weight"]), fb=put(sd["backbone.final_layer_norm.bias"]),
                           hw=put(hw), hb=put(hb), basis=put(basis), wsq=put(wsq))
        return self._w

    def _buffers(self, b: int, T: int):
        key = (b, T)
        if key not in self._cache:
            P = T + 6                                                    # rows per clip: its frames, then six rows no stage reads
            M = (b - 1) * P + T                                          # GEMM rows
            if len(self._cache) >= CACHE_MAX:
                self._cache.pop(next(iter(self._cache)))
            f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)
            pair = lambda n: [f(M, n), f(M, n)]                          # the two buffers a chain of K chunks alternates between
            self._cache[key] = dict(P=P, M=M, staged=f(b * P, self.c_pad), x=pair(self.dim), y=f(M, self.dim), t=pair(self.dim),
                                    h=pair(self.hidden), logits=pair(self.n_logits), spec=f(M, self.k_spec), frames=pair(self.n_fft))
        return self._cache[key]

    @staticmethod
    def _gemm_chain(a, lda, K, w, bias, pair, M, N):
        """(M, K) rows at `a` (row stride lda) times w (N, K) + bias into one of the two (M, N) buffers of `pair`, which is returned.  K is
        cut into chunks of K_CHUNK: the exact-fp32 GEMM adds its K products in one fp32 chain, whose error grows with K.  Chunk 0 stores
        acc + bias; chunk c adds to the result of chunk c - 1 through the RESID epilogue, so the partial sums are added in chunk order."""
        flat, n_chunks = a.reshape(-1), -(-K // K_CHUNK)
        for c in range(n_chunks):
            k0, k1 = c * K_CHUNK, min((c + 1) * K_CHUNK, K)
            seg = [(flat[k0:], lda, k1 - k0)]
            if c == 0:
                L.gemm(seg, w[:, k0:], pair[0], M=M, N=N, compute=L.F32, bias=bias, ldo=N)
            else:
                L.gemm(seg, w[:, k0:], pair[c & 1], M=M, N=N, compute=L.F32, epilogue=L.EPI_RESID, resid=pair[(c - 1) & 1], ldr=N, ldo=N)
        return pair[(n_chunks - 1) & 1]

    # the stages of a call, one method each (scripts/vocos_probe.py times them apart)
    def _stage_in(self, x, lens_dev, buf, b, T):
        L._launch("vocos_stage_in", 0.0, 4.0 * b * (self.C * T + (T + 6) * self.c_pad),
                  lambda: L.lib().v2a_vocos_stage_in(x.data_ptr(), x.stride(0), x.stride(1), b, self.C, T, L._p(lens_dev), buf["staged"].data_ptr(),
                                                     self.c_pad, L.stream_ptr()))

    def _layernorm(self, x, y, gamma, beta, M):
        L._launch("vocos_layernorm", 0.0, 8.0 * M * self.dim,
                  lambda: L.lib().v2a_clip_layernorm(x.data_ptr(), self.dim, y.data_ptr(), self.dim, L.F32, M, self.dim, gamma.data_ptr(), beta.data_ptr(),
                                                     LN_EPS, L.stream_ptr()))

    def _stage_embed(self, buf):
        """The embed convolution over overlapping rows of the staged input (lda = c_pad, K = 7 c_pad) and backbone.norm -> x[0]."""
        w, M = self._weights(), buf["M"]
        e = self._gemm_chain(buf["staged"], self.c_pad, 7 * self.c_pad, w["ew"], w["eb"], buf["t"], M, self.dim)
        self._layernorm(e, buf["x"][0], w["ng"], w["nb"], M)

    def _stage_block(self, blk, buf, lens_dev, b, T, src):
        """One ConvNeXt block: x[src] -> x[1 - src]."""
        M, x, y = buf["M"], buf["x"], buf["y"]
        L._launch("vocos_dwconv_ln", 2.0 * 7 * b * T * self.dim, 8.0 * b * T * self.dim,
                  lambda: L.lib().v2a_vocos_dwconv_ln(x[src].data_ptr(), self.dim, blk["dw"].data_ptr(), blk["db"].data_ptr(), blk["ng"].data_ptr(),
                                                      blk["nb"].data_ptr(), LN_EPS, b, T, buf["P"], self.dim, L._p(lens_dev), y.data_ptr(), self.dim,
                                                      L.stream_ptr()))
        h = self._gemm_chain(y, self.dim, self.dim, blk["w1"], blk["b1"], buf["h"], M, self.hidden)
        L._launch("vocos_gelu", 0.0, 8.0 * M * self.hidden, lambda: L.lib().v2a_vocos_gelu(h.data_ptr(), self.hidden, M, self.hidden, L.stream_ptr()))
        p = self._gemm_chain(h, self.hidden, self.hidden, blk["w2"], blk["b2"], buf["t"], M, self.dim)
        L._launch("vocos_scale_residual", 2.0 * M * self.dim, 12.0 * M * self.dim,
                  lambda: L.lib().v2a_vocos_scale_residual(p.data_ptr(), self.dim, blk["gamma"].data_ptr(), x[src].data_ptr(), self.dim,
                                                           x[1 - src].data_ptr(), self.dim, M, self.dim, L.stream_ptr()))

    def _stage_head(self, buf, src):
        """backbone.final_layer_norm -> y, head.out -> the logits buffer, which is returned."""
        w, M = self._weights(), buf["M"]
        self._layernorm(buf["x"][src], buf["y"], w["fg"], w["fb"], M)
        return self._gemm_chain(buf["y"], self.dim, self.dim, w["hw"], w["hb"], buf["logits"], M, self.n_logits)

    def _stage_spectrum(self, logits, buf):
        M = buf["M"]
        L._launch("vocos_spectrum", 0.0, 4.0 * M * (self.n_fft + 2 + self.k_spec),
                  lambda: L.lib().v2a_vocos_spectrum(logits.data_ptr(), self.n_logits, M, self.n_fft, buf["spec"].data_ptr(), self.k_spec, L.stream_ptr()))

    def _stage_idft(self, buf):
        """-> the buffer that holds the windowed frames irfft(S[:, t]) * w."""
        return self._gemm_chain(buf["spec"], self.k_spec, self.k_spec, self._weights()["basis"], None, buf["frames"], buf["M"], self.n_fft)

    def _stage_overlap_add(self, frames, buf, lens_dev, b, T, out):
        L._launch("vocos_overlap_add", 0.0, 4.0 * b * T * self.n_fft + 4.0 * b * (T - 1) * self.hop,
                  lambda: L.lib().v2a_vocos_overlap_add(frames.data_ptr(), self.n_fft, buf["P"], self._weights()["wsq"].data_ptr(), b, T, self.n_fft,
                                                        self.hop, L._p(lens_dev), out.data_ptr(), out.stride(0), L.stream_ptr()))

    @torch.no_grad()
    def decode(self, features, lens=None, out=None, taps=None):
        """features (b, C, T) or (C, T) fp32 on the host or the device -> (b, (T - 1) hop) fp32 on the device.
        lens: b integers, 2 <= lens[i] <= T: clip i is decoded as if it were alone with lens[i] frames (every convolution zero padded at
        its own end, its own envelope); the result is then a list of (lens[i] - 1) hop waves, views of one buffer, from one pass.
        out: an fp32 (b, (T - 1) hop) destination on the device with unit stride along time and any row stride.
        taps: a dict that receives copies of the intermediate activations (tests): "embed", "block{i}", "final" (b, T, dim), "logits"
        (b, T, n_fft + 2), "S" (b, T, n_fft / 2 + 1, 2) and "wave"; frames at or behind lens[i] hold no result."""
        x = torch.as_tensor(features)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1] != self.C or x.shape[0] < 1:
            raise ValueError(f"features are (b, {self.C}, T) or ({self.C}, T), got {tuple(torch.as_tensor(features).shape)}")
        if not x.is_floating_point():
            raise ValueError(f"features are floating point, got {x.dtype}")
        b, T = int(x.shape[0]), int(x.shape[2])
        if T < 2:
            raise ValueError(f"a wave needs at least 2 frames ((T - 1) hop samples), got T={T}")
        if b > 65535 or T > MAX_FRAMES or b * (T + 6) >= 1 << 31:
            raise ValueError(f"{b} clips of {T} frames are more than one launch takes")
        lens_list = None
        if lens is not None:
            lens_list = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
            if len(lens_list) != b or any(not 2 <= v <= T for v in lens_list):
                raise ValueError(f"lens must be {b} integers in 2 .. T={T}, got {lens_list}")
        n_out = (T - 1) * self.hop
        w = self._weights()
        x = x.to(self.dev, torch.float32).contiguous()
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (b, n_out) or out.dtype != torch.float32
                                or out.device != x.device or out.stride(1) != 1 or (b > 1 and out.stride(0) < n_out)):
            raise ValueError(f"out must be a ({b}, {n_out}) fp32 tensor on {x.device} with unit stride along time and rows that do not overlap")
        buf = self._buffers(b, T)
        if out is None:
            out = torch.empty(b, n_out, dtype=torch.float32, device=self.dev) if lens_list is None else \
                torch.zeros(b, n_out, dtype=torch.float32, device=self.dev)
        lens_dev = None if lens_list is None else torch.tensor(lens_list, dtype=torch.int32, device=self.dev)
        P, M = buf["P"], buf["M"]

        def tap(name, t, width):
            if taps is not None:
                full = torch.zeros(b * P, t.shape[1], dtype=torch.float32, device=self.dev)
                full[:M] = t
                taps[name] = full.view(b, P, -1)[:, :T, :width].clone()

        with torch.cuda.device(self.dev):
            self._stage_in(x, lens_dev, buf, b, T)
            self._stage_embed(buf)
            tap("embed", buf["x"][0], self.dim)
            src = 0
            for i, blk in enumerate(w["blocks"]):
                self._stage_block(blk, buf, lens_dev, b, T, src)
                src = 1 - src
                tap(f"block{i}", buf["x"][src], self.dim)
            logits = self._stage_head(buf, src)
            tap("final", buf["y"], self.dim)
            tap("logits", logits, self.n_fft + 2)
            self._stage_spectrum(logits, buf)
            tap("S", buf["spec"], 2 * self.n_bins)
            frames = self._stage_idft(buf)
            self._stage_overlap_add(frames, buf, lens_dev, b, T, out)
        if taps is not None:
            taps["S"] = taps["S"].view(b, T, self.n_bins, 2)
            taps["wave"] = out.clone()
        if lens_list is None:
            return out
        return [out[i, :(n - 1) * self.hop] for i, n in enumerate(lens_list)]

    __call__ = decode
