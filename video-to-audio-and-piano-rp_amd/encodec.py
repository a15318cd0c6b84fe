"""Encodec 24 kHz decoder (the vocoder) and encoder on the MI355X kernels.

Mirrors `EncodecWrapper.decode` (src/e2_tts_pytorch/e2_tts_crossatt3.py:434-437): `self.model.decoder(emb)` then
`output[0]`, called on the sampler's latents at predict.py:277-278.  The network is the SEANet decoder of
`transformers.models.encodec` (reference pin transformers==4.46.0): Conv1d(128->512, k7), 2-layer LSTM + skip, four
[ELU, ConvTranspose1d(k = 2r, stride r), residual block] stages for r = 8, 5, 4, 2, ELU, Conv1d(32->1, k7); all
convolutions causal and weight-normalised.  750 latent frames -> 240 000 samples.

Design: activations are time-major [T][C] fp32.  A causal Conv1d(k) is then ONE `v2a_gemm` whose A rows overlap
(lda = C, K = k*C) over a buffer with k-1 reflected rows in front; a ConvTranspose1d(k = 2r, stride r) is ONE `v2a_gemm`
with A row q = [x[q-1], x[q]] (K = 2C) and N = r*Cout columns ordered (phase, channel), whose [L][r*Cout] output is the
up-sampled [L*r][Cout] signal in place -- no col2im, no scatter.  `v2a_elu_pad` applies ELU and writes the pad rows in one
pass; `v2a_lstm2` runs both LSTM layers' recurrences in one persistent kernel (weights in registers, T + 1 exchange steps).  Weight norm is
resolved at load time.  Everything is fp32 (exact-fp32 MFMA): the whole decoder is ~30 GFLOP, memory- and latency-bound.
There is no CPU fallback: without libv2a_cfm.so every call raises.

`EncodecEncoder` is the mirror (`EncodecWrapper.forward`, x3:428-432, predict.py:222): Conv1d(1->32, k7), four [residual block, ELU,
Conv1d(k = 2r, stride r)] stages for r = 2, 4, 5, 8, the LSTM, ELU, Conv1d(512->128, k7).  A strided convolution is ONE `v2a_gemm`
whose A rows overlap with lda = r*C (K = k*C, M = ceil(T/r)) over a buffer that `v2a_elu_pad_lr` padded on both sides: the library
reflects k - r samples in front and, where the length is not a multiple of r, up to r - 1 behind (`encoder_padding_plan`).  The
wide, thin end -- stem + the C = 32 block over 240 000 time steps -- is one fused VALU kernel (`v2a_encodec_stage0`);
`fused_stem=False` keeps the generic composition of it reachable for A/B runs.  What the two engines share -- buffers, the LSTM and the
convolution, the decoder's being the encoder's at stride 1 -- is `_SEANet`; each calls its own pad kernel.

`EncodecQuantizer` is the third part of `EncodecModel`, the residual vector quantizer between the two (`EncodecModel.encode` / `.decode`):
`v2a_encodec_rvq_encode` searches every stage's codebook in one launch (exact-fp32 MFMA scores, the residual in registers) and
`v2a_encodec_rvq_decode` sums the chosen codewords in the library's order; `rvq_encode_torch` / `rvq_decode_torch` restate the library for
host tests.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib as L

RATIOS = (8, 5, 4, 2)
HIDDEN, FILTERS = 128, 32


def expected_state_dict_shapes() -> dict[str, tuple]:
    """Key layout of `EncodecModel(EncodecConfig()).decoder.state_dict()` (weight_norm parametrisation)."""
    s: dict[str, tuple] = {}

    def conv(p, co, ci, k, transpose=False):
        s[f"{p}.conv.bias"] = (co,)
        s[f"{p}.conv.parametrizations.weight.original0"] = ((ci if transpose else co), 1, 1)
        s[f"{p}.conv.parametrizations.weight.original1"] = (ci, co, k) if transpose else (co, ci, k)

    c = FILTERS * 2 ** len(RATIOS)
    conv("layers.0", c, HIDDEN, 7)
    for l in range(2):
        s[f"layers.1.lstm.weight_ih_l{l}"] = (4 * c, c)
        s[f"layers.1.lstm.weight_hh_l{l}"] = (4 * c, c)
        s[f"layers.1.lstm.bias_ih_l{l}"] = (4 * c,)
        s[f"layers.1.lstm.bias_hh_l{l}"] = (4 * c,)
    idx = 3
    for r in RATIOS:
        conv(f"layers.{idx}", c // 2, c, 2 * r, transpose=True)
        c //= 2
        conv(f"layers.{idx + 1}.block.1", c // 2, c, 3)
        conv(f"layers.{idx + 1}.block.3", c, c // 2, 1)
        conv(f"layers.{idx + 1}.shortcut", c, c, 1)
        idx += 3
    conv(f"layers.{idx}", 1, FILTERS, 7)
    return s


def _resolve_weight(sd, p):
    """Plain `conv.weight`, the parametrised (original0 = g, original1 = v) pair, or the legacy weight_g / weight_v pair
    of the hub checkpoint: w = g * v / ||v|| with the norm over all dims but the first (torch weight_norm, dim 0)."""
    if f"{p}.conv.weight" in sd:
        return sd[f"{p}.conv.weight"].float()
    for gk, vk in ((f"{p}.conv.parametrizations.weight.original0", f"{p}.conv.parametrizations.weight.original1"),
                   (f"{p}.conv.weight_g", f"{p}.conv.weight_v")):
        if gk in sd and vk in sd:
            g, v = sd[gk].float(), sd[vk].float()
            return g * v / v.norm(dim=(1, 2), keepdim=True)
    raise KeyError(f"Encodec: no weight for {p}.conv (looked for .weight, parametrizations.weight.original0/1, weight_g/v)")


def conv_padding(length: int, k: int, stride: int = 1) -> tuple[int, int, int]:
    """(pad_left, pad_right, out_len) of a causal `EncodecConv1d(k, stride)` on `length` samples: k - stride reflected samples in
    front, and behind as many as make the last window full (`_get_extra_padding_for_conv1d`, in integers)."""
    pad_left = k - stride
    n_frames = -((length - k + pad_left) // -stride)              # ceil((length - k + pad_total) / stride + 1) - 1
    pad_right = n_frames * stride + k - pad_left - length
    return pad_left, pad_right, (length + pad_left + pad_right - k) // stride + 1


class _SEANet:
    """What the decoder and the encoder share: named fp32 buffers, the 2-layer LSTM (weight packing, launch, timeout check) and the
    causal convolution as one GEMM over overlapping rows.  The two differ in the kernel that pads: `_pad`."""

    def _load(self, state_dict, device, part):
        """Device, buffers and the state dict on the host, `part.` (decoder / encoder of an `EncodecModel`) stripped."""
        L.lib()                                                   # fail loudly without the HIP library
        self.dev = torch.device(device)
        self._bufs: dict = {}
        sd = {k: v.detach().cpu() for k, v in state_dict.items()}
        if any(k.startswith(f"{part}.layers.") for k in sd):
            sd = {k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(f"{part}.")}
        return sd

    def _f32(self, t):
        return t.float().contiguous().to(self.dev)

    def _load_lstm(self, sd, p, H):
        self.H = H
        self.lstm = []
        for l in range(2):
            self.lstm.append(dict(wih=self._f32(sd[f"{p}.lstm.weight_ih_l{l}"]), whh=self._f32(sd[f"{p}.lstm.weight_hh_l{l}"]),
                                  b=self._f32(sd[f"{p}.lstm.bias_ih_l{l}"].float() + sd[f"{p}.lstm.bias_hh_l{l}"].float())))
        self._ws = torch.zeros(8 * H + 2, dtype=torch.int32, device=self.dev)      # exchange tables of both LSTM layers + error flag

    def _buf(self, name, rows, C):
        key = (name, rows, C)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(rows, C, device=self.dev, dtype=torch.float32)
        return t

    def _conv(self, cv, src, T, name, *, act, resid=None):
        """Causal Conv1d(k, stride r) on time-major src (T, ci): ELU (optional) + reflect pads, then one GEMM over overlapping rows
        (lda = r*ci) -> (`conv_padding`'s out_len, co).  The decoder's convolutions have stride 1: k - 1 rows in front, none behind."""
        k, ci, co, r = cv["k"], cv["ci"], cv["co"], cv.get("r", 1)
        pl, pr, To = conv_padding(T, k, r)
        a = src
        if act or pl or pr:
            a = self._buf(name + ".in", T + pl + pr, ci)
            self._pad(src, a, T, ci, pl, pr, act)
        out = self._buf(name, To, co)
        L.gemm([(a, r * ci, k * ci)], cv["w"], out, M=To, N=co, compute=L.F32, bias=cv["b"], ldo=co,
               epilogue=L.EPI_RESID if resid is not None else L.EPI_STORE, resid=resid, ldr=co)
        return out

    def _lstm2(self, x, T):
        """2-layer LSTM + skip on x (T, H): one GEMM for layer 0's input projection, then both recurrences in one persistent kernel."""
        H = self.H
        l0, l1 = self.lstm
        gx = self._buf("gx0", T, 4 * H)
        L.gemm([(x, H, H)], l0["wih"], gx, M=T, N=4 * H, compute=L.F32, bias=l0["b"], ldo=4 * H)
        y = self._buf("lstm_out", T, H)
        L.lstm2(gx, l0["whh"], l1["wih"], l1["b"], l1["whh"], y, self._ws, T=T, H=H, resid=x)
        return y

    def _check_lstm(self):
        if int(self._ws[8 * self.H].item()):                                       # one host sync per clip
            raise L.V2AError("v2a_lstm2: a workgroup timed out at the step barrier (GPU oversubscribed?); result discarded")


class EncodecDecoder(_SEANet):
    """HIP mirror of `EncodecWrapper.decode` / `EncodecModel.decoder`.

    state_dict: an `EncodecModel` state dict (keys `decoder.layers...`) or the decoder's own (`layers...`)."""

    def __init__(self, state_dict, device="cuda:0"):
        sd = self._load(state_dict, device, "decoder")
        f32 = self._f32

        def conv(p):
            w = _resolve_weight(sd, p)                            # (co, ci, k)
            co, ci, k = w.shape
            return dict(w=f32(w.permute(0, 2, 1).reshape(co, k * ci)), b=f32(sd[f"{p}.conv.bias"]), co=co, ci=ci, k=k)

        def convt(p):
            w = _resolve_weight(sd, p)                            # (ci, co, k = 2r)
            ci, co, k = w.shape
            r = k // 2
            assert k == 2 * r
            # row (phase, co); columns [x[q-1] part: tap phase + r | x[q] part: tap phase]
            wp = torch.cat([w[:, :, r:].permute(2, 1, 0), w[:, :, :r].permute(2, 1, 0)], 2).reshape(r * co, 2 * ci)
            return dict(w=f32(wp), b=f32(sd[f"{p}.conv.bias"].float().repeat(r)), co=co, ci=ci, r=r)

        self.c0 = conv("layers.0")
        self._load_lstm(sd, "layers.1", self.c0["co"])
        self.stages = []
        idx = 3
        for r in RATIOS:
            self.stages.append(dict(up=convt(f"layers.{idx}"), b1=conv(f"layers.{idx + 1}.block.1"), b3=conv(f"layers.{idx + 1}.block.3"),
                                    sc=conv(f"layers.{idx + 1}.shortcut")))
            assert self.stages[-1]["up"]["r"] == r
            idx += 3
        self.cf = conv(f"layers.{idx}")
        self.hop = math.prod(RATIOS)

    def _pad(self, src, a, T, C, pl, pr, act):
        assert pr == 0                                             # stride 1: k - 1 reflected rows in front, none behind
        L.elu_pad(src, a, T=T, C_=C, pad=pl, reflect=True, act=act)

    def _decode_one(self, emb, taps=None):
        """emb (128, T) on the device -> waveform (T * 320,)."""
        T = emb.shape[1]
        x0 = emb.t().contiguous()                                                  # time-major (T, 128)
        x = self._lstm2(self._conv(self.c0, x0, T, "c0", act=False), T)
        if taps is not None:
            taps["lstm"] = x.t().clone()
        Lc, C = T, self.H
        for si, st in enumerate(self.stages):
            up = st["up"]
            r, co = up["r"], up["co"]
            a = self._buf(f"s{si}.upin", Lc + 1, C)
            L.elu_pad(x, a, T=Lc, C_=C, pad=1, reflect=False, act=True)
            u = self._buf(f"s{si}.up", Lc, r * co)                                  # == (Lc * r, co) time-major
            L.gemm([(a, C, 2 * C)], up["w"], u, M=Lc, N=r * co, compute=L.F32, bias=up["b"], ldo=r * co)
            Lc, C = Lc * r, co
            u = u.view(Lc, C)
            h1 = self._conv(st["b1"], u, Lc, f"s{si}.b1", act=True)
            h2 = self._conv(st["b3"], h1, Lc, f"s{si}.b3", act=True)
            x = self._conv(st["sc"], u, Lc, f"s{si}.out", act=False, resid=h2)
            if taps is not None:
                taps[f"stage{r}"] = x.t().clone()
        wav = self._conv(self.cf, x, Lc, "final", act=True)                         # (Lc, 1)
        return wav.view(Lc)

    @torch.no_grad()
    def decoder(self, emb, taps=None):
        """`EncodecModel.decoder(emb)`: emb (b, 128, T) -> (b, 1, 320*T) fp32 on the device."""
        assert emb.ndim == 3 and emb.shape[1] == HIDDEN, f"emb must be (b, {HIDDEN}, T), got {tuple(emb.shape)}"
        if emb.shape[2] < 7:
            raise ValueError("EncodecDecoder: need at least 7 latent frames (reflect padding of the k=7 convolutions)")
        emb = emb.to(self.dev, torch.float32)
        out = torch.empty(emb.shape[0], 1, emb.shape[2] * self.hop, device=self.dev, dtype=torch.float32)
        for i in range(emb.shape[0]):
            out[i, 0].copy_(self._decode_one(emb[i], taps if i == 0 else None))
            self._check_lstm()
        return out

    def decode(self, emb):
        """`EncodecWrapper.decode(emb)` (x3:434-437): the first clip's waveform, shape (1, samples)."""
        return self.decoder(emb)[0]


# ---- encoder -----------------------------------------------------------------------------------------------------------
MIN_FRAMES = 7          # the final k7 convolution reflects 6 frames; below that the library zero-extends first (not mirrored here)


def expected_encoder_state_dict_shapes() -> dict[str, tuple]:
    """Key layout of `EncodecModel(EncodecConfig()).encoder.state_dict()` (weight_norm parametrisation)."""
    s: dict[str, tuple] = {}

    def conv(p, co, ci, k):
        s[f"{p}.conv.bias"] = (co,)
        s[f"{p}.conv.parametrizations.weight.original0"] = (co, 1, 1)
        s[f"{p}.conv.parametrizations.weight.original1"] = (co, ci, k)

    c = FILTERS
    conv("layers.0", c, 1, 7)
    idx = 1
    for r in reversed(RATIOS):
        conv(f"layers.{idx}.block.1", c // 2, c, 3)
        conv(f"layers.{idx}.block.3", c, c // 2, 1)
        conv(f"layers.{idx}.shortcut", c, c, 1)
        conv(f"layers.{idx + 2}", 2 * c, c, 2 * r)
        c *= 2
        idx += 3
    for l in range(2):
        s[f"layers.{idx}.lstm.weight_ih_l{l}"] = (4 * c, c)
        s[f"layers.{idx}.lstm.weight_hh_l{l}"] = (4 * c, c)
        s[f"layers.{idx}.lstm.bias_ih_l{l}"] = (4 * c,)
        s[f"layers.{idx}.lstm.bias_hh_l{l}"] = (4 * c,)
    conv(f"layers.{idx + 2}", HIDDEN, c, 7)
    return s


def encoder_padding_plan(n: int) -> list[tuple[str, int, int, int]]:
    """(conv prefix, pad_left, pad_right, out_len) of every convolution of the encoder, in execution order, for n samples: `conv_padding`,
    which the engine sizes every buffer and launch with, walked over the stack."""
    plan = []
    T = n

    def add(p, k, stride=1):
        nonlocal T
        pl, pr, T = conv_padding(T, k, stride)
        plan.append((p, pl, pr, T))

    add("layers.0", 7)
    idx = 1
    for r in reversed(RATIOS):
        add(f"layers.{idx}.block.1", 3)
        add(f"layers.{idx}.block.3", 1)
        add(f"layers.{idx}.shortcut", 1)
        add(f"layers.{idx + 2}", 2 * r, r)
        idx += 3
    add(f"layers.{idx + 2}", 7)
    return plan


def encoder_frames(n: int) -> int:
    """Latent frames of n samples, ceil(n / 320); ValueError below MIN_FRAMES (n < 1 921), the decoder's limit too."""
    hop = math.prod(RATIOS)
    T = -(-int(n) // hop)
    if T < MIN_FRAMES:
        raise ValueError(f"EncodecEncoder: {n} samples give {T} latent frames, need at least {MIN_FRAMES} "
                         f"({(MIN_FRAMES - 1) * hop + 1} samples: reflect padding of the k=7 convolutions)")
    return T


class EncodecEncoder(_SEANet):
    """HIP mirror of `EncodecWrapper.forward` / `EncodecModel.encoder` (no quantizer).

    state_dict: an `EncodecModel` state dict (keys `encoder.layers...`) or the encoder's own (`layers...`).
    fused_stem: layers 0 and 1 in the one-pass `v2a_encodec_stage0` kernel; False composes them from `v2a_gemm` / `v2a_elu_pad_lr`
    like the later stages (the stem as a GEMM over a zero-padded K = 16 patch buffer) -- kept for A/B timing and value comparison."""

    def __init__(self, state_dict, device="cuda:0", fused_stem=True):
        sd = self._load(state_dict, device, "encoder")
        self.fused_stem = bool(fused_stem)
        f32 = self._f32

        def conv(p, stride=1):
            w = _resolve_weight(sd, p)                            # (co, ci, k)
            co, ci, k = w.shape
            # w3 / b_cpu: the resolved (co, ci, k) weight and the bias on the host -- the stage-0 parameter block is packed from them
            return dict(w=f32(w.permute(0, 2, 1).reshape(co, k * ci)), b=f32(sd[f"{p}.conv.bias"]), co=co, ci=ci, k=k, r=stride, w3=w,
                        b_cpu=sd[f"{p}.conv.bias"].float())

        self.stem = conv("layers.0")
        assert (self.stem["ci"], self.stem["k"]) == (1, 7)
        self.stem["w"] = f32(F.pad(self.stem["w3"][:, 0], (0, 16 - 7)))           # (32, 16): K padded to the GEMM's granule
        self.stages = []
        idx = 1
        for r in reversed(RATIOS):
            self.stages.append(dict(b1=conv(f"layers.{idx}.block.1"), b3=conv(f"layers.{idx}.block.3"), sc=conv(f"layers.{idx}.shortcut"),
                                    down=conv(f"layers.{idx + 2}", r)))
            assert self.stages[-1]["down"]["k"] == 2 * r
            idx += 3
        self.cf = conv(f"layers.{idx + 2}")
        self._load_lstm(sd, f"layers.{idx}", self.cf["ci"])
        self.hop = math.prod(RATIOS)
        s0 = self.stages[0]
        # parameter block of v2a_encodec_stage0 (include/v2a_cfm.h)
        self.stage0 = f32(torch.cat([self.stem["w3"].reshape(-1), self.stem["b_cpu"], s0["sc"]["w3"].reshape(-1),
                                     s0["sc"]["b_cpu"] + s0["b3"]["b_cpu"], s0["b1"]["w3"].permute(0, 2, 1).reshape(-1), s0["b1"]["b_cpu"],
                                     s0["b3"]["w3"].reshape(-1)]))
        assert self.stage0.numel() == L.ENCODEC_STAGE0_PARAMS

    def _pad(self, src, a, T, C, pl, pr, act):
        L.elu_pad_lr(src, a, T=T, C_=C, pad_left=pl, pad_right=pr, act=act)

    def _resblock(self, st, x, T, name):
        h1 = self._conv(st["b1"], x, T, name + ".b1", act=True)
        h2 = self._conv(st["b3"], h1, T, name + ".b3", act=True)
        return self._conv(st["sc"], x, T, name + ".out", act=False, resid=h2)

    def _stage0(self, wave, n):
        """Layers 0 and 1: wave (n,) -> (n, 32) time-major."""
        out = self._buf("s0.out", n, FILTERS)
        if self.fused_stem:
            L.encodec_stage0(wave, self.stage0, out, n=n)
            return out
        # composed form: the stem's 7-tap patches in a zero-padded (n, 16) buffer, then the generic path
        patches = self._buf("stem.in", n, 16)
        patches.zero_()
        patches[:, :7].copy_(F.pad(wave.view(1, 1, n), (6, 0), mode="reflect").view(-1).unfold(0, 7, 1))
        x0 = self._buf("stem", n, FILTERS)
        L.gemm([(patches, 16, 16)], self.stem["w"], x0, M=n, N=FILTERS, compute=L.F32, bias=self.stem["b"], ldo=FILTERS)
        return self._resblock(self.stages[0], x0, n, "s0")

    def _encode_one(self, wave, taps=None):
        """wave (n,) fp32 on the device -> latent (128, ceil(n / 320))."""
        n = wave.shape[0]
        x = self._stage0(wave, n)
        T = n
        if taps is not None:
            taps["layer1"] = x.t().clone()
        for si, st in enumerate(self.stages):
            if si:
                x = self._resblock(st, x, T, f"s{si}")
            x = self._conv(st["down"], x, T, f"s{si}.down", act=True)
            T = x.shape[0]
            if taps is not None:
                taps[f"layer{3 * si + 3}"] = x.t().clone()
        y = self._lstm2(x, T)
        if taps is not None:
            taps["layer13"] = y.t().clone()
        z = self._conv(self.cf, y, T, "final", act=True)                           # (T, 128)
        return z.t().contiguous()

    @torch.no_grad()
    def encode_list(self, waves, taps=None):
        """Ragged lengths: a list of 1-D waves -> a list of (128, ceil(n_i / 320)) latents on the device, one clip at a time."""
        lens = [encoder_frames(w.shape[-1]) for w in waves]                         # refuse before any launch
        out = []
        for i, (w, T) in enumerate(zip(waves, lens)):
            assert w.ndim == 1, f"encode_list takes 1-D waves, got {tuple(w.shape)}"
            z = self._encode_one(w.to(self.dev, torch.float32).contiguous(), taps if i == 0 else None)
            assert z.shape == (HIDDEN, T), (tuple(z.shape), T)
            out.append(z)
            self._check_lstm()
        return out

    def encoder(self, wave, taps=None):
        """`EncodecModel.encoder(wave)`: wave (b, 1, n) -> (b, 128, ceil(n / 320)) fp32 on the device."""
        assert wave.ndim == 3 and wave.shape[1] == 1, f"wave must be (b, 1, n), got {tuple(wave.shape)}"
        return torch.stack(self.encode_list([wave[i, 0] for i in range(wave.shape[0])], taps))

    def forward(self, waveform):
        """`EncodecWrapper.forward(waveform)` (x3:428-432): waveform (channels, n); the processor is handed `waveform[0]` and, for
        this model, neither normalises nor chunks it -> (1, 128, T)."""
        assert waveform.ndim == 2, f"waveform must be (channels, n), got {tuple(waveform.shape)}"
        return self.encoder(waveform[:1].unsqueeze(0))

    __call__ = forward


# ---- residual vector quantizer -----------------------------------------------------------------------------------------
FRAME_RATE = 75                                     # EncodecConfig().frame_rate: 24 000 / 320
RVQ_CODEBOOK_MULTIPLE = 512                         # v2a_encodec_rvq_encode: 8 waves x 64 codewords per pass


def quantizer_codebooks(state_dict) -> torch.Tensor:
    """(S, codebook_size, dim) fp32 from an `EncodecModel` state dict (`quantizer.layers.{i}.codebook.embed`) or the quantizer's own
    (`layers.{i}.codebook.embed`); `cluster_size`, `embed_avg` and `inited` (training statistics) are not read."""
    sd = state_dict
    if any(k.startswith("quantizer.layers.") for k in sd):
        sd = {k[len("quantizer."):]: v for k, v in sd.items() if k.startswith("quantizer.")}
    books = []
    while f"layers.{len(books)}.codebook.embed" in sd:
        books.append(sd[f"layers.{len(books)}.codebook.embed"].detach().cpu().float())
    if not books:
        raise KeyError("EncodecQuantizer: no `layers.0.codebook.embed` (or `quantizer.layers.0.codebook.embed`) in the state dict")
    if any(b.ndim != 2 or b.shape != books[0].shape for b in books):
        raise ValueError(f"EncodecQuantizer: codebooks of different shapes: {sorted({tuple(b.shape) for b in books})}")
    return torch.stack(books).contiguous()


def num_quantizers_for_bandwidth(bandwidth, codebook_size: int, num_quantizers: int, frame_rate: int = FRAME_RATE) -> int:
    """`EncodecResidualVectorQuantizer.get_num_quantizers_for_bandwidth`: kbps -> stages; None or 0 means all of them.  As the
    library's, the count is not capped at `num_quantizers`: slicing the layer list caps it there, the callers below do."""
    if bandwidth is None or not bandwidth > 0.0:
        return num_quantizers
    return int(max(1, math.floor(bandwidth * 1000 / (math.log2(codebook_size) * frame_rate))))


def rvq_encode_torch(codebooks, x, n_q=None):
    """Plain-torch restatement of `EncodecResidualVectorQuantizer.encode`, operation for operation, in the dtype of `x`: codebooks
    (S, Kc, D), x (b, D, t) -> int64 (n_q, b, t).  For host tests: the device path is `EncodecQuantizer.encode`."""
    n_q = codebooks.shape[0] if n_q is None else n_q
    residual = x
    out = []
    for s in range(n_q):
        embed = codebooks[s].to(x.dtype)
        h = residual.permute(0, 2, 1)
        flat = h.reshape(-1, h.shape[-1])
        et = embed.t()
        dist = -(flat.pow(2).sum(1, keepdim=True) - 2 * flat @ et + et.pow(2).sum(0, keepdim=True))
        ind = dist.max(dim=-1).indices.view(*h.shape[:-1])
        residual = residual - F.embedding(ind, embed).permute(0, 2, 1)
        out.append(ind)
    return torch.stack(out)


def rvq_decode_torch(codebooks, codes, dtype=torch.float32):
    """Plain-torch restatement of `EncodecResidualVectorQuantizer.decode`: codes (n_q, b, t) -> (b, D, t), the stages summed in order
    from 0.0 in `dtype`."""
    out = torch.full((), 0.0, dtype=dtype)
    for s, ind in enumerate(codes):
        out = out + F.embedding(ind.long(), codebooks[s].to(dtype)).permute(0, 2, 1)
    return out


class EncodecQuantizer:
    """HIP mirror of `EncodecModel.quantizer` (`EncodecResidualVectorQuantizer`): `encode` is the library's `quantizer.encode`
    (latents -> codes), `decode` its `quantizer.decode` (codes -> latents).

    state_dict: an `EncodecModel` state dict (keys `quantizer.layers.{i}.codebook.embed`) or the quantizer's own."""

    def __init__(self, state_dict, device="cuda:0"):
        cb = quantizer_codebooks(state_dict)
        self.num_quantizers, self.codebook_size, self.dim = cb.shape
        if self.dim != HIDDEN or self.codebook_size % RVQ_CODEBOOK_MULTIPLE:
            raise ValueError(f"EncodecQuantizer: codebooks of {self.codebook_size} x {self.dim}; the kernel takes dimension {HIDDEN} and "
                             f"a codebook size that is a multiple of {RVQ_CODEBOOK_MULTIPLE}")
        L.lib()                                                   # fail loudly without the HIP library
        self.dev = dev = torch.device(device)
        self.codebooks = cb.to(dev)
        self.norms = cb.double().pow(2).sum(-1).float().to(dev)   # |e_j|^2, summed in float64 and rounded once

    def num_quantizers_for_bandwidth(self, bandwidth=None) -> int:
        return min(self.num_quantizers, num_quantizers_for_bandwidth(bandwidth, self.codebook_size, self.num_quantizers))

    def _frames(self, shape, strides, channels_last, what):
        """(B, T, (batch, frame, channel) strides) of a 3-D tensor in either layout; the channel axis must be the codebook dimension."""
        if len(shape) != 3 or shape[2 if channels_last else 1] != self.dim:
            raise ValueError(f"EncodecQuantizer.{what}: expected {'(b, t, %d)' % self.dim if channels_last else '(b, %d, t)' % self.dim}, "
                             f"got {tuple(shape)}")
        b, c, t = (0, 2, 1) if channels_last else (0, 1, 2)
        return shape[b], shape[t], (strides[b], strides[t], strides[c])

    @torch.no_grad()
    def encode(self, x, bandwidth=None, channels_last=False):
        """x float32 (b, 128, t) -- or (b, t, 128) with channels_last -- read in place through its strides -> int64 (n_q, b, t) on the
        device, `EncodecResidualVectorQuantizer.encode(x, bandwidth)`; `EncodecModel.encode`'s audio_codes[0] is its transpose(0, 1)."""
        if not (torch.is_tensor(x) and x.is_floating_point()):
            raise ValueError("EncodecQuantizer.encode: a float tensor of latents is expected")
        B, T, _ = self._frames(x.shape, x.stride(), channels_last, "encode")
        n_q = self.num_quantizers_for_bandwidth(bandwidth)
        codes = torch.empty(n_q, B, T, dtype=torch.int64, device=self.dev)
        if B * T == 0:
            return codes
        x = x.to(self.dev, torch.float32)
        if any(s < 0 for s in x.stride()):
            x = x.contiguous()
        _, _, strides = self._frames(x.shape, x.stride(), channels_last, "encode")
        L.encodec_rvq_encode(x, strides, self.codebooks, self.norms, codes, B=B, T=T, n_q=n_q)
        return codes

    @torch.no_grad()
    def decode(self, codes, channels_last=False):
        """codes integer (n_q, b, t), the first n_q stages -> float32 (b, 128, t), or (b, t, 128) with channels_last:
        `EncodecResidualVectorQuantizer.decode(codes)`.  An index outside [0, codebook_size) is a ValueError before any launch."""
        if not torch.is_tensor(codes) or codes.is_floating_point() or codes.is_complex() or codes.dtype == torch.bool or codes.ndim != 3:
            raise ValueError("EncodecQuantizer.decode: an integer tensor (n_q, b, t) is expected")
        n_q, B, T = codes.shape
        if not 1 <= n_q <= self.num_quantizers:
            raise ValueError(f"EncodecQuantizer.decode: {n_q} stages of codes, the quantizer has {self.num_quantizers}")
        if codes.numel() and (int(codes.min()) < 0 or int(codes.max()) >= self.codebook_size):
            raise ValueError(f"EncodecQuantizer.decode: codes outside [0, {self.codebook_size})")
        out = torch.empty((B, T, self.dim) if channels_last else (B, self.dim, T), dtype=torch.float32, device=self.dev)
        if B * T == 0:
            return out
        codes = codes.to(self.dev, torch.int64).contiguous()
        _, _, strides = self._frames(out.shape, out.stride(), channels_last, "decode")
        L.encodec_rvq_decode(codes, self.codebooks, out, strides, B=B, T=T, n_q=n_q)
        return out
