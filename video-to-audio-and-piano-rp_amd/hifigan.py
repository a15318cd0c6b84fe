"""The HiFi-GAN vocoder on the device: 64-bin mel frames -> 16 kHz waves, the `decode_to_waveform` half of the reference's third
`self.vocos` (`'vae'`, x3:1404-1409; `VaeWrapper.decode`, x3:470-490).  The other half, `decode_first_stage` (the AudioLDM VAE decoder),
is not built.  The network is `Generator(HIFIGAN_16K_64)` of src/audioldm/hifigan/models.py under `vocoder_infer` (utilities.py:76-86):

    x = conv_pre(mel)                                                        Conv1d(num_mels, C0, 7, padding=3)
    per stage i:  x = ups[i](leaky_relu(x, 0.1))                             ConvTranspose1d(C, C / 2, k_i, u_i, padding=(k_i - u_i) // 2)
                  x = ((r_0(x) + r_1(x)) + r_2(x)) / 3                       ResBlocks of kernel 3, 7, 11: three rounds of
                                                                             x = c2(leaky_relu(c1(leaky_relu(x, 0.1)), 0.1)) + x, c1 dilated 1, 3, 5
    wave = tanh(conv_post(leaky_relu(x, 0.01)))                              Conv1d(C, 1, 7, padding=3); the last slope is F.leaky_relu's default

A transposed convolution gives (L - 1) u - 2 p + k = u L + (k - u) % 2 frames: the shipped k = 16, u = 5 gives 5 L + 1, the whole network
160 T + 32 samples (`output_length`).

Layout: activations are time-major fp32 rows (frames, C); frame t of clip b at stage s is row b * P_s + t with P_s = u_s P_(s-1), so that
the (frames, u C_out) output of a polyphase transposed-convolution GEMM IS the up-sampled (u frames, C_out) signal, for every clip of the
batch at once.  P_0 = T + 2 HALO leaves room for the zero halo of every operand buffer at every stage.  The launches of a call
(csrc/hifigan.hip, include/v2a_cfm.h):
  * `v2a_hifigan_act_pad` makes every GEMM operand: the sum of one to three sources in a fixed order, the MRF mean's division, the leaky
    ReLU, and zero rows around every clip's own length.
  * An undilated convolution is an exact-fp32 `v2a_gemm` over overlapping rows (lda = C, K = k C); a dilated one reads tap j as the A
    segment (a + j d C, lda = C, ka = C), up to three per launch; a transposed one is a GEMM against `polyphase_weight`.  Every GEMM's K is cut
    into launches of at most K_CHUNK columns, launch c added to the sum of the launches before it through the RESID epilogue in place
    (`conv_launches`): the exact-fp32 GEMM adds the K products of a launch in one fp32 chain whose error grows with K (vocos.py).
  * With fused=True the convolutions of the stages with C in FUSED_CHANNELS run on `v2a_hifigan_conv` instead, a direct dilated convolution
    that applies the leaky ReLU and the zero padding while it stages its input tile: no operand buffer, one launch per convolution.
  * `v2a_hifigan_post`: conv_post, tanh, and the fp32 wave or `vocoder_infer`'s truncating int16.
One arithmetic mode, fp32 throughout.  A clip's bits depend on its own frames alone.  There is no CPU fallback."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib as L

HIFIGAN_16K_64 = dict(num_mels=64, upsample_initial_channel=1024, upsample_rates=(5, 4, 2, 2, 2), upsample_kernel_sizes=(16, 16, 8, 4, 4),
                      resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
LRELU_SLOPE, POST_SLOPE = 0.1, 0.01          # models.py:7; F.leaky_relu's default in front of conv_post (models.py:174)
# K of one GEMM launch.  Measured at T = 1000 (profiles/hifigan.txt): 128 / 256 / 512 / 1024 give 24.7 / 20.1 / 17.5 / 16.0 ms per clip and a
# largest tap error of 0.85 / 1.16 / 1.61 / 1.65 error scales (the tests allow 4); Vocos found 4.5 at K = 1536 (vocos.py K_CHUNK).
K_CHUNK = 512
TILE = 128                                   # V2A_HIFIGAN_TILE: frames of a workgroup of v2a_hifigan_conv
FUSED_CHANNELS = (32, 64, 128)               # widths v2a_hifigan_conv takes
LDS_HALF_CU = 80 * 1024                      # above this a tile of v2a_hifigan_conv leaves room for one workgroup per CU, not two


def fused_default(C: int, k: int, d: int) -> bool:
    """Whether fused=True runs Conv1d(C, C, k, dilation d) on v2a_hifigan_conv: where it was measured faster than the composition
    (profiles/hifigan.txt).  That is every shape of the three widths but those whose tile, (TILE + (k - 1) d) rows of C + 4 floats,
    passes half a CU's LDS -- at C = 128 the spans (k - 1) d >= 30: (7, 5), (11, 3), (11, 5), where one workgroup fits a CU instead of two
    and the direct kernel took 0.99 - 1.12 times the composition's time; those stay on the composition."""
    return C in FUSED_CHANNELS and (TILE + (k - 1) * d) * (C + 4) * 4 <= LDS_HALF_CU
PREFIXES = ("first_stage_model.vocoder.", "vocoder.")


def expected_state_dict_shapes(config: dict = HIFIGAN_16K_64) -> dict:
    """Key -> shape of `Generator(h).state_dict()` after `remove_weight_norm()`; with weight norm in place every `.weight` is a
    `.weight_g` (first dim, 1, 1) / `.weight_v` pair instead, which the constructor folds."""
    c0, mels = int(config["upsample_initial_channel"]), int(config["num_mels"])
    rates, uks = tuple(config["upsample_rates"]), tuple(config["upsample_kernel_sizes"])
    rks, dil = tuple(config["resblock_kernel_sizes"]), tuple(tuple(d) for d in config["resblock_dilation_sizes"])
    assert len(rates) == len(uks)
    s = {"conv_pre.bias": (c0,), "conv_pre.weight": (c0, mels, 7)}       # the module's own order: bias in front of the re-registered weight
    for i, k in enumerate(uks):
        s[f"ups.{i}.bias"], s[f"ups.{i}.weight"] = (c0 >> (i + 1),), (c0 >> i, c0 >> (i + 1), k)
    for i in range(len(uks)):
        c = c0 >> (i + 1)
        for j, rk in enumerate(rks):
            for part in ("convs1", "convs2"):
                for m in range(len(dil[j])):
                    p = f"resblocks.{i * len(rks) + j}.{part}.{m}"
                    s[p + ".bias"], s[p + ".weight"] = (c,), (c, c, rk)
    s["conv_post.bias"], s["conv_post.weight"] = (1,), (1, c0 >> len(uks), 7)
    return s


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g v / ||v||, the norm over every dim but the first (torch weight_norm, dim 0), in float64."""
    g, v = g.double(), v.double()
    return g * v / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.ndim - 1)))


def _resolve_weight(sd, p):
    """float64 `p.weight`: plain, the legacy weight_g / weight_v pair, or the parametrised original0 / original1 pair."""
    if p + ".weight" in sd:
        return sd[p + ".weight"].double()
    for gk, vk in ((p + ".weight_g", p + ".weight_v"), (p + ".parametrizations.weight.original0", p + ".parametrizations.weight.original1")):
        if gk in sd and vk in sd:
            if sd[gk].ndim != sd[vk].ndim or sd[gk].shape[0] != sd[vk].shape[0]:
                raise ValueError(f"HiFiGAN: {gk} has shape {tuple(sd[gk].shape)} beside {vk} of shape {tuple(sd[vk].shape)}")
            return fold_weight_norm(sd[gk], sd[vk])
    raise ValueError(f"HiFiGAN: missing key {p}.weight (or its weight_g / weight_v pair)")


class ConvTPlan(NamedTuple):
    """ConvTranspose1d(k, stride u, padding p = (k - u) // 2) in polyphase form: output block q (frames u q .. u q + u - 1) reads the
    `taps` input frames q - s_max .. q - s_max + taps - 1; L frames give u L + extra, in L + extra blocks."""
    k: int
    u: int
    p: int
    s_max: int
    taps: int
    extra: int

    def out_len(self, n: int) -> int:
        return self.u * n + self.extra

    @property
    def reach(self) -> int:                                   # zero rows the window needs on either side of a clip
        return max(self.s_max, self.taps - 1 - self.s_max)


def convt_plan(k: int, u: int) -> ConvTPlan:
    """Output frame o = u q + r gets x[i] w[j] with j = o + p - u i = u (q - i) + r + p; 0 <= j < k for some phase r < u bounds
    s = q - i to -((p + u - 1) // u) .. (k - 1 - p) // u, all in integers."""
    k, u = int(k), int(u)
    if u < 1 or k < u:
        raise ValueError(f"a transposed convolution of kernel {k} and stride {u} has no polyphase plan (1 <= stride <= kernel)")
    p = (k - u) // 2
    s_min, s_max = -((p + u - 1) // u), (k - 1 - p) // u
    return ConvTPlan(k, u, p, s_max, s_max - s_min + 1, (k - u) % 2)


def polyphase_weight(w: torch.Tensor, u: int) -> torch.Tensor:
    """w (ci, co, k) of a ConvTranspose1d -> (u co, taps ci) in w's dtype: row r co + o, column t ci + i = w[i][o][u (s_max - t) + r + p],
    zero where that tap falls outside [0, k)."""
    ci, co, k = w.shape
    pl = convt_plan(k, u)
    out = torch.zeros(u, co, pl.taps, ci, dtype=w.dtype)
    for r in range(u):
        for t in range(pl.taps):
            j = u * (pl.s_max - t) + r + pl.p
            if 0 <= j < k:
                out[r, :, t, :] = w[:, :, j].t()
    return out.reshape(u * co, pl.taps * ci)


def conv_launches(k: int, d: int, C: int, k_chunk: int = K_CHUNK) -> list:
    """The GEMM launches of Conv1d(C, *, k, dilation d) over a zero-padded time-major buffer: a list of launches, each a list of A
    segments (offset, ka).  `offset` counts floats from the row base, frame t - (k - 1) d / 2 of output frame t; lda = C.  The weight
    matrix is (co, k C) with column j C + c = w[co][c][j], and the segments of all launches, in order, walk its columns once.
    d == 1: the k taps are K = k C contiguous floats, cut into launches of k_chunk.  d > 1: tap j is the segment (j d C, C), cut at
    k_chunk where C is wider; up to three segments and k_chunk columns go into a launch."""
    if d == 1:
        return [[(k0, min(k_chunk, k * C - k0))] for k0 in range(0, k * C, k_chunk)]
    pieces = [(j * d * C + c0, min(k_chunk, C - c0)) for j in range(k) for c0 in range(0, C, k_chunk)]
    out, cur = [], []
    for piece in pieces:
        if cur and (len(cur) == 3 or sum(n for _, n in cur) + piece[1] > k_chunk):
            out.append(cur)
            cur = []
        cur.append(piece)
    out.append(cur)
    return out


def pack_conv_fragments(w: torch.Tensor) -> torch.Tensor:
    """w (C, C, k) fp32 -> the k C C floats v2a_hifigan_conv reads: float 4 i + e with i = ((j C / 16 + kq) C / 16 + n) 64 + lane is
    w[16 n + (lane & 15)][16 kq + 4 e + (lane >> 4)][j], the A operand of the MFMA's k step 4 kq + e for output tile n."""
    co, ci, k = w.shape
    assert co == ci and co % 16 == 0
    nt = co // 16
    v = w.permute(2, 0, 1).reshape(k, nt, 16, nt, 4, 4)       # (j, n, m16, kq, e, g)
    return v.permute(0, 3, 1, 5, 2, 4).contiguous().reshape(-1)      # (j, kq, n, g, m16, e)


def stage_lengths(T: int, rates, kernels) -> list:
    """Frames in front of and behind every transposed convolution: [T, L_1, ..., samples]."""
    out = [int(T)]
    for k, u in zip(kernels, rates):
        out.append(convt_plan(k, u).out_len(out[-1]))
    return out


def output_length(T: int, rates=HIFIGAN_16K_64["upsample_rates"], kernels=HIFIGAN_16K_64["upsample_kernel_sizes"]) -> int:
    """Samples of T mel frames: 160 T + 32 for the shipped configuration."""
    return stage_lengths(T, rates, kernels)[-1]


class HiFiGAN:
    """`HiFiGAN(state_dict, device="cuda:0", upsample_rates=(5, 4, 2, 2, 2), resblock_dilations=((1, 3, 5),) * 3, fused=True, k_chunk=K_CHUNK)`.
    num_mels, the channel counts and every kernel size are read from the shapes; strides and dilations are not in them.  Weight-norm
    pairs are folded in float64; a `vocoder.` or `first_stage_model.vocoder.` prefix is stripped.  fused: True = `v2a_hifigan_conv` at
    the shapes of `fused_default`, False = the GEMM composition everywhere, "all" = the direct kernel at every width it takes.
    k_chunk: the K of one GEMM launch, a multiple of 16 (scripts/hifigan_probe.py measures others than K_CHUNK).
    ValueError for what the plan cannot express; weights go to the device on first use."""

    def __init__(self, state_dict, device="cuda:0", upsample_rates=(5, 4, 2, 2, 2), resblock_dilations=((1, 3, 5),) * 3, fused=True, k_chunk=K_CHUNK):
        if not isinstance(state_dict, dict):
            raise TypeError(f"HiFiGAN: a state dict, got {type(state_dict).__name__}")
        if fused not in (True, False, "all"):
            raise ValueError(f"HiFiGAN: fused={fused!r} (True, False or \"all\")")
        if int(k_chunk) < 16 or int(k_chunk) % 16:
            raise ValueError(f"HiFiGAN: k_chunk={k_chunk} must be a positive multiple of 16 (the K granularity of the exact-fp32 GEMM)")
        self.k_chunk = int(k_chunk)
        sd = dict(state_dict)
        for pre in PREFIXES:
            if any(k.startswith(pre + "conv_pre.") for k in sd):
                sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
                break
        self.rates = tuple(int(u) for u in upsample_rates)
        self.dilations = tuple(tuple(int(d) for d in ds) for ds in resblock_dilations)
        pre_w = _resolve_weight(sd, "conv_pre")
        if pre_w.ndim != 3 or pre_w.shape[2] != 7:
            raise ValueError(f"HiFiGAN: conv_pre.weight has shape {tuple(pre_w.shape)}, expected (C0, num_mels, 7)")
        self.c0, self.C = int(pre_w.shape[0]), int(pre_w.shape[1])
        n_up = len(self.rates)
        nk = len(self.dilations)
        if not 1 <= nk <= 3 or any(len(ds) < 1 for ds in self.dilations):
            raise ValueError(f"HiFiGAN: resblock_dilations={self.dilations}: one to three ResBlocks per stage (v2a_hifigan_act_pad adds up to three)")
        if f"ups.{n_up}.bias" in sd or f"resblocks.{n_up * nk}.convs1.0.bias" in sd:
            raise ValueError(f"HiFiGAN: the state dict has more stages (ups.{n_up}) or ResBlocks (resblocks.{n_up * nk}) than "
                             f"upsample_rates={self.rates} and {nk} dilation lists name")
        ups = [_resolve_weight(sd, f"ups.{i}") for i in range(n_up)]
        for i, w in enumerate(ups):
            if w.ndim != 3:
                raise ValueError(f"HiFiGAN: ups.{i}.weight has shape {tuple(w.shape)}, expected (C, C / 2, k)")
        self.up_kernels = tuple(int(w.shape[2]) for w in ups)
        rks = []
        for j in range(nk):
            w = _resolve_weight(sd, f"resblocks.{j}.convs1.0")
            if w.ndim != 3:
                raise ValueError(f"HiFiGAN: resblocks.{j}.convs1.0.weight has shape {tuple(w.shape)}, expected (C, C, k)")
            rks.append(int(w.shape[2]))
        self.res_kernels = tuple(rks)
        self.config = dict(num_mels=self.C, upsample_initial_channel=self.c0, upsample_rates=self.rates, upsample_kernel_sizes=self.up_kernels,
                           resblock_kernel_sizes=self.res_kernels, resblock_dilation_sizes=self.dilations)
        for name, c in [("conv_pre.weight: num_mels", self.C)] + [(f"ups.{i}.weight: channels", self.c0 >> (i + 1)) for i in range(n_up)]:
            if c < 16 or c % 16:
                raise ValueError(f"HiFiGAN: {name} = {c} must be a multiple of 16 (the K granularity of the exact-fp32 GEMM)")
        if self.c0 % (1 << n_up):
            raise ValueError(f"HiFiGAN: conv_pre.weight: {self.c0} channels do not halve {n_up} times")
        self.plans = []
        for i, (k, u) in enumerate(zip(self.up_kernels, self.rates)):
            try:
                self.plans.append(convt_plan(k, u))
            except ValueError as e:
                raise ValueError(f"HiFiGAN: ups.{i}.weight: {e}") from None
        for j, rk in enumerate(self.res_kernels):
            if rk % 2 == 0:
                raise ValueError(f"HiFiGAN: resblocks.{j}.convs1.0.weight: kernel size {rk} must be odd (\"same\" padding)")
        w64 = {}
        for key, shape in expected_state_dict_shapes(self.config).items():
            p, kind = key.rsplit(".", 1)
            if kind == "weight":
                t = _resolve_weight(sd, p)
            else:
                if key not in sd:
                    raise ValueError(f"HiFiGAN: missing key {key}")
                t = sd[key].double()
            if tuple(t.shape) != shape:
                raise ValueError(f"HiFiGAN: {key} has shape {tuple(t.shape)}, expected {shape}")
            w64[key] = t.detach().cpu()
        self.n_up, self.nk = n_up, nk
        self.hop = math.prod(self.rates)
        self.c_last = self.c0 >> n_up
        if self.c_last > 512:
            raise ValueError(f"HiFiGAN: conv_post.weight: {self.c_last} channels are more than the 512 v2a_hifigan_post takes")
        pads = [(rk - 1) * d // 2 for rk, ds in zip(self.res_kernels, self.dilations) for d in ds] + [(rk - 1) // 2 for rk in self.res_kernels]
        self.halo = max([3] + pads + [pl.reach for pl in self.plans]) + 1
        self.fused = fused
        self.dev = torch.device(device)
        self._w64 = w64
        self._w = None
        self._cache = None

    # ---- geometry ----------------------------------------------------------------------------------------------------------
    def output_length(self, T: int) -> int:
        return stage_lengths(T, self.rates, self.up_kernels)[-1]

    def _fused_at(self, C: int, k: int, d: int) -> bool:
        if self.fused is False or C not in FUSED_CHANNELS:
            return False
        return True if self.fused == "all" else fused_default(C, k, d)

    def _geometry(self, b: int, T: int):
        """Per stage boundary s = 0 .. n_up: (frames of the longest clip, rows per clip, channels)."""
        lens = stage_lengths(T, self.rates, self.up_kernels)
        pitch, chans = [T + 2 * self.halo], [self.c0]
        for i, u in enumerate(self.rates):
            pitch.append(pitch[-1] * u)
            chans.append(self.c0 >> (i + 1))
        for n, p in zip(lens, pitch):
            assert p >= n + 2 * self.halo, (n, p, self.halo)             # room for the zero halo of an operand buffer at every stage
        return lens, pitch, chans

    def _weights(self):
        if self._w is None:
            L.lib()                                                      # fail loudly without the HIP library, before the copies
            w64, dev = self._w64, self.dev
            put = lambda t: t.to(torch.float32).contiguous().to(dev)

            def conv(p, d=1):
                w = w64[p + ".weight"]                                   # (co, ci, k)
                co, ci, k = w.shape
                c = dict(w=put(w.permute(0, 2, 1).reshape(co, k * ci)), b=put(w64[p + ".bias"]), k=k, C=ci)
                if co == ci and self._fused_at(ci, k, d):
                    c["wp"] = put(pack_conv_fragments(w.to(torch.float32)))
                return c

            stages = []
            for i, u in enumerate(self.rates):
                up = dict(w=put(polyphase_weight(w64[f"ups.{i}.weight"], u)), b=put(w64[f"ups.{i}.bias"].repeat(u)))
                blocks = [dict(c1=[conv(f"resblocks.{i * self.nk + j}.convs1.{m}", d) for m, d in enumerate(ds)],
                               c2=[conv(f"resblocks.{i * self.nk + j}.convs2.{m}") for m in range(len(ds))]) for j, ds in enumerate(self.dilations)]
                stages.append(dict(up=up, blocks=blocks))
            pw = w64["conv_pre.weight"]
            self._w = dict(pre=dict(w=put(pw.permute(0, 2, 1).reshape(self.c0, 7 * self.C)), b=put(w64["conv_pre.bias"]), k=7, C=self.C), stages=stages,
                           post_w=put(w64["conv_post.weight"][0].t()), post_b=put(w64["conv_post.bias"]))          # taps (7, C)
        return self._w

    def _buffers(self, b: int, T: int):
        if self._cache is None or self._cache[0] != (b, T):
            self._cache = None                                           # the old set goes before the new one comes
            lens, pitch, chans = self._geometry(b, T)
            size = max([b * pitch[0] * self.C] + [b * p * c for p, c in zip(pitch, chans)])
            if b > 65535 or b * pitch[-1] >= 1 << 31 or pitch[-1] > 1 << 28:
                raise ValueError(f"{b} clips of {T} frames are more than one launch takes")
            names = ["u", "t", "op"] + [f"r{j}" for j in range(self.nk)]
            self._cache = ((b, T), {n: torch.zeros(size, dtype=torch.float32, device=self.dev) for n in names})
        return self._cache[1]

    # ---- launches ----------------------------------------------------------------------------------------------------------
    def _act_pad(self, srcs, src_pitch, b, T, C, lens_dev, div, slope, out, out_pitch, halo):
        s = [t.data_ptr() for t in srcs] + [0] * (3 - len(srcs))
        L._launch("hifigan_act_pad", 0.0, 4.0 * b * C * (len(srcs) * T + out_pitch),
                  lambda: L.lib().v2a_hifigan_act_pad(s[0], s[1], s[2], src_pitch, C, b, T, C, L._p(lens_dev), float(div), float(slope), out.data_ptr(),
                                                      out_pitch, halo, L.stream_ptr()))

    @staticmethod
    def _gemm_chain(op, base, lda, launches, w, bias, out, M, N, resid=None):
        """The launches of `conv_launches` (or the chunks of a plain K range) of one GEMM: A rows at op + base + offset, row stride lda;
        the first launch stores acc + bias (+ resid), launch c adds to `out` in place through the RESID epilogue, in launch order."""
        k0 = 0
        for c, segs in enumerate(launches):
            a = [(op[base + off:], lda, ka) for off, ka in segs]
            first = c == 0
            r = resid if first else out
            L.gemm(a, w[:, k0:], out, M=M, N=N, compute=L.F32, bias=bias if first else None, ldo=N,
                   epilogue=L.EPI_RESID if r is not None else L.EPI_STORE, resid=r, ldr=N)
            k0 += sum(ka for _, ka in segs)

    def _conv_gemm(self, cv, op, d, out, pitch, b, n, resid=None):
        """Conv1d(k, dilation d, "same" zero padding) over the operand buffer `op` (rows per clip `pitch`, halo self.halo) -> out rows
        b * pitch + t."""
        C, k = cv["C"], cv["k"]
        pad = (k - 1) * d // 2
        self._gemm_chain(op, (self.halo - pad) * C, C, conv_launches(k, d, C, self.k_chunk), cv["w"], cv["b"], out, (b - 1) * pitch + n, cv["w"].shape[0], resid)

    def _conv_fused(self, cv, x, d, out, pitch, b, n, lens_dev, resid=None):
        C, k = cv["C"], cv["k"]
        L._launch(f"hifigan_conv<{C}>", 2.0 * b * n * C * C * k, 4.0 * (b * n * C * (3 if resid is not None else 2) + k * C * C),
                  lambda: L.lib().v2a_hifigan_conv(x.data_ptr(), C, pitch, b, n, C, L._p(lens_dev), cv["wp"].data_ptr(), cv["b"].data_ptr(), k, d,
                                                   LRELU_SLOPE, L._p(resid), C, out.data_ptr(), C, L.stream_ptr()))

    def _resblock(self, blk, ds, u, r, buf, pitch, b, n, C, lens_dev):
        """Three rounds of x = c2(lrelu(c1(lrelu(x)))) + x from x = u into r (u is left as it is)."""
        x = u
        for c1, c2, d in zip(blk["c1"], blk["c2"], ds):
            if "wp" in c1:
                self._conv_fused(c1, x, d, buf["t"], pitch, b, n, lens_dev)
            else:
                self._act_pad([x], pitch, b, n, C, lens_dev, 1.0, LRELU_SLOPE, buf["op"], pitch, self.halo)
                self._conv_gemm(c1, buf["op"], d, buf["t"], pitch, b, n)
            if "wp" in c2:
                self._conv_fused(c2, buf["t"], 1, r, pitch, b, n, lens_dev, resid=x)
            else:
                self._act_pad([buf["t"]], pitch, b, n, C, lens_dev, 1.0, LRELU_SLOPE, buf["op"], pitch, self.halo)
                self._conv_gemm(c2, buf["op"], 1, r, pitch, b, n, resid=x)
            x = r

    def _upsample(self, i, srcs, div, buf, geo, b, lens_dev):
        """leaky ReLU of the mean of `srcs` (stage boundary i) -> the transposed convolution -> buf["u"] at stage boundary i + 1."""
        lens, pitch, chans = geo
        pl, up, C = self.plans[i], self._weights()["stages"][i]["up"], chans[i]
        self._act_pad(srcs, pitch[i], b, lens[i], C, lens_dev, div, LRELU_SLOPE, buf["op"], pitch[i], self.halo)
        K = pl.taps * C
        launches = [[(k0, min(self.k_chunk, K - k0))] for k0 in range(0, K, self.k_chunk)]
        self._gemm_chain(buf["op"], (self.halo - pl.s_max) * C, C, launches, up["w"], up["b"], buf["u"], (b - 1) * pitch[i] + lens[i] + pl.extra,
                         pl.u * chans[i + 1])

    # ---- the call ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, mel, lens=None, out=None, taps=None, pcm=False):
        """mel (b, C, T) or (C, T) fp32 on the host or the device -> (b, samples) fp32 on the device, samples = `output_length(T)`.
        lens: b integers, 1 <= lens[i] <= T: clip i is decoded as if it were alone with lens[i] frames (zero padding at its own ends);
        the result is then a list of `output_length(lens[i])` waves, views of one buffer, from one pass.
        out: a (b, samples) destination on the device with unit stride along time and any row stride.
        pcm: int16 `trunc(wave * 32768)` saturated to -32768 .. 32767 instead of the fp32 wave (`vocoder_infer`).
        taps: a dict that receives copies of intermediate activations in the module's layout (b, C, frames) (tests): "conv_pre", per
        stage "up{i}" and "mrf{i}", "pre" (b, samples) in front of tanh, and "wave"; frames at or behind a clip's length hold zeros."""
        x = torch.as_tensor(mel)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1] != self.C or x.shape[0] < 1:
            raise ValueError(f"mel frames are (b, {self.C}, T) or ({self.C}, T), got {tuple(torch.as_tensor(mel).shape)}")
        if not x.is_floating_point():
            raise ValueError(f"mel frames are floating point, got {x.dtype}")
        b, T = int(x.shape[0]), int(x.shape[2])
        if T < 1:
            raise ValueError("a wave needs at least one frame")
        lens_list = None
        if lens is not None:
            lens_list = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
            if len(lens_list) != b or any(not 1 <= v <= T for v in lens_list):
                raise ValueError(f"lens must be {b} integers in 1 .. T={T}, got {lens_list}")
        geo = self._geometry(b, T)
        slen, pitch, chans = geo
        n_out, dtype = slen[-1], torch.int16 if pcm else torch.float32
        w = self._weights()
        x = x.to(self.dev, torch.float32).transpose(1, 2).contiguous()                # time-major (b, T, C)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (b, n_out) or out.dtype != dtype
                                or out.device != x.device or out.stride(1) != 1 or (b > 1 and out.stride(0) < n_out)):
            raise ValueError(f"out must be a ({b}, {n_out}) {dtype} tensor on {x.device} with unit stride along time and rows that do not overlap")
        buf = self._buffers(b, T)
        if out is None:
            out = (torch.empty if lens_list is None else torch.zeros)(b, n_out, dtype=dtype, device=self.dev)
        sl = None                                                                     # per stage boundary: every clip's frames, int32 on the device
        if lens_list is not None:
            per_clip = [stage_lengths(n, self.rates, self.up_kernels) for n in lens_list]
            sl = torch.tensor([[pc[s] for pc in per_clip] for s in range(self.n_up + 1)], dtype=torch.int32, device=self.dev)
        ld = lambda s: None if sl is None else sl[s]

        def tap(name, t, s, C):
            if taps is not None:
                v = t[:b * pitch[s] * C].view(b, pitch[s], C)[:, :slen[s]].transpose(1, 2).clone()
                if sl is not None:
                    v = v * (torch.arange(slen[s], device=self.dev)[None, None, :] < sl[s][:, None, None])
                taps[name] = v

        with torch.cuda.device(self.dev):
            self._act_pad([x], T, b, T, self.C, ld(0), 1.0, 1.0, buf["op"], pitch[0], self.halo)
            self._conv_gemm(w["pre"], buf["op"], 1, buf["u"], pitch[0], b, T)
            tap("conv_pre", buf["u"], 0, self.c0)
            srcs, div = [buf["u"]], 1.0
            for i, st in enumerate(w["stages"]):
                self._upsample(i, srcs, div, buf, geo, b, ld(i))
                s, C = i + 1, chans[i + 1]
                tap(f"up{i}", buf["u"], s, C)
                srcs = [buf[f"r{j}"] for j in range(self.nk)]
                for blk, ds, r in zip(st["blocks"], self.dilations, srcs):
                    self._resblock(blk, ds, buf["u"], r, buf, pitch[s], b, slen[s], C, ld(s))
                div = float(self.nk)
                if taps is not None:
                    self._act_pad(srcs, pitch[s], b, slen[s], C, ld(s), div, 1.0, buf["t"], pitch[s], 0)
                    tap(f"mrf{i}", buf["t"], s, C)
            s, C = self.n_up, self.c_last
            self._act_pad(srcs, pitch[s], b, slen[s], C, ld(s), div, POST_SLOPE, buf["op"], pitch[s], self.halo)
            obs = out.stride(0) if b > 1 else n_out                                   # one batch stride for wave, pcm and pre
            side = lambda: torch.zeros(b, obs, dtype=torch.float32, device=self.dev)[:, :n_out]
            pre = side() if taps is not None else None
            wave = side() if taps is not None and pcm else None
            L._launch("hifigan_post", 2.0 * 7 * b * n_out * C, 4.0 * b * n_out * (C + 1),
                      lambda: L.lib().v2a_hifigan_post(buf["op"].data_ptr() + 4 * self.halo * C, pitch[s], b, n_out, C, L._p(ld(s)), w["post_w"].data_ptr(),
                                                       w["post_b"].data_ptr(), L._p(wave) if pcm else out.data_ptr(), out.data_ptr() if pcm else 0, L._p(pre),
                                                       obs, L.stream_ptr()))
        if taps is not None:
            taps["pre"] = pre
            taps["wave"] = wave if pcm else out.clone()
        if lens_list is None:
            return out
        return [out[i, :self.output_length(n)] for i, n in enumerate(lens_list)]

    __call__ = decode

    def decode_to_waveform(self, dec, lens=None):
        """`AutoencoderKL.decode_to_waveform`: dec (b, 1, T, C), the VAE decoder's mel image -> int16 (b, samples) on the device,
        `vocoder_infer`'s `(wav * 32768).astype("int16")` with a product of exactly +-32768 saturated."""
        dec = torch.as_tensor(dec)
        if dec.ndim != 4 or dec.shape[1] != 1 or dec.shape[3] != self.C:
            raise ValueError(f"dec is (b, 1, T, {self.C}), got {tuple(dec.shape)}")
        return self.decode(dec[:, 0].permute(0, 2, 1), lens=lens, pcm=True)
