"""Roll2Midi generator on the MI355X kernels: the U-Net that turns a Video2Roll key roll into the MIDI roll.

Mirrors `Generator` of src/audeo/Roll2MidiNet.py:42-87 (`r2m` below) in eval mode and the way Roll2Midi_inference.py:36-71
runs it: 100-frame windows of key probabilities (1, keys, w) -> probabilities of the same shape, thresholded at 0.5.

Design (not a translation of the reference's NCHW module tree):
  * every convolution of the net is 3x3 / stride 1 / pad 1, so all maps share one (n, keys, w) pixel grid, stored NHWC fp32;
  * each convolution is one `v2a_gemm` with the eval-mode BatchNorm (eps = 0.8: `nn.BatchNorm2d(c, 0.8)`, r2m:12,28) folded into
    weight / bias; a `ConvTranspose2d(ci, co, 3, 1, 1)` (r2m:27) is the plain convolution with w'[co][ci][ky][kx] =
    w[ci][co][2-ky][2-kx], transformed once at load time; ReLU of the up blocks in the GEMM epilogue;
  * bf16 / bf16x3: implicit GEMM over zero-bordered maps (offset tables, no patch matrix).  The skip concatenations (r2m:38) are
    never materialised: up_k writes channels [0, co) of the concatenated map and d_k was written once into channels [co, co + skip)
    of that same map, from where down_{k+1} reads it as a channel slice (the tables are plain element offsets);
  * fp32: explicit `v2a_im2col` patch matrices and the exact-fp32 GEMM; a concatenated input is two A segments of one GEMM;
  * three row kernels complete it (csrc/roll2midi.hip): `v2a_roll2midi_stem` (down1: K = 9 fills no K tile), `v2a_leaky_shadow`
    (LeakyReLU(0.2), which the GEMM epilogue lacks, + the bf16 / hi | lo copy the next GEMM reads) and `v2a_roll2midi_head`
    (conv1d 80 -> 1 + sigmoid + threshold).
`Roll2MidiEnhanceEngine` is the attention-gated generator of src/audeo/Roll2MidiNet_enhance.py (`enh`), the one the reference's trainer
and evaluator import: the same walk over wider up blocks, with a fourth row kernel, `v2a_roll2midi_gate`, behind up1..up4 (`folded_gate`).
`engine_for` picks the class from a state dict's keys.
The BatchNorm fold, the weight packing, the bordered maps with their channel slices and the offset tables are conv2d.py's, shared with
video2roll.py.  There is no CPU fallback: without libv2a_cfm.so every call raises.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import conv2d
from .conv2d import ConvMemory, gemm_weight, split_args

KEYS = 51
BN_EPS = 0.8                # nn.BatchNorm2d(out_size, 0.8): the second positional argument is eps (r2m:12,28)
LEAKY = 0.2
_DOWN = ((1, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 1024))             # down1..down6: (ci, co)   r2m:46-51
_UP = ((1024, 512), (1024 + 512, 256), (512 + 256, 128), (256 + 128, 64), (128 + 64, 16))   # up1..up5: (ci, co)       r2m:53-57
UP5_PAD = 64                # up5's 16 output channels as a GEMM of 64 (zero weight rows): the head reads the first 16
_UP_ENH = ((1024, 1024), (1024 + 1024, 512), (512 + 512, 256), (256 + 256, 128), (128 + 128, 64))      # up1..up5 of enh:74-78
_GATES = ((2048, 1024, 512), (1024, 512, 256), (512, 256, 128), (256, 128, 64))    # att1..att4: (in, g, out) channels   enh:69-72


def expected_state_dict_shapes() -> dict[str, tuple]:
    """Key layout of `Generator((1, 51, 100)).state_dict()`, the reference's `checkpoint['state_dict_G']`."""
    s: dict[str, tuple] = {}

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.{k}"] = (c,)
        s[f"{p}.num_batches_tracked"] = ()

    for i, (ci, co) in enumerate(_DOWN, 1):
        s[f"down{i}.model.0.weight"] = (co, ci, 3, 3)
        if i > 1:
            bn(f"down{i}.model.1", co)
    for i, (ci, co) in enumerate(_UP, 1):
        s[f"up{i}.model.0.weight"] = (ci, co, 3, 3)          # ConvTranspose2d: [in][out][ky][kx]
        bn(f"up{i}.model.1", co)
    s["conv1d.weight"] = (1, 80, 1, 1)
    s["conv1d.bias"] = (1,)
    return s


def expected_enhance_state_dict_shapes() -> dict[str, tuple]:
    """Key layout of `Roll2MidiNet_enhance.Generator((1, 51, 100)).state_dict()`, in the module's own order (the gates are registered
    between the down and the up blocks, enh:61-79)."""
    plain = expected_state_dict_shapes()
    s = {k: v for k, v in plain.items() if k.startswith("down")}
    for i, (c, cg, co) in enumerate(_GATES, 1):
        for name, shp in (("theta_x", (co, c, 1, 1)), ("phi_g", (co, cg, 1, 1)), ("psi", (1, co, 1, 1))):
            s[f"att{i}.{name}.weight"] = shp
            s[f"att{i}.{name}.bias"] = (shp[0],)
    for i, (ci, co) in enumerate(_UP_ENH, 1):
        s[f"up{i}.model.0.weight"] = (ci, co, 3, 3)
        for k in ("weight", "bias", "running_mean", "running_var"):
            s[f"up{i}.model.1.{k}"] = (co,)
        s[f"up{i}.model.1.num_batches_tracked"] = ()
    s["conv1d.weight"] = (1, 128, 1, 1)
    s["conv1d.bias"] = (1,)
    return s


def check_state_dict(sd: dict) -> None:
    if any(k.startswith("att") for k in sd):
        raise NotImplementedError("Roll2MidiEngine: the state dict holds attention gates (att1.* ...): that is Roll2MidiNet_enhance.py, "
                                  "which Roll2MidiEnhanceEngine runs (roll2midi.engine_for picks the class); this class is the plain "
                                  "Generator of Roll2MidiNet.py")
    conv2d.check_state_dict(sd, expected_state_dict_shapes(), "Roll2MidiEngine")


def check_enhance_state_dict(sd: dict) -> None:
    conv2d.check_state_dict(sd, expected_enhance_state_dict_shapes(), "Roll2MidiEnhanceEngine")


def folded_gate(sd: dict, k: int) -> tuple[torch.Tensor, float]:
    """Gate att{k} (`AttentionGate.forward`, enh:49-55) as one weight vector: there is no nonlinearity between theta_x + phi_g and psi,
    and the gate input g = d_(6-k) is the last Cg channels of x = u_k, so per pixel
        psi(theta_x(x) + phi_g(g)) = w . x + b,   w = psi_w theta_w + [0 ... 0 | psi_w phi_w],   b = psi_w . (theta_b + phi_b) + psi_b.
    Computed in float64 and rounded once: (w fp32 (C,), b as a Python float)."""
    g = lambda name: sd[f"att{k}.{name}"].double()
    psi = g("psi.weight").reshape(-1)                                       # (Co,)
    theta, phi = g("theta_x.weight").flatten(1), g("phi_g.weight").flatten(1)      # (Co, C), (Co, Cg)
    w = psi @ theta
    w[theta.shape[1] - phi.shape[1]:] += psi @ phi
    b = psi @ (g("theta_x.bias") + g("phi_g.bias")) + g("psi.bias").reshape(())
    return w.float().contiguous(), float(b)


def transposed_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(ci, co, 3, stride 1, pad 1) weight [ci][co][ky][kx] -> the Conv2d(ci, co, 3, 1, 1) weight of the same map."""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def folded_conv(sd: dict, name: str) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Block `name` (down1..6, up1..5) as a plain convolution: fp32 weight [co][ci][3][3] with the BatchNorm scale folded in, and the
    folded shift as bias (None for down1, which has neither BatchNorm nor bias)."""
    w = sd[f"{name}.model.0.weight"].float()
    if name.startswith("up"):
        w = transposed_conv_weight(w)
    bn = f"{name}.model.1"
    if f"{bn}.weight" not in sd:
        return w, None
    return conv2d.fold_batchnorm(w, None, *(sd[f"{bn}.{k}"].float() for k in ("weight", "bias", "running_mean", "running_var")), BN_EPS)


def window_spans(t: int, window: int) -> list[tuple[int, int]]:
    """[start, stop) of the windows `refine` cuts t frames into: whole windows, then the shorter rest."""
    return [(s, min(s + window, t)) for s in range(0, t, window)]


class Roll2MidiEngine:
    """`Generator` of Roll2MidiNet.py in eval mode on HIP kernels.

    sd: the reference's `checkpoint['state_dict_G']` (or pass prefix=).  compute: "bf16" (bf16 MFMA operands, fp32 accumulate /
    activations), "bf16x3" (split-bf16 hi | lo planes on both sides, three MFMA products per fp32 product: the parity mode at
    implicit-GEMM speed; default) or "fp32" (exact-fp32 MFMA over explicit patch matrices).
    chunk: windows per pass.  Default 8 in the bf16 / bf16x3 modes (no patch matrix; the maps of a 51x100 window take 87 MB in fp32
    plus 44 / 87 MB of shadows) and 2 in fp32 mode (the patch matrices of up2, K = 13 824, take 282 MB per window).  A window's
    output does not depend on the chunk it ran in."""

    _UPS, _PAD = _UP, UP5_PAD                # (ci, co) of up1..up5; the GEMM width a narrower up block is padded to
    _FP32_CHUNK = 2
    _check = staticmethod(check_state_dict)

    def __init__(self, sd, device="cuda:0", compute="bf16x3", prefix="", chunk=None):
        L.lib()                                                   # fail loudly without the HIP library
        if compute not in ("bf16", "bf16x3", "fp32"):
            raise ValueError(f"compute must be 'bf16', 'bf16x3' or 'fp32', got {compute!r}")
        self.dev = torch.device(device)
        self.compute = compute
        self.split = compute == "bf16x3"
        self.implicit = compute != "fp32"
        self.code = L.F32 if compute == "fp32" else L.BF16
        self.mode = L.SH_NONE if compute == "fp32" else (L.SH_SPLIT if self.split else L.SH_BF16)
        self.chunk = int(chunk) if chunk else (8 if self.implicit else self._FP32_CHUNK)
        sd = {k[len(prefix):]: v.detach().cpu() for k, v in sd.items() if k.startswith(prefix)}
        self._check(sd)
        dev = self.dev
        self.w, self.bias = {}, {}
        for name, segs, pad in self._layers():
            w, b = folded_conv(sd, name)
            wk = gemm_weight(w, None if self.implicit else segs, pad)
            if pad and b is not None:
                b = torch.cat([b, torch.zeros(pad - b.shape[0])])
            self.w[name] = (L.split_planes(wk) if self.split else wk.to(torch.bfloat16 if self.implicit else torch.float32)).to(dev).contiguous()
            self.bias[name] = None if b is None else b.to(dev).contiguous()
        self.stem_wt = folded_conv(sd, "down1")[0].reshape(64, 9).t().contiguous().to(dev)        # [tap][co]
        self.head_w = sd["conv1d.weight"].float().reshape(-1).contiguous().to(dev)
        self.head_b = float(sd["conv1d.bias"].float()[0])
        self.mem = ConvMemory(dev, self.split)              # activation maps, offset tables, patch-matrix scratch
        self._load_more(sd)

    def _load_more(self, sd):
        """What a subclass keeps of the state dict besides the convolutions."""

    @classmethod
    def _layers(cls):
        """(block, widths of the concatenated inputs, padded output width) of the convolutions that run as GEMMs."""
        out = [(f"down{i}", (ci,), 0) for i, (ci, _) in enumerate(_DOWN, 1) if i > 1]
        for i, (ci, co) in enumerate(cls._UPS, 1):
            skip = 0 if i == 1 else _DOWN[6 - i][1]                 # d5, d4, d3, d2 behind up1..up4's outputs (r2m:74-82)
            out.append((f"up{i}", (ci,) if i == 1 else (ci - skip, skip), cls._PAD if co < cls._PAD else 0))
        return out

    # ---- buffers ------------------------------------------------------------------------------------
    def _maps(self, n, H, W):
        """The slices d1..d6 (down outputs) and p1..p5 (up outputs) for n windows of H x W."""
        b = 1 if self.implicit else 0
        new = lambda name, C: self.mem.map(name, n, H, W, C, b, self.implicit)
        m = {}
        if self.implicit:
            # concatenated maps [p_k | d_(6-k)]: r2m:38 without the copy
            for k, (_, co) in enumerate(self._UPS, 1):
                cu, cd = max(co, self._PAD), _DOWN[5 - k][1]
                m[f"u{k}"] = u = new(f"u{k}", cu + cd)
                m[f"p{k}"], m[f"d{6 - k}"] = u.slice(0, cu), u.slice(cu, cd)
            m["d6"] = new("d6", 1024)
        else:
            for k, (_, co) in enumerate(_DOWN, 1):
                m[f"d{k}"] = new(f"d{k}", co)
            for k, (_, co) in enumerate(self._UPS, 1):
                m[f"p{k}"] = new(f"p{k}", max(co, self._PAD))
        return m

    # ---- one convolution ----------------------------------------------------------------------------
    def _conv(self, name, srcs, dst, n, H, W, *, relu, shadow=None):
        """srcs: the slices whose concatenation the convolution reads (implicit GEMM: ONE slice of a concatenated map).  shadow: whether
        the GEMM epilogue writes dst's shadow (default: behind a ReLU, where nothing else follows)."""
        shadow = relu if shadow is None else shadow
        w, bias, rows, N = self.w[name], self.bias[name], n * H * W, self.w[name].shape[0]
        assert N == dst.C
        if self.implicit:
            (src,) = srcs
            t = self.mem.tables(src, dst, 3, 3, 1, 1)
            shadowed = dst if shadow else None                # down blocks: v2a_leaky_shadow writes the shadow after the activation
            L.gemm([src.operand(9 * src.C)], w, dst.base(), M=rows, N=N, compute=self.code,
                   bias=bias, relu=relu, ldo=dst.pitch, out_bf16=dst.shadow() if shadow else None, ld_out_bf16=dst.pitch,
                   a_row_offset=t[0], a_ktile_offset=t[1], out_row_offset=t[2], **split_args(self.split, shadowed))
            return
        segs = []
        for i, src in enumerate(srcs):
            K = 9 * src.C
            col = self.mem.col(rows, K, i)
            L.im2col(src.f32, col, B=n, H=H, W=W, C_=src.C, kh=3, kw=3, stride=1, pad=1, Ho=H, Wo=W, ldo=K)
            segs.append((col, K, K))
        L.gemm(segs, w, dst.f32, M=rows, N=N, compute=self.code, bias=bias, relu=relu, ldo=dst.pitch)

    def _leaky(self, sl, n, H, W):
        L.leaky_shadow(sl.base(), sl.shadow(), n=n, H=H, W=W, C_=sl.C, shadow_mode=self.mode, lo_offset=sl.lo,
                       pitch=sl.pitch, border=sl.border)

    def _pass(self, x, logits, probs, midi, threshold, taps=None):
        """x (n, H, W) fp32 on the device -> the dense (n, H, W) outputs that are not None."""
        n, H, W = x.shape
        m = self._maps(n, H, W)
        d1 = m["d1"]
        L.roll2midi_stem(x, self.stem_wt, d1.base(), d1.shadow(), n=n, H=H, W=W, co=64, shadow_mode=self.mode,
                         lo_offset=d1.lo, pitch=d1.pitch, border=d1.border)
        for k in range(2, 7):                                        # r2m:64-72
            self._conv(f"down{k}", [m[f"d{k - 1}"]], m[f"d{k}"], n, H, W, relu=False)
            self._leaky(m[f"d{k}"], n, H, W)
        self._conv("up1", [m["d6"]], m["p1"], n, H, W, relu=True)    # r2m:74
        for k in range(2, 6):                                        # r2m:76-82: up_k(cat(up_(k-1), d_(7-k)))
            srcs = [m[f"u{k - 1}"]] if self.implicit else [m[f"p{k - 1}"], m[f"d{7 - k}"]]
            self._conv(f"up{k}", srcs, m[f"p{k}"], n, H, W, relu=True)
        p5 = m["p5"]
        L.roll2midi_head(p5.base(), d1.base(), self.head_w, u_pitch=p5.pitch, nu=16, d_pitch=d1.pitch, nd=64, bias=self.head_b,
                         threshold=threshold, n=n, H=H, W=W, border=d1.border, logits=logits, probs=probs, midi=midi)
        if taps is not None:
            for k in range(1, 7):
                taps.setdefault(f"d{k}", []).append(m[f"d{k}"].nchw().clone())
            for k in range(1, 6):
                up = m[f"p{k}"].nchw(_UP[k - 1][1])
                taps.setdefault(f"u{k}", []).append(torch.cat([up, m[f"d{6 - k}"].nchw()], 1))

    def _run(self, x, threshold, want_logits=False, want_midi=False, taps=None):
        """x (n, keys, w) -> (probs or logits (n, keys, w) fp32, midi (n, keys, w) uint8 or None), chunk windows per pass."""
        x = x.to(self.dev, torch.float32).contiguous()
        n = x.shape[0]
        out = torch.empty_like(x)
        midi = torch.empty(x.shape, device=self.dev, dtype=torch.uint8) if want_midi else None
        for s in range(0, n, self.chunk):
            e = min(s + self.chunk, n)
            self._pass(x[s:e], out[s:e] if want_logits else None, None if want_logits else out[s:e], None if midi is None else midi[s:e],
                       threshold, taps)
        return out, midi

    # ---- reference-shaped entry points ------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, return_logits=False, taps=None):
        """`Generator.forward` in eval mode (r2m:60-87): x (n, 1, keys, w) probabilities -> (n, 1, keys, w) probabilities, or with
        return_logits the values in front of the last sigmoid.  Any keys >= 1 and w >= 1: the net is fully convolutional.
        taps: a dict that receives d1..d6 and u1..u5 (the concatenated outputs of the up blocks), NCHW, one entry per pass."""
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError(f"Roll2MidiEngine.forward: x must be (n, 1, keys, w), got {tuple(x.shape)}")
        if x.shape[0] == 0:
            return torch.empty(x.shape, device=self.dev, dtype=torch.float32)
        return self._run(x[:, 0], 0.5, want_logits=return_logits, taps=taps)[0].unsqueeze(1)

    @torch.no_grad()
    def refine(self, roll, window=100, threshold=0.5, tail="own"):
        """roll (b, t, keys) key probabilities (`Video2RollEngine.frame_probs`) -> (probs (b, t, keys) fp32, midi (b, t, keys) uint8 =
        probs >= threshold).  t is cut into windows of `window` frames (Roll2Midi_inference.py:44-49 with 2 x 50 frames); the shorter
        last one runs at its own width (tail="own") or, as the reference does (Roll2Midi_inference.py:39-42, 58: zero LOGITS in front
        of torch.sigmoid), padded to the full width with probability 0.5 and cropped afterwards (tail="pad")."""
        if tail not in ("own", "pad"):
            raise ValueError(f"refine: tail must be 'own' or 'pad', got {tail!r}")
        if roll.dim() != 3 or int(window) < 1:
            raise ValueError(f"refine: roll must be (b, t, keys) and window >= 1, got {tuple(roll.shape)}, window {window}")
        window = int(window)
        roll = roll.to(self.dev, torch.float32)
        b, t, keys = roll.shape
        probs = torch.empty(b, t, keys, device=self.dev, dtype=torch.float32)
        midi = torch.empty(b, t, keys, device=self.dev, dtype=torch.uint8)
        full = t // window
        groups = []                                                   # (first frame, windows, frames per window, frames kept)
        if full:
            groups.append((0, full, window, window))
        if t % window:
            groups.append((full * window, 1, window if tail == "pad" else t % window, t % window))
        for first, nw, w, keep in groups:
            x = roll[:, first:first + nw * keep]
            if keep < w:
                x = torch.cat([x, torch.full((b, w - keep, keys), 0.5, device=self.dev)], 1)
            x = x.reshape(b * nw, w, keys).transpose(1, 2)            # (windows, keys, w): the reference's `data.T`
            p, mi = self._run(x, float(threshold), want_midi=True)
            probs[:, first:first + nw * keep] = p.transpose(1, 2)[:, :keep].reshape(b, nw * keep, keys)
            midi[:, first:first + nw * keep] = mi.transpose(1, 2)[:, :keep].reshape(b, nw * keep, keys)
        return probs, midi


class Roll2MidiEnhanceEngine(Roll2MidiEngine):
    """`Generator` of Roll2MidiNet_enhance.py in eval mode on HIP kernels: the checkpoint Roll2Midi_train.py writes and
    Roll2Midi_evaluate.py reads.  Constructor, `forward`, `refine`, `chunk` and the three compute modes are `Roll2MidiEngine`'s.

    The down path is the plain net's; the up blocks are wider (up1 1024 -> 1024 ... up5 256 -> 64, conv1d 128 -> 1) and an attention
    gate follows up1..up4 (enh:95-105): u_k = cat(up_k(.), d_(6-k)), u_k <- u_k * sigmoid(psi(theta_x(u_k) + phi_g(d_(6-k)))).  The
    three 1x1 convolutions fold into one weight vector (`folded_gate`), so a gate is one `v2a_roll2midi_gate` launch: a dot per pixel
    over the map the next convolution reads anyway, the scaling in place, and the shadow of the whole u_k (a gated up block asks its
    GEMM epilogue for none).  Gating d_(6-k) in place is sound: down_(7-k), its only other reader, ran before any up block.
    chunk: default 8 in the bf16 / bf16x3 modes (the maps of a 51x100 window take 108 MB in fp32 plus 54 / 108 MB of shadows) and 2 in
    fp32 mode: the two patch matrices of up2 (K = 18 432 over two segments) take 376 MB per window, 752 MB at the default."""

    _UPS = _UP_ENH
    _check = staticmethod(check_enhance_state_dict)

    def _load_more(self, sd):
        self.gate_w, self.gate_b = {}, {}
        for k in range(1, 5):
            w, b = folded_gate(sd, k)
            self.gate_w[k], self.gate_b[k] = w.to(self.dev), b

    def _gate(self, k, m, n, H, W, alpha=None):
        """u_k <- u_k * alpha in place, with its shadow: segment 0 is up_k's output, segment 1 the skip d_(6-k) behind it."""
        seg = lambda sl: (sl.base(), sl.pitch, sl.C, sl.shadow(), sl.lo)
        p = m[f"p{k}"]
        L.roll2midi_gate(seg(p), seg(m[f"d{6 - k}"]), self.gate_w[k], bias=self.gate_b[k], shadow_mode=self.mode, n=n, H=H, W=W,
                         border=p.border, alpha=alpha)

    def _pass(self, x, logits, probs, midi, threshold, taps=None):
        n, H, W = x.shape
        m = self._maps(n, H, W)
        d1 = m["d1"]
        L.roll2midi_stem(x, self.stem_wt, d1.base(), d1.shadow(), n=n, H=H, W=W, co=64, shadow_mode=self.mode,
                         lo_offset=d1.lo, pitch=d1.pitch, border=d1.border)
        for k in range(2, 7):                                        # enh:83-93
            self._conv(f"down{k}", [m[f"d{k - 1}"]], m[f"d{k}"], n, H, W, relu=False)
            self._leaky(m[f"d{k}"], n, H, W)
        if taps is not None:                                         # the skips as the down blocks left them: the gates scale them in place
            for k in range(1, 7):
                taps.setdefault(f"d{k}", []).append(m[f"d{k}"].nchw().clone())
        for k in range(1, 6):                                        # enh:95-107: up_k, then att_k over cat(up_k, d_(6-k))
            srcs = [m["d6"]] if k == 1 else ([m[f"u{k - 1}"]] if self.implicit else [m[f"p{k - 1}"], m[f"d{7 - k}"]])
            self._conv(f"up{k}", srcs, m[f"p{k}"], n, H, W, relu=True, shadow=k == 5)
            if k < 5:
                alpha = None if taps is None else torch.empty(n, H, W, device=self.dev, dtype=torch.float32)
                self._gate(k, m, n, H, W, alpha)
                if taps is not None:
                    taps.setdefault(f"a{k}", []).append(alpha.unsqueeze(1))
            if taps is not None:
                taps.setdefault(f"u{k}", []).append(torch.cat([m[f"p{k}"].nchw(), m[f"d{6 - k}"].nchw()], 1))
        p5 = m["p5"]
        L.roll2midi_head(p5.base(), d1.base(), self.head_w, u_pitch=p5.pitch, nu=64, d_pitch=d1.pitch, nd=64, bias=self.head_b,
                         threshold=threshold, n=n, H=H, W=W, border=d1.border, logits=logits, probs=probs, midi=midi)


def engine_for(sd: dict, device="cuda:0", **kw) -> Roll2MidiEngine:
    """The engine of a `state_dict_G`: `Roll2MidiEnhanceEngine` if it holds the attention gates (`att1.theta_x.weight`), else
    `Roll2MidiEngine`.  kw (compute, prefix, chunk) go to the constructor."""
    cls = Roll2MidiEnhanceEngine if kw.get("prefix", "") + "att1.theta_x.weight" in sd else Roll2MidiEngine
    return cls(sd, device, **kw)
