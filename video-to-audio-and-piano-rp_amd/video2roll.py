"""Video2Roll frame encoder on the MI355X kernels.

Mirrors `E2TTS.encode_frames` (src/e2_tts_pytorch/e2_tts_crossatt3.py:1525-1553) and the network it runs,
`Video2RollNet.resnet18(num_classes=51)` (src/audeo/Video2RollNet.py:127-251, `v2r` below): 5-frame windows of
100x900 grey frames -> 51 key probabilities per frame, repeated x3 in time and cropped / padded to the latent length.

Design (not a translation of the reference's NCHW module tree):
  * activations NHWC fp32; every convolution is one `v2a_gemm` -- the same MFMA GEMM the sampler uses -- with the eval-mode
    BatchNorm folded into weight / bias at load time and ReLU / residual add in the GEMM epilogue: an implicit GEMM over
    zero-bordered maps in the bf16 / bf16x3 modes, `v2a_im2col` patch matrices (the 5-frame window of the first layer gathered on
    the fly) in fp32 mode.  The fold, the weight packing, the maps and the offset tables are conv2d.py's, shared with roll2midi.py;
    the first layer's packed column patches and their tables are this engine's own;
  * FRB gates, spatial softmax, the last 1x1 conv, global pooling, fc and sigmoid are one fused kernel per window
    (`v2a_roll_head`; pooling commutes with the 1x1 conv, so only per-channel position sums are formed);
  * windows are processed in chunks so the patch matrix of the first layer (28 MB per window in bf16) stays bounded.
There is no CPU fallback: without libv2a_cfm.so every call raises.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L
from .conv2d import ConvMemory, Map, check_state_dict, fold_batchnorm, gemm_weight, split_args

NOTES = 51
BN_EPS = 1e-5
_LAYERS = (("layer1", 64, 1), ("layer2", 128, 2), ("layer3", 256, 2), ("layer4", 512, 2))


def expected_state_dict_shapes(num_classes: int = NOTES) -> dict[str, tuple]:
    """Key layout of `Video2RollNet.resnet18(num_classes=51).state_dict()` (v2r:127-168, 254-258)."""
    s: dict[str, tuple] = {}

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.{k}"] = (c,)
        s[f"{p}.num_batches_tracked"] = ()

    s["conv1.weight"] = (64, 5, 11, 11)
    bn("bn1", 64)
    inpl = 64
    for name, planes, stride in _LAYERS:
        for b in range(2):
            p = f"{name}.{b}"
            s[f"{p}.conv1.weight"] = (planes, inpl, 3, 3)
            bn(f"{p}.bn1", planes)
            s[f"{p}.conv2.weight"] = (planes, planes, 3, 3)
            bn(f"{p}.bn2", planes)
            if b == 0 and (stride != 1 or inpl != planes):
                s[f"{p}.downsample.0.weight"] = (planes, inpl, 1, 1)
                bn(f"{p}.downsample.1", planes)
            inpl = planes
    for name, cin in (("FTB2_1", 128), ("FTB2_2", 128), ("FTB3", 256), ("FTB4", 512)):
        s[f"{name}.conv0.weight"] = (128, cin, 1, 1)
        s[f"{name}.conv1.weight"] = (128, 128, 3, 3)
        bn(f"{name}.bn1", 128)
        s[f"{name}.conv2.weight"] = (128, 128, 3, 3)
    for name, c1 in (("FRB2", 128), ("FRB3", 128), ("FRB4", 64)):
        s[f"{name}.fc1.weight"] = (128, c1 + 128)
        s[f"{name}.fc1.bias"] = (128,)
        s[f"{name}.fc2.weight"] = (128, 128)
        s[f"{name}.fc2.bias"] = (128,)
    s["toplayer.weight"] = (64, 512, 1, 1)
    s["toplayer.bias"] = (64,)
    bn("toplayer_bn", 64)
    s["conv2.weight"] = (128, 128, 1, 1)
    s["conv2.bias"] = (128,)
    s["fc.weight"] = (num_classes, 128)
    s["fc.bias"] = (num_classes,)
    return s


class _Conv:
    """One convolution as a GEMM operand: weight [Cout][Kpad] in the compute dtype (BatchNorm scale folded in),
    fp32 bias (folded BatchNorm shift, plus the conv's own bias where it has one).  split (bf16x3 mode): weight rows
    [W_hi | W_lo] (ldw = 2*Kpad), split from the FOLDED fp32 weight."""

    def __init__(self, sd, wkey, bnkey, dev, cd, *, stride, pad, window=False, conv_bias=None, split=False):
        w = sd[wkey].float()
        co, ci, kh, kw = w.shape
        bias = sd[conv_bias].float() if conv_bias else None
        if bnkey is not None:
            w, bias = fold_batchnorm(w, bias, *(sd[f"{bnkey}.{k}"].float() for k in ("weight", "bias", "running_mean", "running_var")), BN_EPS)
        # K order: (c, ky, kx) for the windowed first layer (weight's own order), (ky, kx, c) for NHWC sources; K padded to the granule
        kq = 64 if cd == torch.bfloat16 else 16
        wp = F.pad(w.reshape(co, -1), (0, -(ci * kh * kw) % kq)) if window else gemm_weight(w, k_granule=kq)
        self.Kpad = wp.shape[1]
        self.w = (L.split_planes(wp) if split else wp.to(cd)).to(dev).contiguous()
        self.w_pack = None
        if window and cd == torch.bfloat16:
            # implicit first layer (v2a_frames_pack): per input channel kh rows of 16 columns, padded to whole 64-element K tiles
            g = (kh + 3) // 4
            wq = torch.zeros(co, ci, g * 4, 16)
            wq[:, :, :kh, :kw] = w
            wq = wq.reshape(co, ci * g * 64)
            self.w_pack = (L.split_planes(wq) if split else wq.to(cd)).to(dev).contiguous()
            self.g = g
        self.bias = None if bias is None else bias.to(dev).contiguous()
        self.co, self.ci, self.kh, self.kw, self.stride, self.pad, self.window = co, ci, kh, kw, stride, pad, window

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.kh) // self.stride + 1, (W + 2 * self.pad - self.kw) // self.stride + 1


class Video2RollEngine:
    """`video2roll_net` + `encode_frames` of the reference E2TTS on HIP kernels.

    sd: state dict of the reference module (`video2roll_net.` prefix already stripped, or pass prefix=).
    compute: "bf16" (bf16 MFMA operands, fp32 accumulate / activations), "bf16x3" (split-bf16 hi | lo operand planes on both
    sides, three MFMA products per fp32 product, fp32 accumulate / activations: the parity mode at implicit-GEMM speed) or
    "fp32" (exact-fp32 MFMA over explicit patch matrices).
    chunk: windows per pass.  Default 256 in the bf16 and bf16x3 modes (implicit GEMM: no patch matrix; ~22 MB of activation maps
    per window in bf16, ~29 MB in bf16x3, and one pass per clip measured fastest: 8.8 ms per 251-frame clip vs 13.3 ms at 25 in
    bf16) and 16 in fp32 mode (the explicit fp32 patch matrix of the first layer is 53 MB per window).
    expand: (rep, group) of `encode_frames`' expansion in time (`features.PianoConfig.expand`): (3, 1) repeats every row x3
    (x3:1545), (5, 2) is the 88-key configuration's x2.5 (x3_2:1546-1547).  The number of keys is the checkpoint's (`fc.weight`)."""

    def __init__(self, sd, device="cuda:0", compute="bf16", prefix="", chunk=None, expand=(3, 1)):
        L.lib()                                                   # fail loudly without the HIP library
        self.dev = torch.device(device)
        if compute not in ("bf16", "bf16x3", "fp32"):
            raise ValueError(f"compute must be 'bf16', 'bf16x3' or 'fp32', got {compute!r}")
        self.compute = compute
        self.split = compute == "bf16x3"
        self.cd = torch.float32 if compute == "fp32" else torch.bfloat16
        self.code = L.F32 if compute == "fp32" else L.BF16
        self.chunk = int(chunk) if chunk else (16 if compute == "fp32" else 256)
        self.expand = (int(expand[0]), int(expand[1]))
        if self.expand[0] < 1 or self.expand[1] not in (1, 2):
            raise ValueError(f"expand must be (rep >= 1, group 1 | 2), got {expand!r}")
        sd = {k[len(prefix):]: v.detach().cpu() for k, v in sd.items() if k.startswith(prefix)}
        check_state_dict(sd, expected_state_dict_shapes(sd["fc.weight"].shape[0] if "fc.weight" in sd else NOTES), "Video2RollEngine")
        self.notes = sd["fc.weight"].shape[0]
        dev, cd = self.dev, self.cd
        _Cv = lambda *a, **k: _Conv(*a, split=self.split, **k)
        c = {}
        c["conv1"] = _Cv(sd, "conv1.weight", "bn1", dev, cd, stride=2, pad=4, window=True)
        for name, planes, stride in _LAYERS:
            for b in range(2):
                p = f"{name}.{b}"
                st = stride if b == 0 else 1
                c[f"{p}.conv1"] = _Cv(sd, f"{p}.conv1.weight", f"{p}.bn1", dev, cd, stride=st, pad=1)
                c[f"{p}.conv2"] = _Cv(sd, f"{p}.conv2.weight", f"{p}.bn2", dev, cd, stride=1, pad=1)
                if f"{p}.downsample.0.weight" in sd:
                    c[f"{p}.down"] = _Cv(sd, f"{p}.downsample.0.weight", f"{p}.downsample.1", dev, cd, stride=st, pad=0)
        for name in ("FTB2_1", "FTB2_2", "FTB3", "FTB4"):
            c[f"{name}.conv0"] = _Cv(sd, f"{name}.conv0.weight", None, dev, cd, stride=1, pad=1)
            c[f"{name}.conv1"] = _Cv(sd, f"{name}.conv1.weight", f"{name}.bn1", dev, cd, stride=1, pad=1)
            c[f"{name}.conv2"] = _Cv(sd, f"{name}.conv2.weight", None, dev, cd, stride=1, pad=1)
        c["toplayer"] = _Cv(sd, "toplayer.weight", "toplayer_bn", dev, cd, stride=1, pad=0, conv_bias="toplayer.bias")
        self.convs = c
        t32 = lambda k: sd[k].float().t().contiguous().to(dev)    # [in][out]
        f32 = lambda k: sd[k].float().contiguous().to(dev)
        self.head_w = {}
        for i in (4, 3, 2):
            self.head_w[f"frb{i}_w1t"] = t32(f"FRB{i}.fc1.weight")
            self.head_w[f"frb{i}_b1"] = f32(f"FRB{i}.fc1.bias")
            self.head_w[f"frb{i}_w2t"] = t32(f"FRB{i}.fc2.weight")
            self.head_w[f"frb{i}_b2"] = f32(f"FRB{i}.fc2.bias")
        self.head_w["conv2_wt"] = sd["conv2.weight"].float().reshape(128, 128).t().contiguous().to(dev)
        self.head_w["conv2_b"] = f32("conv2.bias")
        self.head_w["fc_wt"] = t32("fc.weight")
        self.head_w["fc_b"] = f32("fc.bias")
        self.mem = ConvMemory(dev, self.split)              # activation maps, offset tables, patch-matrix scratch
        self._bufs: dict = {}                               # this engine's own: head buffers, packed column patches and their tables
        # bf16: implicit GEMM (the MFMA kernel gathers patch rows from zero-bordered NHWC bf16 maps through offset tables);
        # bf16x3: the same over hi | lo planes of the maps (split shadows) and of the weights, the first layer included;
        # fp32 parity mode: explicit patch matrix + the exact-fp32 GEMM, the windowed first layer through im2col.
        self.implicit = compute != "fp32"

    # ---- one convolution (+bias, +residual, +ReLU in the GEMM epilogue) ---------------------------------
    def _conv(self, name, src, dst_name, *, relu=False, resid=None, border=None, shadow=None, window=None, dst=None):
        cv = self.convs[name]
        if cv.window:
            frames, patches, T, first, n, H, W = window
        else:
            n, H, W = src.n, src.H, src.W
        Ho, Wo = cv.out_hw(H, W)
        rows = n * Ho * Wo
        if border is None:
            border = 1 if self.implicit else 0
        if shadow is None:
            shadow = self.implicit
        if dst is None:
            dst = self.mem.map(dst_name, n, Ho, Wo, cv.co, border, shadow)
        assert (dst.n, dst.H, dst.W, dst.C) == (n, Ho, Wo, cv.co)
        if resid is not None:
            assert (resid.n, resid.H, resid.W, resid.C, resid.border) == (dst.n, dst.H, dst.W, dst.C, dst.border)
        epi = L.EPI_RESID if resid is not None else L.EPI_STORE
        rs = None if resid is None else resid.f32
        sp = split_args(self.split, dst)
        if cv.window and patches is not None:
            # first layer over the packed column patches of this clip (v2a_frames_pack): windows [first, first + n) of the clip
            key = ("c1", T, first, n, H, W)
            t = self._bufs.get(key)
            if t is None:
                Hp = H + 2 * cv.pad
                dev = self.dev
                ni = torch.arange(first, first + n, device=dev, dtype=torch.int64)[:, None, None]
                yo = torch.arange(Ho, device=dev, dtype=torch.int64)[None, :, None]
                xo = torch.arange(Wo, device=dev, dtype=torch.int64)[None, None, :]
                a_row = ((ni * Wo + xo) * Hp + yo * cv.stride) * 16
                kt = torch.arange(cv.ci * cv.g, device=dev, dtype=torch.int64)
                a_k = (kt // cv.g) * (Wo * Hp * 16) + (kt % cv.g) * 64
                assert int(a_row.max()) + int(a_k.max()) + 64 <= (patches.lo or patches.t.numel()) < 2 ** 31      # within the hi plane
                t = self._bufs[key] = (a_row.reshape(-1).to(torch.int32).contiguous(), a_k.to(torch.int32).contiguous())
            L.gemm([patches], cv.w_pack, dst.f32, M=rows, N=cv.co, compute=self.code, epilogue=epi, bias=cv.bias, resid=rs,
                   relu=relu, ldo=cv.co, ldr=cv.co, a_row_offset=t[0], a_ktile_offset=t[1], **sp)
            return dst
        if self.implicit and not cv.window:
            a_row, a_k, o_row = self.mem.tables(src, dst, cv.kh, cv.kw, cv.stride, cv.pad)
            K = cv.kh * cv.kw * cv.ci
            assert K == cv.Kpad and src.C == cv.ci, "NHWC convolutions have whole 64-element K tiles (C % 64 == 0)"
            L.gemm([src.operand(K)], cv.w, dst.f32, M=rows, N=cv.co, compute=self.code, epilogue=epi, bias=cv.bias, resid=rs,
                   relu=relu, ldo=cv.co, ldr=cv.co, out_bf16=dst.sh, ld_out_bf16=cv.co,
                   a_row_offset=a_row, a_ktile_offset=a_k, out_row_offset=o_row, **sp)
            return dst
        # explicit patch matrix
        assert dst.border == 0 or cv.window is False
        col = self.mem.col(rows, cv.Kpad)
        if cv.window:
            L.im2col(frames, col, B=n, H=H, W=W, C_=5, kh=cv.kh, kw=cv.kw, stride=cv.stride, pad=cv.pad, Ho=Ho, Wo=Wo,
                     ldo=cv.Kpad, window_t=T, window_first=first)
        else:
            assert src.border == 0
            L.im2col(src.f32, col, B=n, H=H, W=W, C_=cv.ci, kh=cv.kh, kw=cv.kw, stride=cv.stride, pad=cv.pad, Ho=Ho, Wo=Wo,
                     ldo=cv.Kpad)
        L.gemm([(col, cv.Kpad, cv.Kpad)], cv.w, dst.f32, M=rows, N=cv.co, compute=self.code, epilogue=epi, bias=cv.bias, resid=rs,
               relu=relu, ldo=cv.co, ldr=cv.co)
        return dst

    def _pool(self, src, dst_name, k, stride, pad, mode, *, border=0, shadow=False, dst=None):
        Ho, Wo = (src.H + 2 * pad - k) // stride + 1, (src.W + 2 * pad - k) // stride + 1
        if dst is None:
            dst = self.mem.map(dst_name, src.n, Ho, Wo, src.C, border, shadow)
        if self.split and dst.sh is not None:
            L.pool2d_split(src.f32, dst.f32, dst.sh, lo_offset=dst.lo, B=src.n, H=src.H, W=src.W, C_=src.C, k=k,
                           stride=stride, pad=pad, mode=mode, Ho=Ho, Wo=Wo, in_border=src.border, out_border=dst.border)
            return dst
        L.pool2d(src.f32, dst.f32, B=src.n, H=src.H, W=src.W, C_=src.C, k=k, stride=stride, pad=pad, mode=mode, Ho=Ho, Wo=Wo,
                 out_bf16=dst.sh, in_border=src.border, out_border=dst.border)
        return dst

    def _block(self, p, x):
        """BasicBlock (v2r:70-88)."""
        h = self._conv(f"{p}.conv1", x, f"{p}.h", relu=True)
        res = x
        if f"{p}.down" in self.convs:
            res = self._conv(f"{p}.down", x, f"{p}.down", shadow=False)
        return self._conv(f"{p}.conv2", h, f"{p}.out", relu=True, resid=res)

    def _ftb(self, p, x, avg=True, *, to_conv=False, dst=None):
        """FTB (v2r:24-36): its 1x1 conv0 has padding=1 -- over a zero-bordered map that is a plain 1x1 conv of the border too."""
        x1 = self._conv(f"{p}.conv0", x, f"{p}.x1")
        h = self._conv(f"{p}.conv1", x1, f"{p}.h", relu=True)
        o = self._conv(f"{p}.conv2", h, f"{p}.o", resid=x1, shadow=False)
        k, st = (2, 2) if avg else (3, 1)
        b = 1 if (to_conv and self.implicit) else 0
        return self._pool(o, f"{p}.pool", k, st, 0, 1, border=b, shadow=b == 1, dst=dst)

    def _windows(self, frames, patches, T, first, n, H, W, head, row, taps=None):
        """ResNet.forward up to the pyramid maps (v2r:195-222) for windows [first, first + n) of ONE clip: frames (T, H, W) fp32
        (explicit patch matrix) or its packed column patches (implicit GEMM); the four maps the head needs land in rows
        [row, row + n) of the `head` buffers."""
        c1 = self._conv("conv1", None, "c1", relu=True, border=0, shadow=False, window=(frames, patches, T, first, n, H, W))
        b = 1 if self.implicit else 0
        h = self._pool(c1, "mp", 3, 2, 1, 0, border=b, shadow=self.implicit)
        feats = []
        for name, _, _ in _LAYERS:
            h = self._block(f"{name}.0", h)
            h = self._block(f"{name}.1", h)
            feats.append(h)
        x1, x2, x3, x4 = feats
        P = x4.H * x4.W
        view = lambda k, C: Map(head[k][row:row + n].view(n, x4.H, x4.W, C), None, x4.H, x4.W)
        x5 = self._conv("toplayer", x4, "x5", relu=True, dst=view("x5", 64))
        t = self._ftb("FTB2_1", x2, to_conv=True)
        shapes = []
        for nm, srcm, avg, key in (("FTB2_2", t, True, "x2"), ("FTB3", x3, True, "x3"), ("FTB4", x4, False, "x4")):
            k, st = (2, 2) if avg else (3, 1)
            shapes.append(((srcm.H + 2 - k) // st + 1, (srcm.W + 2 - k) // st + 1))
        if any(sh != (x4.H, x4.W) for sh in shapes):
            raise L.V2AError(f"Video2Roll: pyramid maps disagree for a {H}x{W} input: {shapes} vs {(x4.H, x4.W)}")
        x2_ = self._ftb("FTB2_2", t, dst=view("x2", 128))
        x3_ = self._ftb("FTB3", x3, dst=view("x3", 128))
        x4_ = self._ftb("FTB4", x4, avg=False, dst=view("x4", 128))
        if taps is not None:
            for k, v in dict(c1=c1, x1=x1, x2=x2, x3=x3, x4=x4, x5=x5, x2_=x2_, x3_=x3_, x4_=x4_).items():
                taps.setdefault(k, []).append(v.nchw().clone())
        return P

    def _head_buffers(self, total, H, W):
        cv = self.convs
        h1, w1 = cv["conv1"].out_hw(H, W)
        hc, wc = (h1 + 2 - 3) // 2 + 1, (w1 + 2 - 3) // 2 + 1
        for _ in range(3):                                   # layer2..4 halve the map (3x3, stride 2, pad 1)
            hc, wc = (hc + 2 - 3) // 2 + 1, (wc + 2 - 3) // 2 + 1
        P = hc * wc
        key = ("head", total, P)
        hb = self._bufs.get(key)
        if hb is None:
            e = lambda C: torch.empty(total, P, C, device=self.dev, dtype=torch.float32)
            hb = self._bufs[key] = dict(x2=e(128), x3=e(128), x4=e(128), x5=e(64))
        return hb, P

    def _pack(self, clip_frames, T, H, W):
        """bf16 column patches of one clip for the implicit first layer (v2a_frames_pack) as the operand record of that GEMM;
        bf16x3: hi | lo planes, one after the other (v2a_frames_pack_split)."""
        cv = self.convs["conv1"]
        _, Wo = cv.out_hw(H, W)
        key = ("patches", T, H, W, self.split)
        plane = (T + 4) * Wo * (H + 2 * cv.pad) * 16
        op = self._bufs.get(key)
        if op is None:
            K = cv.ci * cv.g * 64
            buf = torch.empty(plane * (2 if self.split else 1), device=self.dev, dtype=torch.bfloat16)
            op = self._bufs[key] = L.Operand(buf, K, K, plane if self.split else 0)
        if self.split:
            L.frames_pack_split(clip_frames, op.t, lo_offset=op.lo, T=T, H=H, W=W, kw=cv.kw, stride=cv.stride, pad=cv.pad, Wo=Wo)
        else:
            L.frames_pack(clip_frames, op.t, T=T, H=H, W=W, kw=cv.kw, stride=cv.stride, pad=cv.pad, Wo=Wo)
        return op

    def _run(self, frames, T, sigmoid, windows=None, taps=None):
        """frames (clips, T, H, W).  windows: explicit (clip, index) pairs (tests); default every window, clip by clip in chunks."""
        clips, _, H, W = frames.shape
        if windows is None:
            spans = [(c, f, min(self.chunk, T - f)) for c in range(clips) for f in range(0, T, self.chunk)]
        else:
            spans = [(c, w, 1) for c, w in windows]
        total = sum(n for _, _, n in spans)
        head, P = self._head_buffers(total, H, W)
        row, packed = 0, None
        for clip, first, n in spans:
            patches = None
            if self.implicit:
                if packed != clip:
                    pbuf, packed = self._pack(frames[clip], T, H, W), clip
                patches = pbuf
            self._windows(frames[clip], patches, T, first, n, H, W, head, row, taps)
            row += n
        out = torch.empty(total, self.notes, device=self.dev, dtype=torch.float32)
        a = L.RollHeadArgs()
        a.x2, a.x3, a.x4, a.x5 = head["x2"].data_ptr(), head["x3"].data_ptr(), head["x4"].data_ptr(), head["x5"].data_ptr()
        a.B, a.P = total, P
        for k, v in self.head_w.items():
            setattr(a, k, v.data_ptr())
        a.notes, a.apply_sigmoid, a.out = self.notes, 1 if sigmoid else 0, out.data_ptr()
        L.roll_head(a)
        return out

    # ---- reference-shaped entry points ----------------------------------------------------------------
    @torch.no_grad()
    def forward_windows(self, x, taps=None):
        """`ResNet.forward` on explicit windows (n, 5, H, W) -> logits (n, notes) (v2r:195-251).  Each window is loaded as
        its own 5-frame clip; the clip's centre window (index 2) is exactly that un-clamped stack (parity / test entry)."""
        n, c, H, W = x.shape
        assert c == 5
        frames = x.to(self.dev, torch.float32).contiguous()          # (n clips, T = 5 frames, H, W)
        return self._run(frames, 5, False, windows=[(i, 2) for i in range(n)], taps=taps)

    @torch.no_grad()
    def frame_probs(self, x):
        """x (b, 1, t, H, W) -> the key probabilities per video frame (b, t, notes): what `encode_frames` computes before it repeats
        every row x3 for the 75 Hz latent rate.  The Roll2Midi generator (roll2midi.py) works at the video frame rate."""
        b, c, t, H, W = x.shape
        assert c == 1
        frames = x[:, 0].to(self.dev, torch.float32).contiguous()
        return self._run(frames, t, True).view(b, t, self.notes)

    @torch.no_grad()
    def encode_frames(self, x, l: int):
        """`E2TTS.encode_frames(x, l)` (x3:1525-1553): x (b, 1, t, H, W) -> roll probabilities (b, l, notes), rows expanded in
        time by `expand`."""
        b, c, t, H, W = x.shape
        assert c == 1
        frames = x[:, 0].to(self.dev, torch.float32).contiguous()
        roll = self._run(frames, t, True)
        out = torch.empty(b, int(l), self.notes, device=self.dev, dtype=torch.float32)
        rep, group = self.expand
        if group == 1:
            L.roll_expand(roll, out, B=b, t=t, notes=self.notes, rep=rep, l=int(l))
        else:
            L.roll_expand_ratio(roll, out, B=b, t=t, notes=self.notes, rep=rep, group=group, l=int(l))      # x3_2:1546-1554
        return out
