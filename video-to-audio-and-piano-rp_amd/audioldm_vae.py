"""The AudioLDM VAE decoder on the device: latents -> the 64-bin mel image, the `decode_first_stage` half of the reference's third
`self.vocos` (`'vae'`, x3:1404-1409; `VaeWrapper.decode`, x3:470-490), and `VaeVocoder`, which joins it to the HiFi-GAN of hifigan.py:
emb (b, 128, l) -> z (b, 8, l, 16) -> mel (b, 1, 4 l, 64) -> 640 l + 32 samples at 16 kHz, without leaving the device.  The network is
`Decoder` of src/audioldm/variational_autoencoder/modules.py under `default_audioldm_config` (src/audioldm/utils.py:159-181):

    z = post_quant_conv(z / scale_factor)                                    Conv2d(zc, zc, 1)
    h = conv_in(z)                                                           Conv2d(zc, C, 3, padding=1), C = ch * ch_mult[-1]
    h = mid.block_2(mid.attn_1(mid.block_1(h)))
    per level i = top .. 0:  num_res_blocks + 1 ResnetBlocks to ch * ch_mult[i]; for i > 0 Upsample: nearest x2, Conv2d(3)
    mel = conv_out(swish(norm_out(h)))                                       Conv2d(ch, 1, 3, padding=1)
    ResnetBlock: x' + conv2(swish(norm2(conv1(swish(norm1(x)))))), x' = nin_shortcut(x) where the widths differ, else x
    AttnBlock:   x + proj_out(softmax(q k^T C^-0.5) v) over all H W positions of norm(x), one head C wide
    norm = GroupNorm(32, eps 1e-6), swish(x) = x sigmoid(x)

Layout: channels-last fp32 maps, time on H and the frequency bins on W, with Wp = W + 2 and (H + 2) Wp rows per clip (include/v2a_cfm.h,
csrc/audioldm_vae.hip).  A 3x3 convolution is the exact-fp32 `v2a_gemm` over the *flat padded grid* of a bordered operand map: kernel
row ky is the A segment (map + ky Wp C, lda = C, ka = 3 C) -- three neighbouring pixels are 3 C contiguous floats -- and output row p is
the window whose top-left corner is padded position p, so that pixel (y, x) of a clip lands at row y Wp + x ("flat"): no patch matrix, no
offset tables, (H Wp) / (H W) - 1 = 3 - 13 % more rows than pixels.  The rows in between (x >= W) and behind a clip's own length hold
values that no kernel reads.  The last A row read is the last row of the last clip's bordered map, so the buffer needs no spare rows
beyond (H + 2) Wp per clip (`_conv` asserts it).  The launches of a call:
  * `v2a_vae_stage_in`: the reshape of `VaeWrapper.decode` and post_quant_conv (1 / scale_factor folded in float64), 8 channels padded to
    16, so that conv_in is one K = 3 x 48 GEMM.
  * per GroupNorm `v2a_vae_gn_stats` (double partial sums per tile of 512 pixels) and `v2a_vae_gn_act_pad` (normalise, swish, zero border
    and zero rows behind every clip's own length: the padding of the next convolution for a ragged batch).
  * per convolution the launches of `conv2d_launches`: K cut at k_chunk, launch c added to the sum of the launches before it through the
    RESID epilogue in place -- no fp32 chain is longer than k_chunk.  The ResnetBlock's `+ x` is the residual of conv2's first launch;
    `nin_shortcut` is a K = C chain into the destination that conv2's first launch then reads as its residual.
  * the attention, per clip, n = 16 len tokens: q over the interior of the bordered normed map (flat rows, so that proj_out's residual
    and its output are flat maps like every other), k over the dense normed rows, V^T (C, n) = W_v h^T directly from a GEMM, scores (flat
    rows, n) = q k^T, `v2a_vae_softmax` in place, P V as a plain A W^T with K = n in k_chunk launches, proj_out with v's bias folded
    into its own (b_o' = W_o b_v + b_o in float64: softmax rows sum to 1) and `+ x` as its residual.  One score buffer serves every clip.
  * `v2a_vae_upsample_pad` (nearest x2 into a bordered map) in front of an Upsample's convolution; `v2a_vae_conv_out` writes the mel rows.
One arithmetic mode, fp32 throughout.  A clip's bits depend on its own latents alone.  There is no CPU fallback."""
from __future__ import annotations

import math

import torch

from . import _lib as L

AUDIOLDM_VAE = dict(ch=128, ch_mult=(1, 2, 4), num_res_blocks=2, z_channels=8)      # default_audioldm_config, ddconfig (utils.py:159-181)
K_CHUNK = 512                # K of one GEMM launch, as in hifigan.py
GN_TILE, GROUPS, GN_EPS = 512, 32, 1e-6       # V2A_VAE_GN_TILE, V2A_VAE_GROUPS; Normalize (modules.py:38-41)
BINS = 16                    # latent frequency bins: VaeWrapper.decode's reshape(b, l, 8, 16)
PREFIX = "first_stage_model."
IGNORED = ("encoder.", "quant_conv.", "vocoder.", "loss.")


def level_widths(config: dict) -> list:
    return [int(config["ch"]) * int(m) for m in config["ch_mult"]]


def expected_state_dict_shapes(config: dict = AUDIOLDM_VAE) -> dict:
    """Key -> shape of the decoder half of the AudioLDM `AutoencoderKL`: `decoder.*` in the order of `Decoder.state_dict()`
    (attn_resolutions = [], vanilla attention in the middle), then `post_quant_conv.*`."""
    widths, nrb, zc = level_widths(config), int(config["num_res_blocks"]), int(config["z_channels"])
    s = {}

    def conv(p, co, ci, k):
        s[p + ".weight"], s[p + ".bias"] = (co, ci, k, k), (co,)

    def norm(p, c):
        s[p + ".weight"], s[p + ".bias"] = (c,), (c,)

    def block(p, ci, co):
        norm(p + ".norm1", ci)
        conv(p + ".conv1", co, ci, 3)
        norm(p + ".norm2", co)
        conv(p + ".conv2", co, co, 3)
        if ci != co:
            conv(p + ".nin_shortcut", co, ci, 1)

    c = widths[-1]
    conv("decoder.conv_in", c, zc, 3)
    block("decoder.mid.block_1", c, c)
    norm("decoder.mid.attn_1.norm", c)
    for n in ("q", "k", "v", "proj_out"):
        conv(f"decoder.mid.attn_1.{n}", c, c, 1)
    block("decoder.mid.block_2", c, c)
    cin = {}
    for i in reversed(range(len(widths))):                               # the widths follow the forward order, top level first ...
        cin[i] = c
        c = widths[i]
    for i in range(len(widths)):                                         # ... the keys the ModuleList's
        ci = cin[i]
        for j in range(nrb + 1):
            block(f"decoder.up.{i}.block.{j}", ci, widths[i])
            ci = widths[i]
        if i:
            conv(f"decoder.up.{i}.upsample.conv", widths[i], widths[i], 3)
    norm("decoder.norm_out", widths[0])
    conv("decoder.conv_out", 1, widths[0], 3)
    conv("post_quant_conv", zc, zc, 1)
    return s


def config_from_state_dict(sd: dict) -> dict:
    """ch, ch_mult, num_res_blocks and z_channels from the shapes of a prefix-stripped state dict; KeyError names a missing key."""
    def need(k):
        if k not in sd:
            raise KeyError(f"AudioLDMVaeDecoder: missing key {k}")
        return sd[k]
    zc = int(need("decoder.conv_in.weight").shape[1])
    levels = 0
    while f"decoder.up.{levels}.block.0.norm1.weight" in sd:
        levels += 1
    if levels == 0:
        raise KeyError("AudioLDMVaeDecoder: missing key decoder.up.0.block.0.norm1.weight")
    nrb = 0
    while f"decoder.up.0.block.{nrb}.norm1.weight" in sd:
        nrb += 1
    widths = [int(need(f"decoder.up.{i}.block.0.conv1.weight").shape[0]) for i in range(levels)]
    ch = widths[0]
    for i, w in enumerate(widths):
        if w % ch:
            raise ValueError(f"AudioLDMVaeDecoder: decoder.up.{i}.block.0.conv1.weight: {w} channels are no multiple of ch = {ch}")
    return dict(ch=ch, ch_mult=tuple(w // ch for w in widths), num_res_blocks=nrb - 1, z_channels=zc)


def fold_v_bias(w_o: torch.Tensor, b_o: torch.Tensor, b_v: torch.Tensor) -> torch.Tensor:
    """b_o' = W_o b_v + b_o in float64: proj_out(P (V + 1 b_v^T)) = proj_out(P V) + W_o b_v, since the rows of P sum to 1."""
    return w_o.double().flatten(1) @ b_v.double() + b_o.double()


def conv2d_launches(C: int, Wp: int, k_chunk: int = K_CHUNK) -> list:
    """The GEMM launches of a 3x3 convolution of C input channels over a bordered map of row pitch Wp: a list of launches, each a list of
    A segments (offset, ka).  `offset` counts floats from the window's top-left pixel; lda = C.  The weight matrix is (co, 9 C) with column
    (3 ky + kx) C + c = w[co][c][ky][kx], and the segments of all launches, in order, walk its columns once.  Kernel row ky is the 3 C
    contiguous floats at ky Wp C, cut at k_chunk; up to three pieces and k_chunk columns go into a launch."""
    pieces = [(ky * Wp * C + c0, min(k_chunk, 3 * C - c0)) for ky in range(3) for c0 in range(0, 3 * C, k_chunk)]
    out, cur = [], []
    for piece in pieces:
        if cur and (len(cur) == 3 or sum(n for _, n in cur) + piece[1] > k_chunk):
            out.append(cur)
            cur = []
        cur.append(piece)
    out.append(cur)
    return out


def plain_launches(K: int, k_chunk: int = K_CHUNK) -> list:
    return [[(k0, min(k_chunk, K - k0))] for k0 in range(0, K, k_chunk)]


class AudioLDMVaeDecoder:
    """`AudioLDMVaeDecoder(state_dict, device="cuda:0", scale_factor=None, k_chunk=K_CHUNK)`: the decoder half of an AudioLDM
    `AutoencoderKL` state dict (`post_quant_conv.*`, `decoder.*`; a `first_stage_model.` prefix is stripped; `encoder.*`, `quant_conv.*`,
    `vocoder.*` and `loss.*` are ignored).  scale_factor: the argument, else a `scale_factor` entry of the dict, else 1.  ch, ch_mult,
    num_res_blocks and z_channels are read from the shapes.  KeyError / ValueError name a missing or mis-shaped key; ValueError for what
    the plan cannot express: attention outside the middle (`up.*.attn.*`), a 5x5 `upsample.conv` (`UpsampleTimeStride4`), `conv_shortcut`,
    channel counts that are no multiples of 32.  Weights go to the device on first use."""

    def __init__(self, state_dict, device="cuda:0", scale_factor=None, k_chunk=K_CHUNK):
        if not isinstance(state_dict, dict):
            raise TypeError(f"AudioLDMVaeDecoder: a state dict, got {type(state_dict).__name__}")
        if int(k_chunk) < 16 or int(k_chunk) % 16:
            raise ValueError(f"AudioLDMVaeDecoder: k_chunk={k_chunk} must be a positive multiple of 16 (the K granularity of the exact-fp32 GEMM)")
        self.k_chunk = int(k_chunk)
        sd = dict(state_dict)
        if any(k.startswith(PREFIX + "decoder.") for k in sd):
            sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()}
        if scale_factor is None:
            scale_factor = float(sd["scale_factor"]) if "scale_factor" in sd else 1.0
        self.scale_factor = float(scale_factor)
        if not math.isfinite(self.scale_factor) or self.scale_factor == 0.0:
            raise ValueError(f"AudioLDMVaeDecoder: scale_factor={scale_factor}")
        sd = {k: v for k, v in sd.items() if k != "scale_factor" and not k.startswith(IGNORED)}
        for k in sd:
            if k.startswith("decoder.up.") and ".attn." in k:
                raise ValueError(f"AudioLDMVaeDecoder: {k}: attention outside the middle (attn_resolutions) is not built")
            if ".conv_shortcut." in k:
                raise ValueError(f"AudioLDMVaeDecoder: {k}: a 3x3 conv_shortcut is not built (nin_shortcut is)")
            if k.endswith(".upsample.conv.weight") and tuple(sd[k].shape[2:]) != (3, 3):
                raise ValueError(f"AudioLDMVaeDecoder: {k} has shape {tuple(sd[k].shape)}: UpsampleTimeStride4 (a 5x5 convolution) is not built")
        self.config = config_from_state_dict(sd)
        self.widths, self.nrb, self.zc = level_widths(self.config), self.config["num_res_blocks"], self.config["z_channels"]
        w64 = {}
        for key, shape in expected_state_dict_shapes(self.config).items():
            if key not in sd:
                raise KeyError(f"AudioLDMVaeDecoder: missing key {key}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"AudioLDMVaeDecoder: {key} has shape {tuple(sd[key].shape)}, expected {shape}")
            w64[key] = sd[key].detach().double().cpu()
        for i, c in enumerate(self.widths):
            if c % GROUPS:
                raise ValueError(f"AudioLDMVaeDecoder: decoder.up.{i}.block.0.conv1.weight: {c} channels are no multiple of {GROUPS} (the groups of GroupNorm)")
        if not 1 <= self.zc <= 64:
            raise ValueError(f"AudioLDMVaeDecoder: decoder.conv_in.weight: z_channels = {self.zc} (1 .. 64)")
        self.levels = len(self.widths)
        self.up = 1 << (self.levels - 1)                                 # mel rows per latent frame: 4
        self.bins = BINS * self.up                                       # mel bins: 64
        self.C = self.zc * BINS                                          # channels of `emb`: 128
        self.c_pad = (self.zc + 15) // 16 * 16
        self.dev = torch.device(device)
        self._w64, self._w, self._cache = w64, None, None

    # ---- weights -----------------------------------------------------------------------------------------------------------
    def _weights(self):
        if self._w is None:
            L.lib()                                                      # fail loudly without the HIP library, before the copies
            w64, dev = self._w64, self.dev
            put = lambda t: t.to(torch.float32).contiguous().to(dev)

            def conv3(p, pad_to=None):
                w = w64[p + ".weight"]                                   # (co, ci, 3, 3) -> (co, (ky, kx, ci))
                co, ci = w.shape[:2]
                w = w.permute(0, 2, 3, 1)
                if pad_to is not None and pad_to > ci:
                    w = torch.cat([w, w.new_zeros(co, 3, 3, pad_to - ci)], 3)
                    ci = pad_to
                return dict(w=put(w.reshape(co, 9 * ci)), b=put(w64[p + ".bias"]), C=ci, N=co)

            def conv1(p, bias=None):
                w = w64[p + ".weight"]
                return dict(w=put(w.flatten(1)), b=put(w64[p + ".bias"] if bias is None else bias), C=int(w.shape[1]), N=int(w.shape[0]))

            norm = lambda p: dict(g=put(w64[p + ".weight"]), b=put(w64[p + ".bias"]))

            def block(p):
                d = dict(n1=norm(p + ".norm1"), c1=conv3(p + ".conv1"), n2=norm(p + ".norm2"), c2=conv3(p + ".conv2"))
                if p + ".nin_shortcut.weight" in w64:
                    d["nin"] = conv1(p + ".nin_shortcut")
                return d

            a = "decoder.mid.attn_1."
            attn = dict(norm=norm(a + "norm"), q=conv1(a + "q"), k=conv1(a + "k"), wv=put(w64[a + "v.weight"].flatten()),
                        o=conv1(a + "proj_out", fold_v_bias(w64[a + "proj_out.weight"], w64[a + "proj_out.bias"], w64[a + "v.bias"])))
            ups = {}
            for i in range(self.levels):
                ups[i] = dict(blocks=[block(f"decoder.up.{i}.block.{j}") for j in range(self.nrb + 1)])
                if i:
                    ups[i]["us"] = conv3(f"decoder.up.{i}.upsample.conv")
            co = w64["decoder.conv_out.weight"]                          # (1, C, 3, 3) -> taps (ky, kx, c)
            self._w = dict(pq_w=put(w64["post_quant_conv.weight"].flatten(1) / self.scale_factor), pq_b=put(w64["post_quant_conv.bias"]),
                           conv_in=conv3("decoder.conv_in", self.c_pad), mid1=block("decoder.mid.block_1"), attn=attn,
                           mid2=block("decoder.mid.block_2"), ups=ups, norm_out=norm("decoder.norm_out"),
                           out_w=put(co[0].permute(1, 2, 0).reshape(-1)), out_b=put(w64["decoder.conv_out.bias"]))
        return self._w

    # ---- geometry and buffers ----------------------------------------------------------------------------------------------
    def _stages(self, l: int) -> list:
        """Per resolution s = 0 .. levels - 1 (coarse to fine): (H, W, rows per clip)."""
        return [((l << s), (BINS << s), ((l << s) + 2) * ((BINS << s) + 2)) for s in range(self.levels)]

    def _buffers(self, b: int, l: int):
        if self._cache is None or self._cache[0] != (b, l):
            self._cache = None                                           # the old set goes before the new one comes
            st = self._stages(l)
            cmax = [max(self.widths[-1], self.c_pad)] + [max(self.widths[self.levels - 1 - s], self.widths[min(self.levels - s, self.levels - 1)]) for s in range(1, self.levels)]
            size = max(b * pitch * c for (_, _, pitch), c in zip(st, cmax))
            if b > 65535 or b * st[-1][2] >= 1 << 28 or size >= 1 << 40:
                raise ValueError(f"{b} clips of {l} latent frames are more than one launch takes")
            buf = {n: torch.zeros(size, dtype=torch.float32, device=self.dev) for n in ("x", "y", "t", "op")}
            tiles = (st[-1][0] * st[-1][1] + GN_TILE - 1) // GN_TILE
            buf["part"] = torch.zeros(b * tiles * GROUPS * 2, dtype=torch.float64, device=self.dev)
            C, n = self.widths[-1], BINS * l
            mflat = (l - 1) * (BINS + 2) + BINS
            buf["dense"] = torch.zeros(b * n * C, dtype=torch.float32, device=self.dev)
            for name, rows in (("q", mflat), ("k", n), ("o", mflat)):
                buf[name] = torch.zeros(rows * C, dtype=torch.float32, device=self.dev)
            buf["vt"] = torch.zeros(C * n, dtype=torch.float32, device=self.dev)
            buf["s"] = torch.zeros(mflat * n, dtype=torch.float32, device=self.dev)
            self._cache = ((b, l), buf)
        return self._cache[1]

    # ---- launches ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _chain(a, base, lda, launches, w, bias, out, M, N, ldo=None, resid=None):
        """One GEMM in the launches of `conv2d_launches` / `plain_launches`: A rows at a + base + offset with row stride lda; the first
        launch stores acc + bias (+ resid), launch c adds to `out` in place through the RESID epilogue, in launch order."""
        ldo = N if ldo is None else ldo
        k0 = 0
        for c, segs in enumerate(launches):
            first = c == 0
            r = resid if first else out
            L.gemm([(a[base + off:], lda, ka) for off, ka in segs], w[:, k0:], out, M=M, N=N, compute=L.F32, bias=bias if first else None, ldo=ldo,
                   epilogue=L.EPI_RESID if r is not None else L.EPI_STORE, resid=r, ldr=ldo)
            k0 += sum(ka for _, ka in segs)

    def _conv(self, cv, op, out, geo, b, resid=None):
        """Conv2d(3, padding=1) over the bordered operand map `op` -> the flat map `out` (+ the flat map `resid`, which may be `out`)."""
        H, W, pitch = geo
        Wp, C = W + 2, cv["C"]
        M = (b - 1) * pitch + (H - 1) * Wp + W                            # the last clip's last pixel is the last output row
        assert M - 1 + 2 * Wp + 2 < b * pitch and op.numel() >= b * pitch * C and out.numel() >= M * cv["N"]      # the last window ends inside the map
        self._chain(op, 0, C, conv2d_launches(C, Wp, self.k_chunk), cv["w"], cv["b"], out, M, cv["N"], resid=resid)

    def _norm(self, nm, x, src_pitch, src_wp, geo, b, C, lens_dev, swish, out, out_pitch, border, buf):
        H, W, _ = geo
        tiles = (H * W + GN_TILE - 1) // GN_TILE
        lp = L._p(lens_dev)
        L._launch("vae_gn_stats", 3.0 * b * H * W * C, 4.0 * b * H * W * C,
                  lambda: L.lib().v2a_vae_gn_stats(x.data_ptr(), src_pitch, src_wp, b, H, W, C, lp, buf["part"].data_ptr(), tiles, L.stream_ptr()))
        L._launch("vae_gn_act_pad", 8.0 * b * H * W * C, 4.0 * b * C * (H * W + out_pitch),
                  lambda: L.lib().v2a_vae_gn_act_pad(x.data_ptr(), src_pitch, src_wp, b, H, W, C, lp, buf["part"].data_ptr(), tiles, nm["g"].data_ptr(),
                                                     nm["b"].data_ptr(), GN_EPS, 1 if swish else 0, out.data_ptr(), out_pitch, border, L.stream_ptr()))

    def _resblock(self, blk, x, y, buf, geo, b, lens_dev):
        """ResnetBlock.forward from the flat map x into the flat map y (x is left as it is)."""
        H, W, pitch = geo
        ci, co = blk["c1"]["C"], blk["c1"]["N"]
        self._norm(blk["n1"], x, pitch, W + 2, geo, b, ci, lens_dev, True, buf["op"], pitch, 1, buf)
        self._conv(blk["c1"], buf["op"], buf["t"], geo, b)
        self._norm(blk["n2"], buf["t"], pitch, W + 2, geo, b, co, lens_dev, True, buf["op"], pitch, 1, buf)
        resid = x
        if "nin" in blk:
            M = (b - 1) * pitch + (H - 1) * (W + 2) + W
            self._chain(x, 0, ci, plain_launches(ci, self.k_chunk), blk["nin"]["w"], blk["nin"]["b"], y, M, co)
            resid = y
        self._conv(blk["c2"], buf["op"], y, geo, b, resid=resid)

    def _attention(self, at, x, y, buf, geo, b, lens_list, lens_dev):
        """AttnBlock.forward from the flat map x into the flat map y, clip by clip."""
        H, W, pitch = geo
        C, Wp, kc = self.widths[-1], W + 2, self.k_chunk
        self._norm(at["norm"], x, pitch, Wp, geo, b, C, lens_dev, False, buf["op"], pitch, 1, buf)
        self._norm(at["norm"], x, pitch, Wp, geo, b, C, lens_dev, False, buf["dense"], H * W, 0, buf)
        kk = plain_launches(C, kc)
        for i in range(b):
            ln = H if lens_list is None else lens_list[i]
            n, m = ln * W, (ln - 1) * Wp + W                              # tokens; flat rows from the clip's first pixel to its last
            row0 = i * pitch * C
            hd = buf["dense"][i * H * W * C:]
            self._chain(buf["op"], row0 + (Wp + 1) * C, C, kk, at["q"]["w"], at["q"]["b"], buf["q"], m, C)
            self._chain(hd, 0, C, kk, at["k"]["w"], at["k"]["b"], buf["k"], n, C)
            self._chain(at["wv"], 0, C, kk, hd.view(-1)[:n * C].view(n, C), None, buf["vt"], C, n, ldo=n)
            self._chain(buf["q"], 0, C, kk, buf["k"][:n * C].view(n, C), None, buf["s"], m, n, ldo=n)
            L._launch("vae_softmax", 4.0 * m * n, 8.0 * m * n,
                      lambda: L.lib().v2a_vae_softmax(buf["s"].data_ptr(), n, m, n, float(C) ** -0.5, L.stream_ptr()))
            self._chain(buf["s"], 0, n, plain_launches(n, kc), buf["vt"][:C * n].view(C, n), None, buf["o"], m, C)
            self._chain(buf["o"], 0, C, kk, at["o"]["w"], at["o"]["b"], y[row0:], m, C, resid=x[row0:])

    # ---- the call ----------------------------------------------------------------------------------------------------------
    def _check_lens(self, lens, b, l):
        if lens is None:
            return None
        lens_list = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        if len(lens_list) != b or any(not 1 <= v <= l for v in lens_list):
            raise ValueError(f"lens must be {b} integers in 1 .. l={l}, got {lens_list}")
        return lens_list

    @torch.no_grad()
    def _decode(self, src, strides, b, l, lens, taps):
        lens_list = self._check_lens(lens, b, l)
        w, buf, st = self._weights(), self._buffers(b, l), self._stages(l)
        sl = None
        if lens_list is not None:
            sl = torch.tensor([[n << s for n in lens_list] for s in range(self.levels)], dtype=torch.int32, device=self.dev)
        ld = lambda s: None if sl is None else sl[s]
        mel = (torch.empty if lens_list is None else torch.zeros)(b, l * self.up, self.bins, dtype=torch.float32, device=self.dev)

        def tap(name, t, s, C):
            if taps is not None:
                H, W, pitch = st[s]
                v = t[:b * pitch * C].view(b, H + 2, W + 2, C)[:, :H, :W].permute(0, 3, 1, 2).clone()
                if sl is not None:
                    v = torch.where(torch.arange(H, device=self.dev)[None, None, :, None] < sl[s][:, None, None, None], v, torch.zeros_like(v))
                taps[name] = v

        with torch.cuda.device(self.dev):
            H, W, pitch = st[0]
            L._launch("vae_stage_in", 2.0 * b * H * W * self.zc * self.zc, 4.0 * b * (H * W * self.zc + pitch * self.c_pad),
                      lambda: L.lib().v2a_vae_stage_in(src.data_ptr(), *strides, b, H, W, self.zc, L._p(ld(0)), w["pq_w"].data_ptr(), w["pq_b"].data_ptr(),
                                                       buf["op"].data_ptr(), self.c_pad, pitch, L.stream_ptr()))
            x, y = buf["x"], buf["y"]
            self._conv(w["conv_in"], buf["op"], x, st[0], b)
            tap("conv_in", x, 0, self.widths[-1])
            self._resblock(w["mid1"], x, y, buf, st[0], b, ld(0))
            x, y = y, x
            tap("mid1", x, 0, self.widths[-1])
            self._attention(w["attn"], x, y, buf, st[0], b, lens_list, ld(0))
            x, y = y, x
            tap("attn", x, 0, self.widths[-1])
            self._resblock(w["mid2"], x, y, buf, st[0], b, ld(0))
            x, y = y, x
            tap("mid2", x, 0, self.widths[-1])
            for s in range(self.levels):
                i = self.levels - 1 - s
                C = self.widths[i]
                for j, blk in enumerate(w["ups"][i]["blocks"]):
                    self._resblock(blk, x, y, buf, st[s], b, ld(s))
                    x, y = y, x
                    tap(f"up{i}b{j}", x, s, C)
                if i:
                    H, W, pitch = st[s]
                    L._launch("vae_upsample_pad", 0.0, 4.0 * b * C * (H * W + st[s + 1][2]),
                              lambda: L.lib().v2a_vae_upsample_pad(x.data_ptr(), pitch, W + 2, b, H, W, C, L._p(ld(s)), buf["op"].data_ptr(), st[s + 1][2],
                                                                   L.stream_ptr()))
                    self._conv(w["ups"][i]["us"], buf["op"], y, st[s + 1], b)
                    x, y = y, x
                    tap(f"up{i}us", x, s + 1, C)
            s = self.levels - 1
            H, W, pitch = st[s]
            C = self.widths[0]
            self._norm(w["norm_out"], x, pitch, W + 2, st[s], b, C, ld(s), True, buf["op"], pitch, 1, buf)
            L._launch("vae_conv_out", 2.0 * 9 * b * H * W * C, 4.0 * b * (pitch * C + H * W),
                      lambda: L.lib().v2a_vae_conv_out(buf["op"].data_ptr(), pitch, b, H, W, C, L._p(ld(s)), w["out_w"].data_ptr(), w["out_b"].data_ptr(),
                                                       mel.data_ptr(), L.stream_ptr()))
        if taps is not None:
            taps["mel"] = mel[:, None].clone()
        return mel

    def tap_names(self) -> list:
        return tap_names(self.config)

    def decode_rows(self, emb, lens=None, taps=None):
        """emb (b, 16 zc, l) -> the mel rows (b, up l, bins) fp32 on the device, time-major: HiFiGAN's own row layout."""
        x = torch.as_tensor(emb)
        if x.ndim != 3 or x.shape[1] != self.C or x.shape[0] < 1 or x.shape[2] < 1 or not x.is_floating_point():
            raise ValueError(f"latents are floating point (b, {self.C}, l) with l >= 1, got {x.dtype} {tuple(x.shape)}")
        b, l = int(x.shape[0]), int(x.shape[2])
        x = x.to(self.dev, torch.float32).contiguous()
        return self._decode(x, (self.C * l, BINS * l, 1, l), b, l, lens, taps)

    def decode_latents(self, emb, lens=None, taps=None):
        """`VaeWrapper.decode` up to the mel image: emb (b, 128, l) -> (b, 1, 4 l, 64) fp32 on the device; the reshape
        latents[b, c, t, w] = emb[b, 16 c + w, t] happens inside `v2a_vae_stage_in`.  lens: b integers, 1 <= lens[i] <= l: clip i is
        decoded as if it were alone with lens[i] latent frames, bit for bit; rows at or behind 4 lens[i] are zero."""
        return self.decode_rows(emb, lens, taps)[:, None]

    def decode_first_stage(self, z, lens=None, taps=None):
        """`decode_first_stage`: z (b, 8, l, 16) -> the mel image (b, 1, 4 l, 64) fp32 on the device.  lens as for `decode_latents`.
        taps: a dict that receives copies of intermediate activations in the module's layout (b, C, H, W) (tests): "conv_in", "mid1",
        "attn", "mid2", per level i (the module's index, the top one first) "up{i}b{j}" and "up{i}us", and "mel"; rows at or behind a
        clip's length hold zeros."""
        x = torch.as_tensor(z)
        if x.ndim != 4 or x.shape[1] != self.zc or x.shape[3] != BINS or x.shape[0] < 1 or x.shape[2] < 1 or not x.is_floating_point():
            raise ValueError(f"z is floating point (b, {self.zc}, l, {BINS}) with l >= 1, got {x.dtype} {tuple(x.shape)}")
        b, l = int(x.shape[0]), int(x.shape[2])
        x = x.to(self.dev, torch.float32).contiguous()
        return self._decode(x, (self.zc * l * BINS, l * BINS, BINS, 1), b, l, lens, taps)[:, None]

    __call__ = decode_first_stage


def tap_names(config: dict = AUDIOLDM_VAE) -> list:
    levels, nrb = len(config["ch_mult"]), int(config["num_res_blocks"])
    out = ["conv_in", "mid1", "attn", "mid2"]
    for i in reversed(range(levels)):
        out += [f"up{i}b{j}" for j in range(nrb + 1)] + ([f"up{i}us"] if i else [])
    return out + ["mel"]


class VaeVocoder:
    """`VaeVocoder(decoder, hifigan)`: the reference's `VaeWrapper.decode` (x3:470-490) as a vocoder of `E2TTS`: latent frames
    (b, 128, l) -> `AudioLDMVaeDecoder` -> mel rows -> `HiFiGAN` -> 640 l + 32 samples at 16 kHz.  `C` and `hop` are what
    `E2TTS.load_vocoder` and the CLI read."""

    def __init__(self, decoder, hifigan):
        from .hifigan import HiFiGAN
        if not isinstance(decoder, AudioLDMVaeDecoder) or not isinstance(hifigan, HiFiGAN):
            raise TypeError(f"VaeVocoder: an AudioLDMVaeDecoder and a HiFiGAN, got {type(decoder).__name__} and {type(hifigan).__name__}")
        if decoder.bins != hifigan.C:
            raise ValueError(f"VaeVocoder: the decoder writes {decoder.bins} mel bins but the HiFiGAN reads {hifigan.C}")
        if decoder.dev != hifigan.dev:
            raise ValueError(f"VaeVocoder: the decoder is on {decoder.dev} but the HiFiGAN on {hifigan.dev}")
        self.decoder, self.hifigan = decoder, hifigan
        self.C = decoder.C
        self.hop = decoder.up * hifigan.hop
        self.dev = decoder.dev

    @classmethod
    def from_state_dict(cls, sd, device="cuda:0", scale_factor=None, **hifigan_kw):
        """Both halves from one AudioLDM checkpoint dict (`first_stage_model.decoder.*`, `first_stage_model.vocoder.*`, `scale_factor`)."""
        from .hifigan import HiFiGAN
        return cls(AudioLDMVaeDecoder(sd, device, scale_factor=scale_factor), HiFiGAN(sd, device, **hifigan_kw))

    def output_length(self, l: int) -> int:
        return self.hifigan.output_length(self.decoder.up * int(l))

    def _mel(self, features, lens):
        x = torch.as_tensor(features)
        if x.ndim == 2:
            x = x[None]
        rows = self.decoder.decode_rows(x, lens)                          # (b, T, bins)
        mel_lens = None if lens is None else [self.decoder.up * int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        return rows.transpose(1, 2), mel_lens                              # HiFiGAN transposes back: no copy

    def decode(self, features, lens=None, out=None):
        """features (b, 128, l) or (128, l) -> (b, 640 l + 32) fp32 waves on the device; with lens a list of `output_length(lens[i])` waves,
        each clip decoded as if it were alone.  out: as `HiFiGAN.decode`'s."""
        mel, mel_lens = self._mel(features, lens)
        return self.hifigan.decode(mel, lens=mel_lens, out=out)

    __call__ = decode

    def decode_to_waveform(self, features, lens=None):
        """`VaeWrapper.decode`'s int16 result (`vocoder_infer`), (b, 640 l + 32) on the device."""
        mel, mel_lens = self._mel(features, lens)
        return self.hifigan.decode(mel, lens=mel_lens, pcm=True)
