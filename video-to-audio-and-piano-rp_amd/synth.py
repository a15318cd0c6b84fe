"""Synthetic weights and conditioning of the BASELINE shape (no checkpoints or datasets are
reachable offline: every *.pt / *.mp4 in the reference tree is a Git-LFS stub).
Used by bench.py and __graft_entry__.smoke(); distributions follow SURVEY section 8(d)."""
from __future__ import annotations

import math

import torch

from .dit import DiTConfig
from .e2tts import expected_state_dict_shapes


def random_state_dict(cfg: DiTConfig, seed: int = 0, device="cpu") -> dict[str, torch.Tensor]:
    """Random-init weights in the reference's checkpoint key layout.  Matrix weights ~ N(0, 1/fan_in)
    (activations stay O(1) through 12 layers); the parameters the reference zero-initialises
    (to_gamma, AdaLNZero, TextAudioCrossCondition) are non-zero so every kernel does real work."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for k, shp in expected_state_dict_shapes(cfg).items():
        r = lambda: torch.randn(shp, generator=g, device=device, dtype=torch.float32)
        if k.endswith(".g"):
            v = 1.0 + 0.1 * r()
        elif k.endswith("time_cond_mlp.0.weights"):
            v = r()
        elif k.endswith("registers") or k.endswith("abs_pos_emb.weight"):
            v = 0.5 * r()
        elif k.endswith("to_v_head_gate.bias"):
            v = 1.0 + r()
        elif k.endswith(".bias"):
            v = 0.1 * r()
        elif k.endswith("dw_conv1d.0.weight"):
            v = r() / math.sqrt(shp[-1])
        elif "to_gamma.weight" in k:
            v = r() * (0.5 / math.sqrt(shp[-1]))
        elif any(t in k for t in ("text_frames_to_audio", "audio_to_text", "audio_to_frames")):
            v = r() * (0.3 / math.sqrt(shp[-1]))
        else:
            v = r() / math.sqrt(shp[-1])
        sd[k] = v
    return sd


def synthetic_conditioning(cfg: DiTConfig, b: int, n: int = 750, nc: int = 16, seed: int = 0, piano: bool = False, device="cpu"):
    """(y0, clip_embed, roll, context, context_mask): CLIP features piecewise constant over ~31-frame
    runs (24 fps frames nearest-neighbour resampled to 75 Hz, x3:1803-1805), T5 context of nc tokens,
    zero piano roll for V2A (x3:2164-2165) or a ~5 % dense roll for V2P."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=device)
    y0 = r(b, n, cfg.num_channels)
    run = 31
    nseg = (n + run - 1) // run
    text = (0.5 * r(b, nseg, cfg.dim_text)).repeat_interleave(run, dim=1)[:, :n].contiguous()
    context = 0.2 * r(b, nc, cfg.ctx_dim)
    context_mask = torch.ones(b, nc, dtype=torch.bool)
    if piano:
        u = torch.rand(b, n, cfg.notes, generator=g, device=device)
        roll = torch.where(u > 0.95, u, torch.zeros((), device=device))
    else:
        roll = torch.zeros(b, n, cfg.notes, device=device)
    return y0, text, roll, context, context_mask


def random_video2roll_state_dict(seed: int = 0, num_classes: int = 51) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `Video2RollNet.resnet18(num_classes=51)`, or of the 88-key configuration's
    `num_classes=88`: `fc.*` are the last keys, so every tensor in front of them is the same for both (no piano checkpoint is reachable
    offline: `./ckpts/piano5_4_2_8000.pt`, predict.py:68).  numpy's legacy RandomState stream, so the same seed gives the
    same tensors on any machine / torch build (the golden vectors of tests/golden/video2roll_*.npz depend on that).
    Conv weights follow the reference init N(0, sqrt(2 / (k*k*out))) (Video2RollNet.py:160-163); BatchNorm scale, shift
    and running statistics are non-trivial so the folded-BatchNorm path is exercised."""
    import numpy as np

    from .video2roll import expected_state_dict_shapes

    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in expected_state_dict_shapes(num_classes).items():
        if k.endswith("num_batches_tracked"):
            v = np.array(1000, dtype=np.int64)
        elif k.endswith("running_var"):
            v = rs.uniform(0.5, 1.5, shp).astype(np.float32)
        elif k.endswith("running_mean"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".weight"):
            v = (1.0 + 0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif k.endswith(".bias"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif len(shp) == 4:
            v = (rs.standard_normal(shp) * math.sqrt(2.0 / (shp[2] * shp[3] * shp[0]))).astype(np.float32)
        else:
            v = (rs.standard_normal(shp) / math.sqrt(shp[-1])).astype(np.float32)
        sd[k] = torch.from_numpy(v) if v.ndim else torch.tensor(int(v))
    return sd


def random_roll2midi_state_dict(seed: int = 0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `Roll2MidiNet.Generator((1, 51, 100)).state_dict()`, the reference's
    `checkpoint['state_dict_G']` (no Roll2Midi checkpoint is reachable offline).  numpy's legacy RandomState stream, so the golden
    vectors of tests/golden/roll2midi.npz can be regenerated anywhere.  He-scaled convolutions (std sqrt(2 / (9 ci)); the transposed
    ones by their input channels too), BatchNorm weight in [0.8, 1.6] and running_var in [0.5, 2] -- with eps = 0.8 the folded scale
    stays near 1 -- and a conv1d weight scaled so the logits spread over several units."""
    import numpy as np

    from .roll2midi import expected_state_dict_shapes

    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in expected_state_dict_shapes().items():
        if k.endswith("num_batches_tracked"):
            v = np.array(1000, dtype=np.int64)
        elif k.endswith("running_var"):
            v = rs.uniform(0.5, 2.0, shp).astype(np.float32)
        elif k.endswith("running_mean"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif k.endswith("model.1.weight"):
            v = rs.uniform(0.8, 1.6, shp).astype(np.float32)
        elif k == "conv1d.weight":
            v = (rs.standard_normal(shp) * 2.0).astype(np.float32)
        elif k.endswith(".bias"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        else:
            ci = shp[0] if k.startswith("up") else shp[1]
            v = (rs.standard_normal(shp) * math.sqrt(2.0 / (9 * ci))).astype(np.float32)
        sd[k] = torch.from_numpy(v) if v.ndim else torch.tensor(int(v))
    return sd


def random_roll2midi_enhance_state_dict(seed: int = 0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `Roll2MidiNet_enhance.Generator((1, 51, 100)).state_dict()`, drawn in that order from numpy's
    legacy RandomState (tests/golden/roll2midi_enhance.npz).  The scaling of `random_roll2midi_state_dict`; the gates' 1x1 weights
    are N(0, (3 / sqrt(ci))^2), so the gate logits spread over about a unit and alpha is neither 0, 1 nor 0.5 everywhere, and
    conv1d.bias = -2.0, so that about half of the thresholded cells are on (four gates shrink the maps the head reads)."""
    import numpy as np

    from .roll2midi import expected_enhance_state_dict_shapes

    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in expected_enhance_state_dict_shapes().items():
        if k.endswith("num_batches_tracked"):
            v = np.array(1000, dtype=np.int64)
        elif k.endswith("running_var"):
            v = rs.uniform(0.5, 2.0, shp).astype(np.float32)
        elif k.endswith("running_mean"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif k.endswith("model.1.weight"):
            v = rs.uniform(0.8, 1.6, shp).astype(np.float32)
        elif k == "conv1d.weight":
            v = (rs.standard_normal(shp) * 2.0).astype(np.float32)
        elif k == "conv1d.bias":
            v = np.full(shp, -2.0, np.float32)
        elif k.endswith(".bias"):
            v = (0.1 * rs.standard_normal(shp)).astype(np.float32)
        elif k.startswith("att"):
            v = (rs.standard_normal(shp) * (3.0 / math.sqrt(shp[1]))).astype(np.float32)
        else:
            ci = shp[0] if k.startswith("up") else shp[1]
            v = (rs.standard_normal(shp) * math.sqrt(2.0 / (9 * ci))).astype(np.float32)
        sd[k] = torch.from_numpy(v) if v.ndim else torch.tensor(int(v))
    return sd


def synthetic_key_roll(b: int, t: int, keys: int = 51, seed: int = 0, logits: bool = False) -> torch.Tensor:
    """(b, t, keys) fp32 key probabilities as a Video2Roll encoder would give them: a few held notes (high) on a low, noisy floor.
    numpy RandomState and float64 arithmetic rounded once, reproducible across machines.  logits: the values in front of the sigmoid."""
    import numpy as np

    rs = np.random.RandomState(seed)
    logit = -3.0 + 0.8 * rs.standard_normal((b, t, keys))
    for bi in range(b):
        for _ in range(max(2, t // 6)):
            k, s, d = rs.randint(0, keys), rs.randint(0, t), rs.randint(1, 12)
            logit[bi, s:s + d, k] += 6.0
    if logits:
        return torch.from_numpy(logit.astype(np.float32))
    return torch.from_numpy((1.0 / (1.0 + np.exp(-logit))).astype(np.float32))


def synthetic_piano_frames(b: int, t: int, H: int = 100, W: int = 900, seed: int = 0) -> torch.Tensor:
    """(b, 1, t, H, W) grey frames in [0, 1] (ToTensor range, x3:1878-1890): a static keyboard-like stripe pattern plus a
    few moving bright blobs and noise.  numpy RandomState, reproducible across machines."""
    import numpy as np

    rs = np.random.RandomState(seed)
    xs = np.arange(W, dtype=np.float32)[None, :]
    ys = np.arange(H, dtype=np.float32)[:, None]
    base = 0.55 + 0.35 * np.sign(np.sin(xs * (2 * np.pi / 17.3))) * (ys > 0.35 * H)
    out = np.empty((b, 1, t, H, W), dtype=np.float32)
    for bi in range(b):
        cx = rs.uniform(0, W, 6)
        vx = rs.uniform(-6, 6, 6)
        cy = rs.uniform(0.3 * H, H, 6)
        for ti in range(t):
            f = base.copy()
            for j in range(6):
                f += 0.4 * np.exp(-(((xs - (cx[j] + vx[j] * ti) % W) / 14.0) ** 2 + ((ys - cy[j]) / 9.0) ** 2))
            f += 0.03 * rs.standard_normal((H, W)).astype(np.float32)
            out[bi, 0, ti] = np.clip(f, 0.0, 1.0)
    return torch.from_numpy(out)


def random_encodec_decoder_state_dict(seed: int = 0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `EncodecModel(EncodecConfig()).decoder.state_dict()` (weight_norm g / v pairs),
    the facebook/encodec_24khz architecture the reference loads by name (x3:421-423; unreachable offline).  numpy
    RandomState stream: same tensors on any machine.  Scales keep activations O(1) through the stack and the LSTM gates
    out of saturation."""
    import numpy as np

    from .encodec import expected_state_dict_shapes

    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in expected_state_dict_shapes().items():
        if k.endswith("original0"):
            v = rs.uniform(0.8, 1.6, shp)
        elif k.endswith("original1"):
            v = rs.standard_normal(shp) / math.sqrt(shp[1] * shp[2])
        elif "lstm.weight" in k:
            v = rs.uniform(-1.0, 1.0, shp) / math.sqrt(shp[1])
        elif "lstm.bias" in k:
            v = rs.uniform(-0.1, 0.1, shp)
        else:
            v = 0.05 * rs.standard_normal(shp)
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def random_encodec_encoder_state_dict(seed: int = 0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `EncodecModel(EncodecConfig()).encoder.state_dict()`, by the scale rules of
    `random_encodec_decoder_state_dict`: the library's latents of a peak-1 wave come out O(1)."""
    import numpy as np

    from .encodec import expected_encoder_state_dict_shapes

    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in expected_encoder_state_dict_shapes().items():
        if k.endswith("original0"):
            v = rs.uniform(0.8, 1.6, shp)
        elif k.endswith("original1"):
            v = rs.standard_normal(shp) / math.sqrt(shp[1] * shp[2])
        elif "lstm.weight" in k:
            v = rs.uniform(-1.0, 1.0, shp) / math.sqrt(shp[1])
        elif "lstm.bias" in k:
            v = rs.uniform(-0.1, 0.1, shp)
        else:
            v = 0.05 * rs.standard_normal(shp)
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def random_encodec_quantizer_state_dict(seed: int = 0, num_quantizers: int = 32, codebook_size: int = 1024, dim: int = 128,
                                        decay: float = 0.85) -> dict[str, torch.Tensor]:
    """Seeded codebooks in the key layout of `EncodecModel(EncodecConfig(target_bandwidths=[..., 24.0])).quantizer.state_dict()`:
    `layers.{s}.codebook.embed` (codebook_size, dim) standard normal scaled by decay^s -- each stage of a trained residual quantizer
    codes what the stages before it left, so its codewords are shorter -- and the training statistics `inited`, `cluster_size`,
    `embed_avg` beside it, which inference does not read.  numpy RandomState stream: same tensors on any machine."""
    import numpy as np

    rs = np.random.RandomState(seed)
    sd = {}
    for s in range(num_quantizers):
        e = torch.from_numpy((rs.standard_normal((codebook_size, dim)) * decay ** s).astype(np.float32))
        p = f"layers.{s}.codebook."
        sd[p + "inited"] = torch.ones(1)
        sd[p + "cluster_size"] = torch.zeros(codebook_size)
        sd[p + "embed"] = e
        sd[p + "embed_avg"] = e.clone()
    return sd


def synthetic_encodec_latents(codebooks: torch.Tensor, b: int, t: int, seed: int = 0, structured: bool = True) -> torch.Tensor:
    """Seeded (b, dim, t) fp32 latents for the quantizer.  structured: one random codeword per stage, summed, plus noise of 30 % of
    that sum's RMS -- what an encoder trained with the quantizer emits; otherwise standard normal scaled to the same RMS."""
    import numpy as np

    rs = np.random.RandomState(seed)
    S, Kc, D = codebooks.shape
    cb = codebooks.double().numpy()
    idx = rs.randint(0, Kc, (S, b * t))
    x = sum(cb[s][idx[s]] for s in range(S))                          # (b * t, D)
    rms = float(np.sqrt((x ** 2).mean()))
    noise = rs.standard_normal((b * t, D))
    x = x + 0.3 * rms * noise if structured else rms * noise
    return torch.from_numpy(x.reshape(b, t, D).transpose(0, 2, 1).astype(np.float32).copy())


def synthetic_wave(n: int, seed: int = 0, rate: int = 24000) -> torch.Tensor:
    """A seeded (n,) fp32 test signal: 12 sines at 60 - 6000 Hz with random amplitude and phase plus 0.05 white noise, scaled to
    peak <= 1 (numpy RandomState: the same samples on any machine)."""
    import numpy as np

    rs = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / rate
    f = np.exp(rs.uniform(math.log(60.0), math.log(6000.0), 12))
    a = rs.uniform(0.2, 1.0, 12)
    ph = rs.uniform(0.0, 2 * math.pi, 12)
    x = (a[:, None] * np.sin(2 * math.pi * f[:, None] * t[None] + ph[:, None])).sum(0) / a.sum()
    x = 0.8 * x + 0.05 * rs.standard_normal(n)
    return torch.from_numpy((x / max(1.0, np.abs(x).max())).astype(np.float32))


FLAN_T5_LARGE = dict(vocab_size=32128, d_model=1024, d_kv=64, num_heads=16, d_ff=2816, num_layers=24, relative_attention_num_buckets=32,
                     relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def random_t5_encoder_state_dict(config: dict, seed: int = 0, amplify: float = 1.0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `T5EncoderModel(T5Config(**config, feed_forward_proj="gated-gelu"))` (the flan-t5-large
    checkpoint the reference loads from ./ckpts/flan-t5-large, x3:1412-1413, is not reachable offline).  numpy RandomState stream:
    the same tensors on any machine.  q is scaled like T5's own init (no 1/sqrt(d_kv) in the attention) so the scores stay
    O(1); `amplify` multiplies the o and wo projections, which makes the residual stream grow to |h| ~ 1e2 - 1e3 by the last block
    (FLAN-T5's large residual activations) instead of staying O(1)."""
    import numpy as np

    c = dict(config)
    d, H, dkv, dff, nl, V = c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["num_layers"], c["vocab_size"]
    inner = H * dkv
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    nrm = lambda shp, s: t(rs.standard_normal(shp) * s)
    sd = {"shared.weight": nrm((V, d), 1.0)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for i in range(nl):
        P = f"encoder.block.{i}.layer."
        sd[P + "0.SelfAttention.q.weight"] = nrm((inner, d), 1.5 / math.sqrt(d * dkv))
        sd[P + "0.SelfAttention.k.weight"] = nrm((inner, d), 1.0 / math.sqrt(d))
        sd[P + "0.SelfAttention.v.weight"] = nrm((inner, d), 1.0 / math.sqrt(d))
        sd[P + "0.SelfAttention.o.weight"] = nrm((d, inner), amplify / math.sqrt(inner))
        if i == 0:
            sd[P + "0.SelfAttention.relative_attention_bias.weight"] = nrm((c["relative_attention_num_buckets"], H), 1.0)
        sd[P + "0.layer_norm.weight"] = t(1.0 + 0.1 * rs.standard_normal(d))
        sd[P + "1.DenseReluDense.wi_0.weight"] = nrm((dff, d), 1.0 / math.sqrt(d))
        sd[P + "1.DenseReluDense.wi_1.weight"] = nrm((dff, d), 1.0 / math.sqrt(d))
        sd[P + "1.DenseReluDense.wo.weight"] = nrm((d, dff), amplify / math.sqrt(dff))
        sd[P + "1.layer_norm.weight"] = t(1.0 + 0.1 * rs.standard_normal(d))
    sd["encoder.final_layer_norm.weight"] = t(1.0 + 0.1 * rs.standard_normal(d))
    return sd


# OpenCLIP ViT-bigG/14 as CLIPVisionModelWithProjection: IP-Adapter sdxl_models/image_encoder, the reference's "clip_vit" (x3:1423-1425)
VIT_BIGG_14 = dict(hidden_size=1664, intermediate_size=8192, num_hidden_layers=48, num_attention_heads=16, image_size=224, patch_size=14,
                   projection_dim=1280, layer_norm_eps=1e-5, hidden_act="gelu", num_channels=3)
# openai/clip-vit-large-patch14-336 as CLIPVisionModelWithProjection (ViT-L/14 at 336 px, 577 tokens): the reference's "clip_vit2" (x3:1426-1428)
VIT_L_14_336 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=336, patch_size=14,
                    projection_dim=768, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3)


def random_clip_vision_state_dict(config: dict, seed: int = 0, outlier: float = 0.0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `CLIPVisionModelWithProjection(CLIPVisionConfig(**config))` (the IP-Adapter image
    encoder is not reachable offline).  numpy PCG64 float32 normals: the same tensors on any machine.  Matrices ~ N(0, 1/fan_in),
    biases and LayerNorm beta ~ 0.1 N, gamma ~ 1 + 0.1 N, so every epilogue term is exercised.  `outlier > 0` scales the out_proj
    and fc2 rows (and biases) of a few residual channels by `outlier`, which drives those channels to |h| ~ 1e2 over the layers, as
    real CLIP ViTs carry them."""
    import numpy as np

    c = dict(config)
    d, dff, nl, P, S = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["patch_size"], c["image_size"]
    T = 1 + (S // P) ** 2
    rng = np.random.default_rng(seed)
    nrm = lambda shp, s: torch.from_numpy(rng.standard_normal(shp, dtype=np.float32) * np.float32(s))
    hot = torch.from_numpy(rng.choice(d, size=4, replace=False)) if outlier > 0 else None

    def boost(w, b):
        if hot is not None:
            w[hot] *= outlier
            b[hot] *= outlier
        return w, b

    E = "vision_model.embeddings."
    sd = {E + "class_embedding": nrm((d,), 0.5), E + "patch_embedding.weight": nrm((d, c.get("num_channels", 3), P, P), 1.0 / math.sqrt(3 * P * P)),
          E + "position_embedding.weight": nrm((T, d), 0.2)}
    sd["vision_model.pre_layrnorm.weight"] = 1.0 + nrm((d,), 0.1)
    sd["vision_model.pre_layrnorm.bias"] = nrm((d,), 0.1)
    for i in range(nl):
        p = f"vision_model.encoder.layers.{i}."
        for n in ("q", "k", "v"):
            sd[p + f"self_attn.{n}_proj.weight"] = nrm((d, d), 1.0 / math.sqrt(d))
            sd[p + f"self_attn.{n}_proj.bias"] = nrm((d,), 0.1)
        sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"] = boost(nrm((d, d), 1.0 / math.sqrt(d)), nrm((d,), 0.1))
        sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = 1.0 + nrm((d,), 0.1), nrm((d,), 0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = nrm((dff, d), 1.0 / math.sqrt(d)), nrm((dff,), 0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = boost(nrm((d, dff), 1.0 / math.sqrt(dff)), nrm((d,), 0.1))
        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = 1.0 + nrm((d,), 0.1), nrm((d,), 0.1)
    sd["vision_model.post_layernorm.weight"] = 1.0 + nrm((d,), 0.1)
    sd["vision_model.post_layernorm.bias"] = nrm((d,), 0.1)
    sd["visual_projection.weight"] = nrm((c["projection_dim"], d), 1.0 / math.sqrt(d))
    return sd


# facebook/dinov2-giant as Dinov2Model (ViT-g/14, stored at 518 px = 37 x 37 positions): the reference's "dinov2" (x3:1432-1433)
DINOV2_GIANT = dict(hidden_size=1536, num_hidden_layers=40, num_attention_heads=24, mlp_ratio=4, image_size=518, patch_size=14,
                    layer_norm_eps=1e-6, use_swiglu_ffn=True, num_channels=3, layerscale_value=1.0)


def dinov2_ffn_width(config: dict) -> int:
    """Hidden values of the feed-forward: Dinov2SwiGLUFFN rounds 2/3 of hidden_size * mlp_ratio up to a multiple of 8, Dinov2MLP takes all."""
    hf = int(config["hidden_size"] * config.get("mlp_ratio", 4))
    return (int(hf * 2 / 3) + 7) // 8 * 8 if config.get("use_swiglu_ffn", False) else hf


def random_dinov2_state_dict(config: dict, seed: int = 0, outlier: float = 0.0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `Dinov2Model(Dinov2Config(**config))` (dinov2-giant is not reachable offline), by the
    rules of random_clip_vision_state_dict: numpy PCG64 float32 normals, matrices ~ N(0, 1/fan_in), biases and LayerNorm beta ~ 0.1 N,
    gamma ~ 1 + 0.1 N.  LayerScale is drawn uniformly from 0.05 .. 1 (trained values, not the init value 1, so its fold is exercised).
    `outlier > 0` scales the `dense` and `weights_out` / `fc2` rows (and biases) of a few residual channels by `outlier`, which
    drives those channels to |h| ~ 1e2 over the layers."""
    import numpy as np

    c = dict(config)
    d, nl, P, S, ch = c["hidden_size"], c["num_hidden_layers"], c["patch_size"], c["image_size"], c.get("num_channels", 3)
    swiglu, hf = bool(c.get("use_swiglu_ffn", False)), dinov2_ffn_width(c)
    T = 1 + (S // P) ** 2
    rng = np.random.default_rng(seed)
    nrm = lambda shp, s: torch.from_numpy(rng.standard_normal(shp, dtype=np.float32) * np.float32(s))
    hot = torch.from_numpy(rng.choice(d, size=4, replace=False)) if outlier > 0 else None

    def boost(w, b):
        if hot is not None:
            w[hot] *= outlier
            b[hot] *= outlier
        return w, b

    E = "embeddings."
    sd = {E + "cls_token": nrm((1, 1, d), 0.5), E + "mask_token": torch.zeros(1, d), E + "position_embeddings": nrm((1, T, d), 0.2),
          E + "patch_embeddings.projection.weight": nrm((d, ch, P, P), 1.0 / math.sqrt(ch * P * P)),
          E + "patch_embeddings.projection.bias": nrm((d,), 0.1)}
    for i in range(nl):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            sd[p + f"attention.attention.{n}.weight"] = nrm((d, d), 1.0 / math.sqrt(d))
            sd[p + f"attention.attention.{n}.bias"] = nrm((d,), 0.1)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = boost(nrm((d, d), 1.0 / math.sqrt(d)), nrm((d,), 0.1))
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = 1.0 + nrm((d,), 0.1), nrm((d,), 0.1)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = 1.0 + nrm((d,), 0.1), nrm((d,), 0.1)
        sd[p + "layer_scale1.lambda1"] = torch.from_numpy(rng.uniform(0.05, 1.0, d).astype(np.float32))
        sd[p + "layer_scale2.lambda1"] = torch.from_numpy(rng.uniform(0.05, 1.0, d).astype(np.float32))
        if swiglu:
            sd[p + "mlp.weights_in.weight"], sd[p + "mlp.weights_in.bias"] = nrm((2 * hf, d), 1.0 / math.sqrt(d)), nrm((2 * hf,), 0.1)
            sd[p + "mlp.weights_out.weight"], sd[p + "mlp.weights_out.bias"] = boost(nrm((d, hf), 1.0 / math.sqrt(hf)), nrm((d,), 0.1))
        else:
            sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = nrm((hf, d), 1.0 / math.sqrt(d)), nrm((hf,), 0.1)
            sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = boost(nrm((d, hf), 1.0 / math.sqrt(hf)), nrm((d,), 0.1))
    sd["layernorm.weight"], sd["layernorm.bias"] = 1.0 + nrm((d,), 0.1), nrm((d,), 0.1)
    return sd


# open_clip CLIP-convnext_xxlarge-laion2B-s34B-b82K-augreg-soup, the vision tower: the reference's "clip_convnext" (x3:1429-1431)
CONVNEXT_XXLARGE = dict(depths=(3, 4, 30, 3), dims=(384, 768, 1536, 3072), embed_dim=1024)


def random_convnext_state_dict(config: dict, seed: int = 0, outlier: float = 0.0) -> dict[str, torch.Tensor]:
    """Seeded weights in open_clip's key layout of a TimmModel around timm's ConvNeXt (`visual.trunk.*`, `visual.head.proj.weight`;
    the real checkpoint is not reachable offline), `config` = dict(depths, dims, embed_dim), by the rules of
    random_clip_vision_state_dict: numpy PCG64 float32 normals, matrices and convolutions ~ N(0, 1/fan_in), biases and LayerNorm beta
    ~ 0.1 N, LayerNorm gamma ~ 1 + 0.1 N.  The layer scale `gamma` is drawn uniformly from 0.1 .. 1 (trained values of a size at
    which the blocks matter, not the init value 1e-6).  `outlier > 0` scales the `mlp.fc2` rows (and biases) of four channels per stage
    by `outlier`, which drives those channels of the map far above the rest."""
    import numpy as np

    depths, dims, E = tuple(config["depths"]), tuple(config["dims"]), int(config["embed_dim"])
    rng = np.random.default_rng(seed)
    nrm = lambda shp, s: torch.from_numpy(rng.standard_normal(shp, dtype=np.float32) * np.float32(s))
    T = "visual.trunk."
    sd = {T + "stem.0.weight": nrm((dims[0], 3, 4, 4), 1.0 / math.sqrt(48)), T + "stem.0.bias": nrm((dims[0],), 0.1),
          T + "stem.1.weight": 1.0 + nrm((dims[0],), 0.1), T + "stem.1.bias": nrm((dims[0],), 0.1)}
    for s, (n, C) in enumerate(zip(depths, dims)):
        p = T + f"stages.{s}."
        hot = torch.from_numpy(rng.choice(C, size=4, replace=False)) if outlier > 0 else None
        if s:
            Cp = dims[s - 1]
            sd[p + "downsample.0.weight"], sd[p + "downsample.0.bias"] = 1.0 + nrm((Cp,), 0.1), nrm((Cp,), 0.1)
            sd[p + "downsample.1.weight"], sd[p + "downsample.1.bias"] = nrm((C, Cp, 2, 2), 1.0 / math.sqrt(4 * Cp)), nrm((C,), 0.1)
        for j in range(n):
            b = p + f"blocks.{j}."
            sd[b + "conv_dw.weight"], sd[b + "conv_dw.bias"] = nrm((C, 1, 7, 7), 1.0 / 7.0), nrm((C,), 0.1)
            sd[b + "norm.weight"], sd[b + "norm.bias"] = 1.0 + nrm((C,), 0.1), nrm((C,), 0.1)
            sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = nrm((4 * C, C), 1.0 / math.sqrt(C)), nrm((4 * C,), 0.1)
            w2, b2 = nrm((C, 4 * C), 1.0 / math.sqrt(4 * C)), nrm((C,), 0.1)
            if hot is not None:
                w2[hot] *= outlier
                b2[hot] *= outlier
            sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = w2, b2
            sd[b + "gamma"] = torch.from_numpy(rng.uniform(0.1, 1.0, C).astype(np.float32))
    sd[T + "head.norm.weight"], sd[T + "head.norm.bias"] = 1.0 + nrm((dims[-1],), 0.1), nrm((dims[-1],), 0.1)
    sd["visual.head.proj.weight"] = nrm((E, dims[-1]), 1.0 / math.sqrt(dims[-1]))
    return sd


def synthetic_video_frames(n: int, h: int, w: int, seed: int = 0) -> "np.ndarray":
    """(n, h, w, 3) uint8 RGB test frames: smooth per-frame colour gradients plus noise, so the resize filters really average."""
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        a = rng.uniform(-1, 1, (3, 3))
        base = 128 + 90 * np.tanh(a[:, 0, None, None] * yy + a[:, 1, None, None] * xx + a[:, 2, None, None] * np.sin(6 * xx * yy + f))
        img = base.transpose(1, 2, 0) + rng.normal(0, 20, (h, w, 3))
        out[f] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def synthetic_edge_frames(n: int, h: int, w: int, seed: int = 0) -> "np.ndarray":
    """(n, h, w, 3) uint8 RGB test frames of hard edges, which a bicubic filter overshoots on both sides of [0, 255] (the smooth
    frames above never do): frame f cycles through vertical bars, horizontal bars and a checkerboard of 0 / 255 with a period of
    1 to 4 pixels on top of a coarse seeded 0 / 255 block pattern (so that the overshoot survives a reducing filter, which
    averages the fine pattern away), and a frame of saturated colours (every channel 0 or 255, in seeded blocks)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        px = 1 + (f // 4) % 4
        by, bx = max(1, h // int(rng.integers(3, 9))), max(1, w // int(rng.integers(3, 9)))
        coarse = rng.integers(0, 2, (h // by + 1, w // bx + 1, 3))[yy // by, xx // bx]          # (h, w, 3) of 0 / 1
        kind = f % 4
        if kind == 3:
            out[f] = (coarse * 255).astype(np.uint8)                                              # saturated colours
            continue
        fine = ((xx // px) % 2, (yy // px) % 2, (xx // px + yy // px) % 2)[kind]
        # fine pattern in the upper left half of every block, plain blocks elsewhere: edges at both scales
        use_fine = ((yy // by + xx // bx) % 2 == 0)
        grey = np.where(use_fine, fine, coarse[..., 0])
        out[f] = (grey * 255).astype(np.uint8)[..., None]
    return out


def random_hifigan_state_dict(config: dict, seed: int = 0) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of `Generator(h).state_dict()` after `remove_weight_norm()` (src/audioldm/hifigan/models.py; the
    real checkpoint is not reachable offline), `config` as `hifigan.HIFIGAN_16K_64`, in the order of `hifigan.expected_state_dict_shapes`
    from one numpy `RandomState(seed)`: weights ~ N(0, g^2 / fan_in) with fan_in = C_in k for a convolution and C_in k / u for a transposed
    one (each output frame meets k / u of its taps), g = 0.5 for the ResBlock convolutions (eighteen of them add to a stage's signal) and 1
    elsewhere; biases ~ 0.1 N(0, 1).  The module's own `init_weights` (std 0.01) gives waves of 1e-1 that test nothing."""
    import numpy as np
    from .hifigan import expected_state_dict_shapes as shapes

    rng = np.random.RandomState(seed)
    rates = tuple(config["upsample_rates"])
    sd = {}
    for key, shape in shapes(config).items():
        if key.endswith(".bias"):
            std = 0.1
        elif key.startswith("ups."):
            std = 1.0 / math.sqrt(shape[0] * shape[2] / rates[int(key.split(".")[1])])
        else:
            std = (0.5 if key.startswith("resblocks.") else 1.0) / math.sqrt(shape[1] * shape[2])
        sd[key] = torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32))
    return sd


def synthetic_log_mel(b: int, T: int, C: int = 64, seed: int = 0) -> torch.Tensor:
    """(b, C, T) fp32 log-mel-like frames, 2 N(0, 1) - 3 from numpy `RandomState(seed)`: the range of AudioLDM's log-mel images."""
    import numpy as np

    return torch.from_numpy((2.0 * np.random.RandomState(seed).standard_normal((b, C, T)) - 3.0).astype(np.float32))


def random_audioldm_vae_state_dict(config: dict, seed: int = 0, bias_std: float = 0.1) -> dict[str, torch.Tensor]:
    """Seeded weights in the key layout of the AudioLDM `AutoencoderKL`'s decoder half (`decoder.*` of
    src/audioldm/variational_autoencoder/modules.py `Decoder`, and `post_quant_conv.*`): seeded weights, not AudioLDM's;
    `config` as `audioldm_vae.AUDIOLDM_VAE`, in the order of `audioldm_vae.expected_state_dict_shapes` from one numpy `RandomState(seed)`:
    convolution weights ~ N(0, 1 / fan_in), norm weights 1 + 0.1 N(0, 1), every bias (the norms' included) ~ bias_std N(0, 1).
    bias_std = 3 is the "offset" regime: group means that dwarf the deviations and attention logits of tens.  torch's default
    initialisation gives an output that tests nothing."""
    import numpy as np
    from .audioldm_vae import expected_state_dict_shapes as shapes

    rng = np.random.RandomState(seed)
    sd = {}
    for key, shape in shapes(config).items():
        if key.endswith(".bias"):
            v = rng.standard_normal(shape) * bias_std
        elif len(shape) == 1:
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / math.sqrt(shape[1] * shape[2] * shape[3])
        sd[key] = torch.from_numpy(v.astype(np.float32))
    return sd


def synthetic_vae_latents(b: int, l: int, channels: int = 128, seed: int = 0) -> torch.Tensor:
    """(b, channels, l) fp32 latents ~ N(0, 1) from numpy `RandomState(seed)`: the `emb` of `VaeWrapper.decode`."""
    import numpy as np

    return torch.from_numpy(np.random.RandomState(seed).standard_normal((b, channels, l)).astype(np.float32))
