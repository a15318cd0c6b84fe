"""AudioLDM VAE decoder restated in torch, any dtype                                            *** TEST INFRASTRUCTURE ***

Written from the network's description: post_quant_conv of z / scale_factor, conv_in, the middle (ResnetBlock, AttnBlock,
ResnetBlock), per level num_res_blocks + 1 ResnetBlocks and a nearest x2 Upsample with its convolution, norm_out, swish, conv_out.
tests/golden/audioldm_vae.npz, made by scripts/make_golden_audioldm_vae.py from the reference's own module, pins this file in float64
(tests/test_audioldm_vae_host.py); the GPU tests and scripts/audioldm_vae_probe.py then use it for the taps the fixture samples and for
the torch-ops timing.  The cases of the fixture are defined here, for the script and the tests alike."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from v2a_amd.audioldm_vae import AUDIOLDM_VAE, tap_names  # noqa: F401
from v2a_amd.synth import random_audioldm_vae_state_dict, synthetic_vae_latents

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audioldm_vae.npz")
REDUCED = dict(ch=32, ch_mult=(1, 2), num_res_blocks=1, z_channels=8)          # groups of 1 and 2 channels
CONFIGS = {"full": AUDIOLDM_VAE, "small": REDUCED}
REGIMES = {"plain": 0.1, "offset": 3.0}                                          # bias_std: offset = group means that dwarf the deviations
PARAM_SEED = {("full", "plain"): 2201, ("full", "offset"): 2202, ("small", "plain"): 2203, ("small", "offset"): 2204}
INPUT_SEED = 700
RAGGED_LENS, RAGGED_L, RAGGED_SCALE = (5, 16, 9), 16, 0.5
FULL_L, SMALL_L = (1, 2, 5, 16, 40), (3, 11)                                    # 40: 640 tokens, P V's K spans two launches of 512
CHANNELS = 128


def ragged_emb() -> torch.Tensor:
    return synthetic_vae_latents(len(RAGGED_LENS), RAGGED_L, CHANNELS, INPUT_SEED + 100)


def items(cfg_name: str) -> list:
    """(tag, emb (1, 128, l), scale_factor) of every single-clip run the fixture holds for a configuration; the ragged batch is its
    clips, each alone."""
    if cfg_name == "small":
        return [(f"l{l}", synthetic_vae_latents(1, l, CHANNELS, INPUT_SEED + l), 1.0) for l in SMALL_L]
    out = [(f"l{l}", synthetic_vae_latents(1, l, CHANNELS, INPUT_SEED + l), 1.0) for l in FULL_L]
    emb = ragged_emb()
    return out + [(f"ragged{i}", emb[i:i + 1, :, :n].contiguous(), RAGGED_SCALE) for i, n in enumerate(RAGGED_LENS)]


_sd_cache: dict = {}


def state_dict(cfg_name: str, regime: str) -> dict:
    """The seeded weights of a configuration and regime, generated once per process and never changed."""
    key = (cfg_name, regime)
    if key not in _sd_cache:
        _sd_cache[key] = random_audioldm_vae_state_dict(CONFIGS[cfg_name], PARAM_SEED[key], REGIMES[regime])
    return _sd_cache[key]


def to_z(emb: torch.Tensor) -> torch.Tensor:
    """`VaeWrapper.decode`'s reshape: emb (b, 128, l) -> z (b, 8, l, 16)."""
    b, c, l = emb.shape
    return emb.transpose(1, 2).reshape(b, l, c // 16, 16).transpose(1, 2)


def swish(x):
    return x * torch.sigmoid(x)


def norm(p, pre, x):
    return F.group_norm(x, 32, p[pre + ".weight"], p[pre + ".bias"], eps=1e-6)


def conv(p, pre, x, pad):
    return F.conv2d(x, p[pre + ".weight"], p[pre + ".bias"], padding=pad)


def resnet_block(p, pre, x):
    h = conv(p, pre + ".conv1", swish(norm(p, pre + ".norm1", x)), 1)
    h = conv(p, pre + ".conv2", swish(norm(p, pre + ".norm2", h)), 1)
    if pre + ".nin_shortcut.weight" in p:
        x = conv(p, pre + ".nin_shortcut", x, 0)
    return x + h


def attn_block(p, pre, x):
    h = norm(p, pre + ".norm", x)
    b, c, hh, ww = h.shape
    q, k, v = (conv(p, f"{pre}.{n}", h, 0).reshape(b, c, hh * ww) for n in ("q", "k", "v"))
    w = torch.softmax(torch.bmm(q.transpose(1, 2), k) * (int(c) ** -0.5), dim=2)                     # (b, query, key)
    o = torch.bmm(v, w.transpose(1, 2)).reshape(b, c, hh, ww)
    return x + conv(p, pre + ".proj_out", o, 0)


@torch.no_grad()
def decoder(sd, z, config, scale_factor=1.0, dtype=torch.float64) -> dict:
    """z (n, zc, l, 16) -> every tap of `tap_names(config)` in `dtype`, (n, C, H, W); "mel" is (n, 1, 2^(levels - 1) l, 16 * 2^(levels - 1))."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    levels, nrb = len(config["ch_mult"]), int(config["num_res_blocks"])
    taps = {}
    h = conv(p, "post_quant_conv", z.to(dtype) / scale_factor, 0)
    h = taps["conv_in"] = conv(p, "decoder.conv_in", h, 1)
    h = taps["mid1"] = resnet_block(p, "decoder.mid.block_1", h)
    h = taps["attn"] = attn_block(p, "decoder.mid.attn_1", h)
    h = taps["mid2"] = resnet_block(p, "decoder.mid.block_2", h)
    for i in reversed(range(levels)):
        for j in range(nrb + 1):
            h = taps[f"up{i}b{j}"] = resnet_block(p, f"decoder.up.{i}.block.{j}", h)
        if i:
            h = taps[f"up{i}us"] = conv(p, f"decoder.up.{i}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"), 1)
    taps["mel"] = conv(p, "decoder.conv_out", swish(norm(p, "decoder.norm_out", h)), 1)
    return taps
