"""HiFi-GAN generator restated in torch, any dtype                                              *** TEST INFRASTRUCTURE ***

Written from the network's description: conv_pre, per stage leaky ReLU 0.1 -> ConvTranspose1d(k, u, (k - u) // 2) -> the
mean of the ResBlocks, leaky ReLU 0.01 -> conv_post -> tanh.  tests/golden/hifigan.npz, made by scripts/make_golden_hifigan.py from the
reference's own module, pins this file in float64 (tests/test_hifigan_host.py); the GPU tests and scripts/hifigan_probe.py then use it for
the shapes the fixture does not hold whole and for the torch-ops timing.  The cases of the fixture are defined here, for the script and
the tests alike."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from v2a_amd.hifigan import HIFIGAN_16K_64
from v2a_amd.synth import random_hifigan_state_dict, synthetic_log_mel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hifigan.npz")
REDUCED = dict(num_mels=80, upsample_initial_channel=128, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4),
               resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2, 4),) * 2)
CONFIGS = {"full": HIFIGAN_16K_64, "small": REDUCED}
PARAM_SEED = {"full": 1234, "small": 4321}
INPUT_SEED = 500
RAGGED_LENS, RAGGED_T = (5, 16, 9), 16
FULL_T, SMALL_T = (1, 4, 16), (3, 11)


def tap_names(config) -> list:
    n = len(config["upsample_rates"])
    return ["conv_pre"] + [f"{kind}{i}" for i in range(n) for kind in ("up", "mrf")] + ["pre", "wave"]


def ragged_mel() -> torch.Tensor:
    return synthetic_log_mel(len(RAGGED_LENS), RAGGED_T, 64, INPUT_SEED + 100)


def items(cfg_name: str) -> list:
    """(tag, mel (1, C, T)) of every single-clip run the fixture holds for a configuration; the ragged batch is its clips, each alone."""
    C = CONFIGS[cfg_name]["num_mels"]
    if cfg_name == "small":
        return [(f"t{T}", synthetic_log_mel(1, T, C, INPUT_SEED + T)) for T in SMALL_T]
    out = [(f"t{T}", synthetic_log_mel(1, T, C, INPUT_SEED + T)) for T in FULL_T]
    mel = ragged_mel()
    return out + [(f"ragged{i}", mel[i:i + 1, :, :n].contiguous()) for i, n in enumerate(RAGGED_LENS)]


_sd_cache: dict = {}


def state_dict(cfg_name: str) -> dict:
    """The seeded weights of a configuration, generated once per process and never changed."""
    if cfg_name not in _sd_cache:
        _sd_cache[cfg_name] = random_hifigan_state_dict(CONFIGS[cfg_name], PARAM_SEED[cfg_name])
    return _sd_cache[cfg_name]


def conv1d(x, w, b, d=1, slope=None, resid=None):
    """x (n, C, L): Conv1d with dilation d and "same" zero padding behind an optional leaky ReLU, plus an optional residual."""
    if slope is not None:
        x = F.leaky_relu(x, slope)
    y = F.conv1d(x, w, b, dilation=d, padding=(w.shape[2] - 1) * d // 2)
    return y if resid is None else y + resid


@torch.no_grad()
def generator(sd, mel, config, dtype=torch.float64) -> dict:
    """mel (n, C, T) -> every tap of `tap_names(config)` in `dtype`: "wave" and "pre" (n, samples), the others (n, C_s, frames)."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    rates, uks = config["upsample_rates"], config["upsample_kernel_sizes"]
    rks, dil = config["resblock_kernel_sizes"], config["resblock_dilation_sizes"]
    taps = {}
    x = taps["conv_pre"] = F.conv1d(mel.to(dtype), p["conv_pre.weight"], p["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(rates, uks)):
        x = taps[f"up{i}"] = F.conv_transpose1d(F.leaky_relu(x, 0.1), p[f"ups.{i}.weight"], p[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        total = None
        for j, ds in enumerate(dil):
            r, n = x, i * len(rks) + j
            for m, d in enumerate(ds):
                t = conv1d(r, p[f"resblocks.{n}.convs1.{m}.weight"], p[f"resblocks.{n}.convs1.{m}.bias"], d, 0.1)
                r = conv1d(t, p[f"resblocks.{n}.convs2.{m}.weight"], p[f"resblocks.{n}.convs2.{m}.bias"], 1, 0.1, resid=r)
            total = r if total is None else total + r
        x = taps[f"mrf{i}"] = total / len(rks)
    pre = F.conv1d(F.leaky_relu(x, 0.01), p["conv_post.weight"], p["conv_post.bias"], padding=3)
    taps["pre"], taps["wave"] = pre[:, 0], torch.tanh(pre)[:, 0]
    return taps


def to_int16(wave) -> np.ndarray:
    """`vocoder_infer`'s conversion: truncation toward zero."""
    return (wave.cpu().numpy() * 32768).astype("int16")
