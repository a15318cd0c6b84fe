"""Reading the weights of the transformers models behind the HIP encoders (clip.py, dinov2.py, t5.py): a local HF directory, and the
key prefixes a reference checkpoint stores them under."""
from __future__ import annotations

import json
import os

import torch


def read_hf_dir(path: str) -> tuple[dict, dict[str, torch.Tensor]]:
    """A local HF directory -> (config.json, the state dict of model.safetensors, else of pytorch_model.bin)."""
    with open(os.path.join(path, "config.json")) as f:
        hc = json.load(f)
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return hc, load_file(st)
    return hc, torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")


def strip_keys(state_dict, prefixes: tuple[str, ...]) -> dict[str, torch.Tensor]:
    """The model's plain keys from its own state dict, or from a reference checkpoint (optionally under `model_state_dict`) that
    holds it under one of `prefixes` (`image_encoder.`, `text_encoder2.`): then only those keys are kept, without the prefix."""
    sd = state_dict.get("model_state_dict", state_dict) if isinstance(state_dict, dict) else state_dict
    if any(k.startswith(prefixes) for k in sd):
        return {k[len(p):]: v for k, v in sd.items() for p in prefixes if k.startswith(p)}
    return dict(sd)
