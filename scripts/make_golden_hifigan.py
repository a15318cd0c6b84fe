"""Generates tests/golden/hifigan.npz by running the REFERENCE module in float64 and fp32.      *** TEST INFRASTRUCTURE ***

`src/audioldm/hifigan/models.py` of the reference imports only torch, so `Generator` is loaded here straight from the read-only
reference tree (never copied), given a small attribute dict for `h`, stripped of weight norm (`remove_weight_norm()`), and loaded with
seeded weights (`strict=True`: every key of ours present, none extra).  Its float64 outputs pin tests/hifigan_ref.py and the HIP path;
its own fp32 run sets the error scale of every tap.

The fixture holds outputs only (weights and inputs are regenerated from seeds by v2a_amd.synth; the cases are tests/hifigan_ref.py's).
Per configuration c in (full, small) and case tag:
  {c}_{tag}_wave, _pre            float64, whole: the wave and the value in front of tanh, (samples,)
  {c}_{tag}_wave32, _pre32        the reference's own fp32 run
  {c}_{tag}_pcm                   `vocoder_infer`'s `(wav * 32768).astype("int16")` of the float64 wave
  {c}_{tag}_{tap}_shape/_stats/_idx/_val   conv_pre, up{i}, mrf{i}: shape, (mean, mean |.|, max, min) and 64 sampled entries, float64
  {c}_scale_{tap}                 max over the configuration's cases of |reference fp32 - reference float64|, every tap, pre and wave
  {c}_keys, {c}_shapes            the module's own key list, shapes as "AxBxC" strings

Usage:  python scripts/make_golden_hifigan.py  --reference DIR
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import v2a_amd  # noqa: E402,F401
import hifigan_ref as R  # noqa: E402


class AttrDict(dict):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.__dict__ = self


def load_reference_net(ref_root, cfg_name):
    path = os.path.join(ref_root, "src", "audioldm", "hifigan", "models.py")
    spec = importlib.util.spec_from_file_location("ref_hifigan_models", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = R.CONFIGS[cfg_name]
    net = mod.Generator(AttrDict({k: [list(d) for d in v] if k == "resblock_dilation_sizes" else (list(v) if isinstance(v, tuple) else v)
                                  for k, v in cfg.items()}))
    net.eval()
    net.remove_weight_norm()
    net.load_state_dict(R.state_dict(cfg_name), strict=True)          # every key present, none extra
    return net


def run(net, mel, config):
    """Every tap of one forward pass of the reference module, through hooks; the MRF mean from the ResBlocks' outputs by the module's
    own operations ((r0 + r1) + r2, divided by their number)."""
    taps, hooks, nk = {}, [], len(config["resblock_kernel_sizes"])
    keep = lambda name: (lambda m, i, o: taps.__setitem__(name, o.detach().clone()))
    hooks.append(net.conv_pre.register_forward_hook(keep("conv_pre")))
    hooks.append(net.conv_post.register_forward_hook(keep("pre")))
    for i, up in enumerate(net.ups):
        hooks.append(up.register_forward_hook(keep(f"up{i}")))
    for n, rb in enumerate(net.resblocks):
        hooks.append(rb.register_forward_hook(keep(f"rb{n}")))
    wave = net(mel)
    for h in hooks:
        h.remove()
    for i in range(len(net.ups)):
        xs = taps.pop(f"rb{i * nk}")
        for j in range(1, nk):
            xs += taps.pop(f"rb{i * nk + j}")
        taps[f"mrf{i}"] = xs / nk
    taps["pre"], taps["wave"] = taps["pre"][:, 0], wave[:, 0]
    return taps


def sample_idx(shape, k=64, seed=5):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, s, k) for s in shape], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds src/audioldm/hifigan/models.py)")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    rec = {}
    for c, cfg in R.CONFIGS.items():
        net32 = load_reference_net(args.reference, c)
        net = load_reference_net(args.reference, c).double()
        rec[f"{c}_keys"] = np.array(list(net.state_dict().keys()))
        rec[f"{c}_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in net.state_dict().values()])
        scale = {name: 0.0 for name in R.tap_names(cfg)}
        for tag, mel in R.items(c):
            t64, t32 = run(net, mel.double(), cfg), run(net32, mel, cfg)
            for name in scale:
                scale[name] = max(scale[name], float((t32[name].double() - t64[name]).abs().max()))
            for name in ("wave", "pre"):
                rec[f"{c}_{tag}_{name}"] = t64[name][0].numpy()
                rec[f"{c}_{tag}_{name}32"] = t32[name][0].numpy()
            rec[f"{c}_{tag}_pcm"] = (t64["wave"][0].numpy() * 32768).astype("int16")
            for name in R.tap_names(cfg)[:-2]:
                a = t64[name].numpy()
                ii = sample_idx(a.shape)
                rec[f"{c}_{tag}_{name}_shape"] = np.array(a.shape)
                rec[f"{c}_{tag}_{name}_stats"] = np.array([a.mean(), np.abs(a).mean(), a.max(), a.min()])
                rec[f"{c}_{tag}_{name}_idx"] = ii
                rec[f"{c}_{tag}_{name}_val"] = a[tuple(ii.T)]
            pre = t64["pre"][0]
            print(f"{c} {tag}: {mel.shape[2]} frames -> {pre.numel()} samples, pre-tanh std {float(pre.std()) if pre.numel() > 1 else 0:.3f} max "
                  f"{float(pre.abs().max()):.3f}, reference fp32 vs float64 pre-tanh {float((t32['pre'].double() - t64['pre']).abs().max()):.3e}")
        for name, v in scale.items():
            rec[f"{c}_scale_{name}"] = np.float64(v)
        print(c, "error scales:", ", ".join(f"{k} {v:.2e}" for k, v in scale.items()))
    out = R.GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
