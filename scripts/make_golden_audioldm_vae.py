"""Generates tests/golden/audioldm_vae.npz by running the REFERENCE module in float64 and fp32.   *** TEST INFRASTRUCTURE ***

`Decoder` of the reference's src/audioldm/variational_autoencoder/modules.py is loaded here straight from the read-only reference tree
(never copied).  The file imports `audioldm.utils` and `audioldm.latent_diffusion.attention`, whose own imports need packages that are
not installed, so empty `audioldm`, `audioldm.latent_diffusion` and `audioldm.variational_autoencoder` packages and an `audioldm.utils`
with a dummy `instantiate_from_config` are registered first, and latent_diffusion/util.py, latent_diffusion/attention.py and
variational_autoencoder/modules.py are then executed by path.  `decode_first_stage` is the module's `Decoder` behind a `Conv2d` for
`post_quant_conv` and the division by `scale_factor` (autoencoder.py), loaded with seeded weights (`strict=True`: every key of ours
present, none extra).  Its float64 outputs pin tests/audioldm_vae_ref.py and the HIP path; its own fp32 run sets the error scale of
every tap.

The fixture holds outputs only (weights and inputs are regenerated from seeds by v2a_amd.synth; the cases are tests/audioldm_vae_ref.py's).
Per configuration c in (full, small), regime r in (plain, offset) and case tag:
  {c}_{r}_{tag}_mel, _mel32                 the mel image (4 l, 64), float64 and the reference's own fp32 run, whole
  {c}_{r}_{tag}_tap_shape/_stats/_idx/_val  every tap but mel, stacked in the order of `tap_names`: shape, (mean, mean |.|, max, min),
                                            the indices of 64 sampled entries and their float64 values
  {c}_{r}_scale                             max over the cases of |reference fp32 - reference float64|, per tap of `tap_names`
  {c}_keys, {c}_shapes                      the module's own key list (`decoder.*`, `post_quant_conv.*`), shapes as "AxBxC" strings

Usage:  python scripts/make_golden_audioldm_vae.py  --reference DIR
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import v2a_amd  # noqa: E402,F401
import audioldm_vae_ref as R  # noqa: E402


def load_reference_modules(ref_root):
    base = os.path.join(ref_root, "src", "audioldm")
    for name in ("audioldm", "audioldm.latent_diffusion", "audioldm.variational_autoencoder"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    utils = types.ModuleType("audioldm.utils")
    utils.instantiate_from_config = lambda *a, **kw: None
    sys.modules["audioldm.utils"] = utils

    def run(name, *rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    run("audioldm.latent_diffusion.util", "latent_diffusion", "util.py")
    run("audioldm.latent_diffusion.attention", "latent_diffusion", "attention.py")
    return run("audioldm.variational_autoencoder.modules", "variational_autoencoder", "modules.py")


class FirstStage(torch.nn.Module):
    """`decode_first_stage` of the reference: z / scale_factor -> post_quant_conv -> the module's own Decoder."""

    def __init__(self, mod, config):
        super().__init__()
        zc = config["z_channels"]
        self.decoder = mod.Decoder(ch=config["ch"], out_ch=1, ch_mult=tuple(config["ch_mult"]), num_res_blocks=config["num_res_blocks"],
                                   attn_resolutions=[], dropout=0.0, in_channels=1, resolution=256, z_channels=zc, double_z=True)
        self.post_quant_conv = torch.nn.Conv2d(zc, zc, 1)

    def forward(self, z, scale_factor):
        return self.decoder(self.post_quant_conv(1.0 / scale_factor * z))


def run(net, z, scale_factor, config):
    """Every tap of one forward pass of the reference module, through hooks."""
    taps, hooks = {}, []
    keep = lambda name: (lambda m, i, o: taps.__setitem__(name, o.detach().clone()))
    d = net.decoder
    for name, m in (("conv_in", d.conv_in), ("mid1", d.mid.block_1), ("attn", d.mid.attn_1), ("mid2", d.mid.block_2)):
        hooks.append(m.register_forward_hook(keep(name)))
    for i, up in enumerate(d.up):
        for j, blk in enumerate(up.block):
            hooks.append(blk.register_forward_hook(keep(f"up{i}b{j}")))
        if i:
            hooks.append(up.upsample.register_forward_hook(keep(f"up{i}us")))
    taps["mel"] = net(z, scale_factor)
    for h in hooks:
        h.remove()
    assert sorted(taps) == sorted(R.tap_names(config))
    return taps


def sample_idx(shape, k=64, seed=5):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, s, k) for s in shape], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds src/audioldm/variational_autoencoder/modules.py)")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    mod = load_reference_modules(args.reference)
    rec = {}
    for c, cfg in R.CONFIGS.items():
        for r in R.REGIMES:
            net32 = FirstStage(mod, cfg).eval()
            net32.load_state_dict(R.state_dict(c, r), strict=True)        # every key present, none extra
            net = FirstStage(mod, cfg).eval()
            net.load_state_dict(R.state_dict(c, r), strict=True)
            net = net.double()
            rec[f"{c}_keys"] = np.array(list(net.state_dict().keys()))
            rec[f"{c}_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in net.state_dict().values()])
            scale = {name: 0.0 for name in R.tap_names(cfg)}
            for tag, emb, sf in R.items(c):
                z = R.to_z(emb)
                t64, t32 = run(net, z.double(), sf, cfg), run(net32, z, sf, cfg)
                for name in scale:
                    scale[name] = max(scale[name], float((t32[name].double() - t64[name]).abs().max()))
                rec[f"{c}_{r}_{tag}_mel"] = t64["mel"][0, 0].numpy()
                rec[f"{c}_{r}_{tag}_mel32"] = t32["mel"][0, 0].numpy()
                names = R.tap_names(cfg)[:-1]
                arrs = [t64[name].numpy() for name in names]
                idx = [sample_idx(a.shape) for a in arrs]
                rec[f"{c}_{r}_{tag}_tap_shape"] = np.array([a.shape for a in arrs], dtype=np.int32)
                rec[f"{c}_{r}_{tag}_tap_stats"] = np.array([[a.mean(), np.abs(a).mean(), a.max(), a.min()] for a in arrs])
                rec[f"{c}_{r}_{tag}_tap_idx"] = np.stack(idx).astype(np.int16)                       # every dim is below 2^15
                rec[f"{c}_{r}_{tag}_tap_val"] = np.stack([a[tuple(ii.T)] for a, ii in zip(arrs, idx)])
                mel = t64["mel"]
                print(f"{c} {r} {tag}: l = {z.shape[2]} -> mel {tuple(mel.shape)}, |max| {float(mel.abs().max()):.3f}, attention input |max| "
                      f"{float(t64['mid1'].abs().max()):.1f}, reference fp32 vs float64 mel {float((t32['mel'].double() - mel).abs().max()):.3e}")
            rec[f"{c}_{r}_scale"] = np.array([scale[name] for name in R.tap_names(cfg)])
            print(c, r, "error scales:", ", ".join(f"{k} {v:.2e}" for k, v in scale.items()))
    out = R.GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
