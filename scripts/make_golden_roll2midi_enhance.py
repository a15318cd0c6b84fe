"""Generates tests/golden/roll2midi_enhance.npz by running the REFERENCE module in float64.          *** TEST INFRASTRUCTURE ***

`src/audeo/Roll2MidiNet_enhance.py` of the reference (the generator Roll2Midi_train.py and Roll2Midi_evaluate.py import) needs only
torch, so it is loaded here straight from the read-only reference tree (never copied) with seeded weights (`strict=True`: every key
of ours present, none extra) and seeded inputs; its float64 outputs pin `Roll2MidiEnhanceEngine`.  The window / pad / threshold lines
of Roll2Midi_inference.py (36-71) are re-run literally on this module, as scripts/make_golden_roll2midi.py does for the plain one.

The fixture holds outputs only (inputs and weights are regenerated from seeds by v2a_amd.synth, numpy RandomState):
  logits_{n}x{w}, probs_{n}x{w}   float64, (n, 1, 51, w) for (n, w) = (2, 7), (1, 50), (1, 100)
  logits32_{n}x{w}                the reference's own fp32 run of the same inputs (its deviation from float64 sets the fp32 logit bar)
  {tap}_{n}x{w}_shape/_stats/_idx/_val/_val32   d1..d6 (outputs of the down blocks), u1..u4 (outputs of att1..att4: the gated
                                  concatenations), u5 (output of up5), a1..a4 (the gates' alpha, (n, 1, 51, w)): shape, (mean,
                                  mean |.|, max, min), 64 sampled entries in float64 and the same entries of the fp32 run
  state_dict_keys, state_dict_shapes     the reference module's own key list, shapes as "AxBxC" strings
  refine_pad_probs, refine_pad_midi      the literal re-run for a 130-frame roll: float64 probabilities and the int roll, (130, 51)

The script ASSERTS that the seeded network is a test at all: 20 % .. 80 % of the thresholded cells on at every shape, at most 1 %
of the cells within 1e-4 of 0.5, and at every gate a logit std of at least 0.5 with at least 90 % of alpha inside (0.02, 0.98).

Usage:  python scripts/make_golden_roll2midi_enhance.py  --reference DIR
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
import v2a_amd  # noqa: E402,F401
from v2a_amd.synth import random_roll2midi_enhance_state_dict, synthetic_key_roll  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "roll2midi_enhance.npz")
PARAM_SEED, INPUT_SEED, REFINE_SEED = 4321, 77, 79
KEYS = 51
SHAPES = ((2, 7), (1, 50), (1, 100))
REFINE_FRAMES = 130
TAPS = [f"d{i}" for i in range(1, 7)] + [f"u{i}" for i in range(1, 6)] + [f"a{i}" for i in range(1, 5)]


def forward_input(n: int, w: int) -> torch.Tensor:
    """(n, 1, KEYS, w) fp32 probabilities of the forward cases; the tests regenerate them with this function's two lines."""
    return synthetic_key_roll(n, w, KEYS, INPUT_SEED + w).transpose(1, 2)[:, None].contiguous()


def refine_logits() -> np.ndarray:
    return synthetic_key_roll(1, REFINE_FRAMES, KEYS, REFINE_SEED, logits=True)[0].numpy()


def load_reference_net(ref_root):
    path = os.path.join(ref_root, "src", "audeo", "Roll2MidiNet_enhance.py")
    spec = importlib.util.spec_from_file_location("ref_Roll2MidiNet_enhance", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.Generator((1, KEYS, 100))
    net.load_state_dict(random_roll2midi_enhance_state_dict(PARAM_SEED), strict=True)      # every key present, none extra
    net.eval()
    return net


def tap_module(net, name):
    """The module whose output the tap is: down_k, att_k (the gated concatenation), up5, att_k.sigmoid (alpha)."""
    i = int(name[1])
    if name[0] == "d":
        return getattr(net, f"down{i}")
    if name[0] == "a":
        return getattr(net, f"att{i}").sigmoid
    return net.up5 if i == 5 else getattr(net, f"att{i}")


def hooked_run(net, x, extra=()):
    """net(x) -> (probabilities, {tap or extra name: output}); extra: (name, module) pairs."""
    got, hooks = {}, []
    for name, mod in [(t, tap_module(net, t)) for t in TAPS] + [("logits", net.conv1d)] + list(extra):
        hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: got.__setitem__(name, o.detach().clone())))
    probs = net(x)
    for h in hooks:
        h.remove()
    return probs, got


def sample_idx(shape, k=64, seed=5):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, s, k) for s in shape], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds src/audeo/Roll2MidiNet_enhance.py)")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    net32 = load_reference_net(args.reference)
    net = load_reference_net(args.reference).double()
    rec = {}
    # the module's own key list (strict=True above proves it equals the seeded state dict's): pins expected_enhance_state_dict_shapes()
    rec["state_dict_keys"] = np.array(list(net.state_dict().keys()))
    rec["state_dict_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in net.state_dict().values()])

    # ---- forward: float64 logits / probabilities / taps, and the reference's own fp32 run ----
    for n, w in SHAPES:
        tag = f"{n}x{w}"
        x = forward_input(n, w)
        probs, taps = hooked_run(net, x.double(), [(f"z{k}", getattr(net, f"att{k}").psi) for k in range(1, 5)])
        _, taps32 = hooked_run(net32, x)
        rec[f"logits_{tag}"] = taps.pop("logits").numpy()
        rec[f"logits32_{tag}"] = taps32.pop("logits").numpy()
        rec[f"probs_{tag}"] = probs.numpy()
        for k in range(1, 5):                                   # the gates must gate: spread logits, alpha away from 0, 1
            z, a = taps.pop(f"z{k}").numpy(), taps[f"a{k}"].numpy()
            inside = float(((a > 0.02) & (a < 0.98)).mean())
            print(f"forward {tag}: gate {k}: z mean {z.mean():+.3f} std {z.std():.3f}, alpha mean {a.mean():.3f}, inside (0.02, 0.98): {inside:.4f}")
            assert z.std() >= 0.5, (tag, k, z.std())
            assert inside >= 0.90, (tag, k, inside)
        for k in TAPS:
            a, a32 = taps[k].numpy(), taps32[k].numpy()
            ii = sample_idx(a.shape)
            rec[f"{k}_{tag}_shape"] = np.array(a.shape)
            rec[f"{k}_{tag}_stats"] = np.array([a.mean(), np.abs(a).mean(), a.max(), a.min()])
            rec[f"{k}_{tag}_idx"] = ii
            rec[f"{k}_{tag}_val"] = a[tuple(ii.T)]
            rec[f"{k}_{tag}_val32"] = a32[tuple(ii.T)].astype(np.float64)
        z, p = rec[f"logits_{tag}"], rec[f"probs_{tag}"]
        on, near = float((p >= 0.5).mean()), float((np.abs(p - 0.5) <= 1e-4).mean())
        dev32 = float(np.abs(rec[f"logits32_{tag}"] - z).max())
        print(f"forward {tag}: logits std {z.std():.3f}, cells on {on:.4f}, within 1e-4 of 0.5: {near:.4%} of {z.size}, "
              f"reference fp32 vs float64 logits {dev32:.3e}")
        assert 0.20 <= on <= 0.80, (tag, on)
        assert near <= 0.01, (tag, near)

    # ---- refine(tail="pad"): Roll2Midi_inference.py:36-71 re-run on the reference module, self.frame = 50 ----
    # 130 frames are pieces of 50, 50 and 30 frames.  The reference pairs the pieces and silently drops an unpaired last one (:44-49), so
    # an empty fourth piece is supplied: lines 39-42 turn it into all-zero logits, which is what a padded tail is.
    frame = 50
    logit = refine_logits()
    pieces = [logit[s:s + frame] for s in range(0, 4 * frame, frame)]
    data = []
    for est_roll in pieces:                                               # :36-43
        if est_roll.shape[0] != frame:
            target = np.zeros((frame, KEYS))
            target[:est_roll.shape[0], :] = est_roll
            est_roll = target
        data.append(torch.from_numpy(est_roll))
    final_data = []
    for i in range(0, len(data), 2):                                      # :44-49
        if i + 1 < len(data):
            final_data.append(torch.cat([data[i], data[i + 1]], dim=0))
    test_results, test_probs = [], []
    for d in final_data:                                                  # :57-71, the module in float64 instead of cuda fp32
        roll = torch.unsqueeze(torch.unsqueeze(torch.sigmoid(d.T.float()), dim=0), dim=0)
        gen_img = net(roll.double())
        test_probs.append(np.transpose(gen_img.numpy().squeeze(), (1, 0)))
        gen_img = gen_img >= 0.5
        numpy_pre_label = gen_img.cpu().detach().numpy().astype(int)
        numpy_pre_label = np.transpose(numpy_pre_label.squeeze(), (1, 0))
        test_results.append(numpy_pre_label[:frame, :])
        test_results.append(numpy_pre_label[frame:, :])
    rec["refine_pad_midi"] = np.concatenate(test_results)[:REFINE_FRAMES].astype(np.uint8)
    rec["refine_pad_probs"] = np.concatenate(test_probs)[:REFINE_FRAMES]
    on, near = float(rec["refine_pad_midi"].mean()), float((np.abs(rec["refine_pad_probs"] - 0.5) <= 1e-4).mean())
    print(f"refine: {rec['refine_pad_midi'].shape}, cells on {on:.4f}, within 1e-4 of 0.5: {near:.4%}")
    assert 0.20 <= on <= 0.80 and near <= 0.01, (on, near)

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
