"""Golden vectors of the HIP FLAN-T5 encoder (v2a_amd.T5Encoder): transformers' own T5EncoderModel, run in float64 on the CPU with
the seeded weights of v2a_amd.synth.random_t5_encoder_state_dict, writes tests/golden/t5_{small,full,amplified}.npz:
ids / mask / outputs (sampled rows where a sequence is long) and sampled rows of the residual stream after blocks 1, ceil(L/2), L.

    python scripts/make_golden_t5.py [small|full|amplified ...]
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

SMALL = dict(vocab_size=512, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=3, relative_attention_num_buckets=32,
             relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
AMPLIFY = 16.0
# sampled token rows per sequence (every column of a row is kept): 48 for the small model, 12 at d_model 1024, which keeps each
# full-size file under ~0.6 MB; row 0 and row N-1 (a padding row of every shorter prompt of the batch) are always among them
MAX_ROWS = {"small": 48, "full": 12, "amplified": 12}


def cases():
    from v2a_amd.synth import FLAN_T5_LARGE
    return {
        # name: (config, weight seed, amplify, [(lengths of one batch), ...], id seed)
        "small": (SMALL, 11, 1.0, [(9, 5, 13), (200,)], 21),
        "full": (FLAN_T5_LARGE, 12, 1.0, [(37, 21), (512,)], 22),
        "amplified": (FLAN_T5_LARGE, 13, AMPLIFY, [(29, 16)], 23),
    }


def taps_of(L):
    return sorted({1, math.ceil(L / 2), L})


def make_inputs(lengths, vocab, seed):
    """Right-padded ids (EOS = 1 closes every prompt, pad = 0) and the 0/1 mask, like the tokenizer at x3:1650."""
    rs = np.random.RandomState(seed)
    N = max(lengths)
    ids = np.zeros((len(lengths), N), np.int64)
    mask = np.zeros((len(lengths), N), np.int64)
    for b, n in enumerate(lengths):
        ids[b, :n - 1] = rs.randint(2, vocab, n - 1)
        ids[b, n - 1] = 1
        mask[b, :n] = 1
    return ids, mask


def sample_rows(N, seed, max_rows):
    if N <= max_rows:
        return np.arange(N)
    rs = np.random.RandomState(seed)
    return np.sort(np.concatenate([[0, N - 1], rs.choice(np.arange(1, N - 1), max_rows - 2, replace=False)]))


def run_case(name):
    import transformers
    from transformers import T5Config, T5EncoderModel
    from v2a_amd.synth import random_t5_encoder_state_dict
    cfg, wseed, amp, batches, iseed = cases()[name]
    sd = random_t5_encoder_state_dict(cfg, wseed, amp)
    model = T5EncoderModel(T5Config(**cfg, feed_forward_proj="gated-gelu", dropout_rate=0.0, is_encoder_decoder=False)).eval()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing if "embed_tokens" not in k] and not unexpected, (missing, unexpected)
    model = model.double()
    L = cfg["num_layers"]
    taps = taps_of(L)
    out = dict(meta=json.dumps(dict(config=cfg, weight_seed=wseed, amplify=amp, taps=taps, transformers=transformers.__version__,
                                    dtype="float64", batches=[list(b) for b in batches])))
    for bi, lengths in enumerate(batches):
        ids, mask = make_inputs(lengths, cfg["vocab_size"], iseed + bi)
        N = ids.shape[1]
        rows = sample_rows(N, iseed + 100 + bi, MAX_ROWS[name])
        got = {}
        hooks = [model.encoder.block[l - 1].register_forward_hook(
            lambda mod, inp, o, l=l: got.__setitem__(l, (o[0] if isinstance(o, tuple) else o).detach())) for l in taps]
        with torch.no_grad():
            hs = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))[0]
        for h in hooks:
            h.remove()
        p = f"b{bi}_"
        out[p + "ids"] = ids.astype(np.int32)
        out[p + "mask"] = mask.astype(np.int32)
        out[p + "rows"] = rows.astype(np.int32)
        out[p + "out"] = hs[:, rows].numpy().astype(np.float32)
        for l in taps:
            out[p + f"tap{l}"] = got[l][:, rows].numpy().astype(np.float32)
    return out


def main(names):
    os.makedirs(GOLDEN, exist_ok=True)
    for name in names:
        out = run_case(name)
        path = os.path.join(GOLDEN, f"t5_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or list(cases()))
