"""CPU: tests/golden/clip_vit2_small.npz is what transformers computes -- the `small` case re-run through the generating script
(scripts/make_golden_clip_vit2.py) equals the committed fixture -- and the float64 QuickGELU formula the GPU test holds the epilogue to is
the library's QuickGELUActivation."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("make_golden_clip_vit2", os.path.join(ROOT, "scripts", "make_golden_clip_vit2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_fixture_is_reproduced_by_the_library():
    mod = _script()
    z = np.load(os.path.join(ROOT, "tests", "golden", "clip_vit2_small.npz"))
    meta = json.loads(str(z["meta"]))
    out, m2 = {}, dict(cases={})
    mod.run_case("small", out, m2)
    assert m2["cases"]["small"] == meta["cases"]["small"] and meta["cases"]["small"]["config"]["hidden_act"] == "quick_gelu"
    keys = [k for k in z.files if k.startswith("small_")]
    assert sorted(keys) == sorted(out) and any(k.endswith("_embeds") for k in keys)
    for k in keys:
        if k.endswith("_embeds"):
            assert z[k].dtype == np.float64 and float(np.abs(out[k] - z[k]).max()) <= 1e-12, k
        elif k.endswith("_md5"):
            assert list(out[k]) == list(z[k]), k
    # the other case of the file is of the same making
    assert sorted(meta["cases"]) == ["small", "small104"] and meta["cases"]["small104"]["config"]["num_attention_heads"] == 2


def test_quick_gelu_formula_is_the_librarys_activation():
    from transformers.activations import ACT2FN, QuickGELUActivation
    act = ACT2FN["quick_gelu"]
    assert isinstance(act, QuickGELUActivation)
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(4096, generator=g, dtype=torch.float64) * 3, torch.tensor([-1e4, -2e2, -50.0, -0.0, 0.0, 50.0, 2e2, 1e4], dtype=torch.float64)])
    want = act(v)
    assert torch.equal(v * torch.sigmoid(1.702 * v), want)
    # the form the kernels evaluate, v / (1 + exp(-1.702 v)): the same function, finite at both ends (exp overflows to inf, v / inf = -0)
    alt = v / (1 + torch.exp(-1.702 * v))
    assert bool(torch.isfinite(alt).all()) and float((alt - want).abs().max()) <= 1e-15 * float(want.abs().max())
    assert float(alt[-8]) == 0.0 and float(alt[-1]) == 1e4
