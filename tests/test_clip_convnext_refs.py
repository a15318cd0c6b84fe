"""CPU: what the GPU tests of the ConvNeXt encoder stand on.  tests/convnext_ref.py (the float64 restatement under timm's key names that
the eps 1e-5 GPU case relies on) equals, at eps 1e-6, the fixtures transformers' float64 `ConvNextModel` made
(tests/golden/clip_convnext_*.npz, scripts/make_golden_clip_convnext.py); the torchvision normalise table equals torch's fp32
ToTensor / Normalize operations bit for bit; `ResizePlan`'s torchvision crop offset reproduces the fixtures' Pillow crops, and its
default mode is what it was."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fx(name):
    z = np.load(os.path.join(GOLDEN, f"clip_convnext_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def _md5(a):
    return [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in a]


@pytest.mark.parametrize("name", ["small", "wide", "full"])
def test_restatement_equals_the_transformers_fixtures(name):
    import convnext_ref as R
    from v2a_amd.synth import random_convnext_state_dict, synthetic_video_frames
    z, meta = _fx(name)
    for cname, case in meta["cases"].items():
        assert case["eps"] == 1e-6 and max(case["fp32_err"].values()) <= 0.25 * 2e-5
        sd = R.bare_keys(random_convnext_state_dict(case["config"], case["seed"], case["outlier"]))
        for clip, n, h, w, fseed in case["clips"]:
            key = f"{cname}_{clip}"
            fr = synthetic_video_frames(n, h, w, fseed)
            assert _md5(fr) == list(z[key + "_frames_md5"])
            crop, pv = R.preprocess(fr, case["resize"], case["crop"])
            assert _md5(crop) == list(z[key + "_crop_md5"])
            assert np.array_equal(pv.reshape(n, -1)[:, z[key + "_pix_idx"]].numpy(), z[key + "_pix"])
            taps = {"stem": None, (2, 0): None, (2, case["config"]["depths"][2] - 1): None}
            taps.update({(s, d - 1): None for s, d in enumerate(case["config"]["depths"])})
            with torch.no_grad():
                got = R.forward(sd, pv.double(), 1e-6, taps).numpy()
            ref = z[key + "_embeds"]
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"{key}: convnext_ref vs ConvNextModel {err:.2e}")
            assert ref.dtype == np.float64 and err <= 1e-12, (key, err)
            names = {"stem": "stem", "s2b0": (2, 0), "s2bL": (2, case["config"]["depths"][2] - 1)}
            names.update({f"s{s}": (s, d - 1) for s, d in enumerate(case["config"]["depths"])})
            for t in case["taps"]:
                m = taps[names[t]]
                g = m.reshape(n, -1, m.shape[-1])[:, z[key + f"_tap_{t}_rows"]].numpy()
                assert float(np.abs(g - z[key + f"_tap_{t}"]).max()) <= 1e-6 * float(np.abs(g).max()), (key, t)      # stored as float32


def test_torchvision_normalize_table_is_torchs_fp32_arithmetic():
    from v2a_amd.resample import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, normalize_table
    for mean, std in ((OPENAI_CLIP_MEAN, OPENAI_CLIP_STD), ((0.5, 0.4, 0.3), (0.2, 0.3, 0.4))):
        u = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).repeat(3, 1, 1)             # a (3, 256, 1) "image": ToTensor's layout
        t = u.to(torch.float32).div(255)
        want = t.sub(torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)).div(torch.tensor(std, dtype=torch.float32).view(3, 1, 1))
        got = normalize_table(mean, std, formula="torchvision")
        assert got.dtype == np.float32 and got.shape == (3, 256)
        assert np.array_equal(got.view(np.uint32), want[:, :, 0].numpy().view(np.uint32))
    # the two formulas are the same function up to the rounding of u / 255 (a float64 product rounded once against an fp32 division: at
    # most an ulp apart, and for these statistics not at all), and the default is still the transformers one
    a, b = normalize_table(), normalize_table(formula="torchvision")
    assert (np.abs(a - b) <= np.spacing(np.abs(a))).all()
    assert np.array_equal(a, normalize_table(formula="transformers"))
    with pytest.raises(ValueError, match="formula"):
        normalize_table(formula="pil")


def test_resize_plan_torchvision_mode_reproduces_the_fixture_crops():
    from v2a_amd.resample import ResizePlan
    from v2a_amd.synth import synthetic_video_frames
    z, meta = _fx("small")
    bites = 0
    for cname, case in meta["cases"].items():
        for clip, n, h, w, fseed in case["clips"]:
            key = f"{cname}_{clip}"
            rp = ResizePlan(h, w, case["crop"], case["resize"], crop_offset="torchvision")
            floor = ResizePlan(h, w, case["crop"], case["resize"])
            bites += (rp.top, rp.left) != (floor.top, floor.left)
            fr = synthetic_video_frames(n, h, w, fseed)
            assert _md5(np.stack([rp.resize_numpy(f) for f in fr])) == list(z[key + "_crop_md5"]), key
    assert bites >= 3                      # half, halfp at 64 and land at 256: the floor would have cut one pixel further left / up
    rp = ResizePlan(360, 640, 256, 256, crop_offset="torchvision")
    assert rp.out_hw == (256, 455) and (rp.top, rp.left) == (0, 100)
    assert ResizePlan(360, 640, 256, 256).left == 99
    assert ResizePlan(640, 360, 256, 256, crop_offset="torchvision").top == 100
    assert ResizePlan(360, 641, 256, 256, crop_offset="torchvision").left == 100       # 200 / 2: even differences agree with the floor
    with pytest.raises(ValueError, match="crop_offset"):
        ResizePlan(360, 640, 256, 256, crop_offset="round")


def test_default_resize_plans_are_unchanged_for_the_vit_fixtures():
    """The default mode against the arithmetic it had: (h - S) // 2 offsets and the same tables, for every shape of the ViT fixtures."""
    from v2a_amd.resample import ResizePlan, resample_coeffs, resize_output_size, vertical_window
    shapes = set()
    for fam in ("clip", "clip_vit2", "dinov2"):
        for name in ("small", "wide", "full"):
            z = np.load(os.path.join(GOLDEN, f"{fam}_{name}.npz"))
            for case in json.loads(str(z["meta"]))["cases"].values():
                S = case.get("crop", case["config"]["image_size"])
                for c in case["clips"]:
                    shapes.add((c[2], c[3], S, case.get("resize", S)))
    assert len(shapes) >= 8
    for h, w, S, resize in sorted(shapes):
        rp = ResizePlan(h, w, S, resize)
        oh, ow = resize_output_size(h, w, resize)
        top, left = (oh - S) // 2, (ow - S) // 2
        assert (rp.top, rp.left) == (top, left)
        hb, hk = resample_coeffs(w, ow)
        vb, vk = resample_coeffs(h, oh)
        y0, rows, vbr = vertical_window(vb[top:top + S])
        assert np.array_equal(rp.hb, hb[left:left + S]) and np.array_equal(rp.hk, hk[left:left + S])
        assert (rp.y0, rp.rows) == (y0, rows) and np.array_equal(rp.vb, vbr) and np.array_equal(rp.vk, vk[top:top + S])
