"""GPU: the HIP piano-frame preprocessor (piano_frames.py, csrc/piano_frames.hip) against Pillow's own bytes
(tests/golden/piano_frames.npz, scripts/make_golden_piano_frames.py): bit equality for every fixture case, with frame selection and
any chunk size, and `E2TTS.sample(video_frames=..., piano=True)` / `encode_video_frames` end to end."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "piano_frames.npz")
DEV = "cuda:0"


def _fx():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _case_frames(case, z):
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    name, H, W, ns, ne, seed, _ = case
    fr = np.concatenate([synthetic_video_frames(ns, H, W, seed), synthetic_edge_frames(ne, H, W, seed + 100)])
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr]
    assert md5 == list(z[name + "_frames_md5"]), f"{name}: the seeded frames differ from the ones the fixture was made from"
    return fr


def _check(got: torch.Tensor, z, name, frames):
    """`got` (n, 100, 900) on the device must be the fixture's output frames `frames` (a list of frame numbers), bit for bit."""
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == (len(frames), 100, 900), (name, g.shape, g.dtype)
    idx, vals = z[name + "_idx"], z[name + "_vals"]
    samp = g.reshape(len(frames), -1)[:, idx]
    want = vals[np.array(frames)]
    bad = samp != want
    print(f"{name}: frames {list(frames)}: {int(bad.sum())} of {bad.size} sampled values differ, max |d| = {float(np.abs(samp - want).max()):.3e}")
    assert not bad.any(), (name, [(int(f), int(idx[i]), float(samp[f, i]), float(want[f, i])) for f, i in zip(*np.nonzero(bad))][:8])
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in g]
    assert md5 == [z[name + "_out_md5"][j] for j in frames], name


@pytest.mark.parametrize("ci", range(7))
def test_kernels_equal_pillow_bit_for_bit(ci):
    """Every fixture case: all frames (one launch pair over the whole clip, sel = NULL), a selection that repeats and reorders
    frames, and chunks of 1, 3 and all frames -- the same bytes every time."""
    from v2a_amd.piano_frames import PianoFramePreprocessor
    z, meta = _fx()
    case = meta["cases"][ci]
    name = case[0]
    fr = _case_frames(case, z)
    F = len(fr)
    pre = PianoFramePreprocessor(DEV)
    whole = pre(fr)                                                    # host array, chunk 64 >= F: the sel = NULL path
    _check(whole, z, name, list(range(F)))
    frd = torch.from_numpy(fr).to(DEV)
    for chunk in (1, 3, F):
        got = pre(frd, chunk=chunk)                                    # a device tensor
        assert torch.equal(got, whole), (name, chunk)
    sel = [F - 1, 0, 2 % F, 0, F - 1, 1 % F, 1 % F]
    for chunk in (1, 3, len(sel)):
        for src in (fr, frd):                                          # host frames: only the distinct ones are uploaded
            got = pre(src, select=sel, chunk=chunk)
            _check(got, z, name, sel)
    assert pre(frd, select=[]).shape == (0, 100, 900)
    with pytest.raises(IndexError):
        pre(frd, select=[F])
    with pytest.raises(ValueError):
        pre(frd.float())


def test_other_output_size_and_unaligned_width():
    """Ho x Wo are parameters: a width that is no multiple of 4 (padded tmp rows, scalar stores) against the host restatement."""
    from v2a_amd.piano_frames import PianoFramePlan, PianoFramePreprocessor
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    for (H, W, Ho, Wo) in ((121, 203, 37, 41), (64, 97, 50, 333), (30, 2701, 100, 900)):
        fr = np.concatenate([synthetic_video_frames(2, H, W, 3), synthetic_edge_frames(3, H, W, 4)])
        want = PianoFramePlan(H, W, Ho, Wo).preprocess_numpy(fr)
        pre = PianoFramePreprocessor(DEV, Ho, Wo, chunk=2)
        assert np.array_equal(pre(fr).cpu().numpy(), want), (H, W, Ho, Wo)
        assert np.array_equal(pre(fr, select=[4, 1, 1]).cpu().numpy(), want[[4, 1, 1]]), (H, W, Ho, Wo)


# ---- E2TTS wiring -----------------------------------------------------------------------------------------------------------------
def _model():
    from conftest import make_model
    from oracle import e2_cfm_oracle as O
    from v2a_amd.synth import random_video2roll_state_dict
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=16,
                      max_seq_len=256)
    P = O.init_params(cfg, 1234)
    y0, text, _, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=99, piano=True)
    m = make_model(cfg, {**P, **{"video2roll_net." + k: v for k, v in random_video2roll_state_dict(1).items()}}, "fp32", device=DEV)
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, steps=4, cfg_strength=2.0, remove_parallel_component=False,
              return_raw_output=True)
    return m, kw


class _Counting:
    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.inner(*a, **k)


def test_sample_with_video_frames_and_piano(tmp_path):
    """The default frames mode (fp32 under compute_dtype fp32): preprocessing on the GPU adds no arithmetic difference, so the
    sampler's output is equal, not close, to the one from the stack built on the host."""
    from v2a_amd.features import piano_frame_indices, piano_frames_cache_path
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    m, kw = _model()
    l = 40
    # 24 frames over 1.0 s (24 fps) and 9 frames over 0.9 s (10 fps: frames repeat); different sizes
    clips = [(np.concatenate([synthetic_video_frames(20, 72, 128, 1), synthetic_edge_frames(4, 72, 128, 2)]), 1.0),
             (synthetic_video_frames(9, 90, 160, 3), 0.9)]
    idx = [piano_frame_indices(len(f), d, l) for f, d in clips]
    t = max(l // 3 + 1, max(map(len, idx)))
    stack = torch.zeros(2, 1, t, 100, 900)
    for b, ((f, d), ix) in enumerate(zip(clips, idx)):
        stack[b, 0, :len(ix)] = torch.from_numpy(PianoFramePlan(*f.shape[1:3]).preprocess_numpy(f))[torch.tensor(ix)]
    cond = torch.zeros(2, l, 16)
    ref = m.sample(cond, frames=stack, **kw)
    pre = m.piano_frame_preprocessor()
    got = m.sample(cond, video_frames=clips, piano=True, **kw)
    assert torch.equal(got, ref)
    assert pre.frames_done == sum(len(set(ix)) for ix in idx)                        # no paths: only the frames in use
    assert float((got - m.sample(cond, **kw)).abs().max()) > 0                      # the frames do condition the result
    assert torch.equal(m.sample(cond, video_frames=clips, **kw), m.sample(cond, **kw))          # piano=False: frames are not used
    # the stack itself, and the return convention
    frames, midis = m.encode_video_frames(None, l, True, video_frames=clips)
    assert frames.device.type == "cuda" and torch.equal(frames.cpu(), stack)
    assert midis.shape == (2, l, 51) and float(midis.abs().max()) == 0.0
    assert m.encode_video_frames(None, l, False, video_frames=clips) == (None, None)
    assert m.encode_video_frames(None, l, True, video_frames=[None, None]) == (None, None)
    assert m.encode_video_frames([None, None], l, True, video_frames=clips) == (None, None)
    one, _ = m.encode_video_frames(None, l, True, video_frames=[None, clips[1]])
    assert float(one[0].abs().max()) == 0.0 and torch.equal(one[1].cpu(), stack[1])
    # video_paths: caches written in the reference's layout, honoured by the second call
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    m._piano_pre = counting = _Counting(pre)
    first = m.sample(cond, video_paths=paths, video_frames=clips, piano=True, **kw)
    assert counting.calls == 2 and torch.equal(first, ref)
    for p, (f, d) in zip(paths, clips):
        data = np.load(piano_frames_cache_path(p))
        assert data["arr_0"].shape == (len(f), 100, 900, 1) and data["arr_0"].dtype == np.float32 and data["arr_1"].item() == d
        assert np.array_equal(data["arr_0"][..., 0], PianoFramePlan(*f.shape[1:3]).preprocess_numpy(f))
    second = m.sample(cond, video_paths=paths, video_frames=clips, piano=True, **kw)
    assert counting.calls == 2 and torch.equal(second, first)
    fr2, _ = m.encode_video_frames(paths, l, True)                                   # the caches alone
    assert counting.calls == 2 and torch.equal(fr2, stack)
