"""CPU: the host half of the piano-frame preprocessor (piano_frames.py) -- Pillow's grey conversion and integer BICUBIC resample
restated from the module's tables, against live Pillow and against tests/golden/piano_frames.npz
(scripts/make_golden_piano_frames.py) -- the frame selection / cache wiring of features.py and E2TTS, and the library's exports."""
import glob
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "piano_frames.npz")


def _fx():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _case_frames(case):
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    _, H, W, ns, ne, seed, _ = case
    return np.concatenate([synthetic_video_frames(ns, H, W, seed), synthetic_edge_frames(ne, H, W, seed + 100)])


def _md5s(a):
    return [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in a]


def _pillow(frames):
    """The reference's steps (x3:60-63, 1883-1890) on Pillow itself."""
    from PIL import Image
    out = []
    for f in frames:
        grey = np.array(Image.fromarray(f).convert("L"))
        img = Image.fromarray(grey.astype(np.uint8)).resize((900, 100))
        out.append(np.transpose(np.reshape(img, (100, 900, 1)), [2, 0, 1]) / 255.)
    return np.concatenate(out).astype(np.float32)


# ---- the integer restatement ---------------------------------------------------------------------------------------------------
def test_fixture_cases_are_the_ones_the_preprocessor_must_cover():
    _, meta = _fx()
    assert {(c[1], c[2]) for c in meta["cases"]} == {(360, 640), (1080, 1920), (100, 900), (100, 640), (360, 900), (90, 160), (241, 427)}


@pytest.mark.parametrize("ci", range(7))
def test_preprocess_numpy_equals_fixture(ci):
    """Without Pillow: md5 of every output frame's float32 bytes; sampled values make a mismatch readable."""
    from v2a_amd.piano_frames import PianoFramePlan
    z, meta = _fx()
    case = meta["cases"][ci]
    name, H, W = case[:3]
    fr = _case_frames(case)
    assert _md5s(fr) == list(z[name + "_frames_md5"]), f"{name}: the seeded frames differ from the ones the fixture was made from"
    got = PianoFramePlan(H, W).preprocess_numpy(fr)
    assert got.dtype == np.float32 and got.shape == (len(fr), 100, 900)
    samp = got.reshape(len(fr), -1)[:, z[name + "_idx"]]
    assert np.array_equal(samp, z[name + "_vals"]), (name, int((samp != z[name + "_vals"]).sum()), float(np.abs(samp - z[name + "_vals"]).max()))
    assert _md5s(got) == list(z[name + "_out_md5"]), name


@pytest.mark.parametrize("ci", range(7))
def test_preprocess_numpy_equals_live_pillow_on_fixture_cases(ci):
    pytest.importorskip("PIL")
    from v2a_amd.piano_frames import PianoFramePlan
    case = _fx()[1]["cases"][ci]
    fr = _case_frames(case)
    assert np.array_equal(PianoFramePlan(case[1], case[2]).preprocess_numpy(fr), _pillow(fr)), case[0]


@pytest.mark.parametrize("hw", [(224, 224), (250, 300), (640, 360), (448, 700), (900, 1344), (1344, 900), (150, 200), (97, 50),
                                (227, 301), (1350, 1500), (720, 1280), (100, 901), (101, 900), (33, 2700), (300, 30)])
def test_preprocess_numpy_equals_live_pillow_over_sizes(hw):
    """Reduce 1x .. 13x, enlarge up to 30x, both orientations, sizes next to the output's: noise over a random walk (the filters
    really average) and a frame of hard 0 / 255 edges (both clips act)."""
    pytest.importorskip("PIL")
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_edge_frames
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    smooth = np.cumsum(rng.normal(0, 6, hw + (3,)), axis=1)
    img = np.clip(128 + smooth - smooth.mean() + rng.normal(0, 30, hw + (3,)), 0, 255).astype(np.uint8)
    fr = np.concatenate([img[None], synthetic_edge_frames(2, hw[0], hw[1], hw[0] + hw[1])])
    plan = PianoFramePlan(*hw)
    assert np.array_equal(plan.preprocess_numpy(fr), _pillow(fr)), hw
    # the tables stay inside the image: what the kernels read
    assert (plan.hb[:, 0] >= 0).all() and (plan.hb[:, 0] + plan.hb[:, 1] <= hw[1]).all()
    assert (plan.vb[:, 0] >= 0).all() and (plan.vb[:, 0] + plan.vb[:, 1] <= plan.rows).all() and plan.y0 + plan.rows <= hw[0]


def test_other_output_sizes_equal_live_pillow():
    """Ho x Wo is a parameter; 100 x 900 is only the caller's value."""
    pytest.importorskip("PIL")
    from PIL import Image
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_video_frames
    fr = synthetic_video_frames(2, 120, 200, 3)
    for Ho, Wo in ((50, 333), (37, 41), (240, 400)):
        want = np.stack([np.asarray(Image.fromarray(f).convert("L").resize((Wo, Ho))) / 255. for f in fr]).astype(np.float32)
        assert np.array_equal(PianoFramePlan(120, 200, Ho, Wo).preprocess_numpy(fr), want), (Ho, Wo)


def test_scale_table_is_the_float64_division_cast_to_float32():
    from v2a_amd.piano_frames import PianoFramePlan, scale_table
    want = (np.arange(256, dtype=np.uint8) / 255.).astype(np.float32)
    assert scale_table().dtype == np.float32 and np.array_equal(scale_table(), want)
    assert np.array_equal(PianoFramePlan(36, 64).lut, want)


def test_clips_of_both_passes_are_exercised_by_the_edge_frames():
    """What the fixture's generator asserts for its two large cases, at a size that is quick here."""
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_edge_frames
    fr = synthetic_edge_frames(8, 360, 640, 101)
    assert set(np.unique(fr)) == {0, 255}
    assert any(len({tuple(p) for p in f.reshape(-1, 3)[::97]} - {(0, 0, 0), (255, 255, 255)}) > 0 for f in fr), "no saturated-colour frame"
    hs, vs = PianoFramePlan(360, 640).integer_passes(fr)
    assert hs.min() < 0 and hs.max() > 255 and vs.min() < 0 and vs.max() > 255, (hs.min(), hs.max(), vs.min(), vs.max())


def test_plan_refuses_other_shapes():
    from v2a_amd.piano_frames import PianoFramePlan
    plan = PianoFramePlan(36, 64)
    with pytest.raises(ValueError):
        plan.preprocess_numpy(np.zeros((1, 36, 65, 3), np.uint8))
    with pytest.raises(ValueError):
        plan.preprocess_numpy(np.zeros((1, 36, 64, 3), np.float32))


# ---- frame selection, batching and the cache (features.py) --------------------------------------------------------------------
class _Stub:
    """A preprocess= that counts calls and frames: frame f of a clip becomes a constant image of value f + 1 (taken from the
    frame's first byte, so that it does not depend on the order of `select`)."""

    def __init__(self, hw=(4, 6)):
        self.calls, self.frames, self.hw = 0, 0, hw

    def __call__(self, frames, select=None):
        fr = np.asarray(frames)
        sel = list(range(fr.shape[0])) if select is None else list(select)
        self.calls += 1
        self.frames += len(sel)
        vals = torch.tensor([float(fr[j, 0, 0, 0]) + 1 for j in sel])
        return vals[:, None, None].expand(len(sel), *self.hw).contiguous()


def _clip(F, hw=(8, 12)):
    fr = np.zeros((F,) + hw + (3,), np.uint8)
    fr[:, 0, 0, 0] = np.arange(F)
    return fr


def _restate(F, duration, l, start=0, mx=None):
    """x3:1903-1913 in plain words."""
    if mx is None:
        mx = int(duration * 24000)
    out = []
    for i in range(start, mx + 960, 960):
        out.append(min(round(i / 24000 / (duration / F)), F - 1))
        if len(out) >= math.floor(l / 3.0) + 1:
            break
    return out


def test_piano_frames_from_video_resizes_distinct_frames_once():
    import v2a_amd
    # 12 fps: every video frame serves about two latent triples
    stub = _Stub()
    idx = _restate(24, 2.0, 150)
    got = v2a_amd.piano_frames_from_video(_clip(24), 2.0, 150, stub)
    assert len(set(idx)) < len(idx) and stub.calls == 1 and stub.frames == len(set(idx))
    assert got.shape == (len(idx), 4, 6) and torch.equal(got[:, 0, 0], torch.tensor([j + 1.0 for j in idx]))
    # 30 fps: no frame repeats, a window through start_sample / max_sample
    stub = _Stub()
    idx = _restate(60, 2.0, 30, 4800, 30000)
    got = v2a_amd.piano_frames_from_video(torch.from_numpy(_clip(60)), 2.0, 30, stub, start_sample=4800, max_sample=30000)
    assert len(set(idx)) == len(idx) == stub.frames and torch.equal(got[:, 0, 0], torch.tensor([j + 1.0 for j in idx]))


def test_load_piano_frames_with_video_frames(tmp_path):
    import v2a_amd
    vids = [str(tmp_path / f"v{i}.mp4") for i in range(3)]
    clips = [(_clip(48), 2.0), None, (_clip(30), 1.2)]
    l = 150
    stub = _Stub()
    got = v2a_amd.load_piano_frames([vids[0], None, (vids[2], 2400, 20000)], l, video_frames=clips, preprocess=stub, write_cache=False)
    i0, i2 = _restate(48, 2.0, l), _restate(30, 1.2, l, 2400, 20000)
    t = max(math.floor(l / 3) + 1, len(i0), len(i2))
    assert got.shape == (3, 1, t, 4, 6) and got.dtype == torch.float32
    want = torch.zeros(3, t)
    want[0, :len(i0)] = torch.tensor([j + 1.0 for j in i0])
    want[2, :len(i2)] = torch.tensor([j + 1.0 for j in i2])
    assert torch.equal(got[:, 0, :, 0, 0], want) and torch.equal(got[:, 0, :, 3, 5], want)
    assert float(got[1].abs().max()) == 0.0                                              # a None path: an all-zero clip
    assert stub.calls == 2 and stub.frames == len(set(i0)) + len(set(i2))                # only the frames in use
    assert not glob.glob(str(tmp_path / "*.npz"))                                       # write_cache=False writes nothing
    # write_cache (the default): every frame is resized and the cache has the reference's layout
    stub = _Stub()
    first = v2a_amd.load_piano_frames([vids[0], None, (vids[2], 2400, 20000)], l, video_frames=clips, preprocess=stub)
    assert torch.equal(first, got) and stub.calls == 2 and stub.frames == 48 + 30
    data = np.load(v2a_amd.piano_frames_cache_path(vids[0]))
    assert data["arr_0"].shape == (48, 4, 6, 1) and data["arr_0"].dtype == np.float32 and data["arr_1"].item() == 2.0
    assert np.array_equal(data["arr_0"][:, 0, 0, 0], np.arange(48) + 1.0)
    # read back: the same tensor, no preprocessing; an existing cache wins over frames
    stub = _Stub()
    assert torch.equal(v2a_amd.load_piano_frames([vids[0], None, (vids[2], 2400, 20000)], l), first)
    other = [(_clip(48) + 7, 2.0), None, (_clip(30) + 7, 1.2)]
    assert torch.equal(v2a_amd.load_piano_frames([vids[0], None, (vids[2], 2400, 20000)], l, video_frames=other, preprocess=stub), first)
    assert stub.calls == 0
    # nothing to read and nothing to preprocess: today's error; all None: None
    with pytest.raises(FileNotFoundError, match="moviepy"):
        v2a_amd.load_piano_frames([vids[1]], l, video_frames=[None], preprocess=stub)
    with pytest.raises(ValueError):
        v2a_amd.load_piano_frames([vids[1]], l, video_frames=[clips[0]])
    with pytest.raises(ValueError):
        v2a_amd.load_piano_frames([vids[1]], l, video_frames=clips, preprocess=stub)
    assert v2a_amd.load_piano_frames([None, None], l, video_frames=[None, None], preprocess=stub) is None


def test_load_piano_frames_with_real_tables(tmp_path):
    """The same wiring with preprocess_numpy behind it: the cache holds Pillow's frames as (F, 100, 900, 1)."""
    import v2a_amd
    from v2a_amd.synth import synthetic_video_frames
    fr = synthetic_video_frames(6, 36, 64, 5)
    plan = v2a_amd.PianoFramePlan(36, 64)

    def pre(frames, select=None):
        out = torch.from_numpy(plan.preprocess_numpy(np.asarray(frames)))
        return out if select is None else out[torch.tensor(list(select))]

    vp = str(tmp_path / "a.mp4")
    got = v2a_amd.load_piano_frames([vp], 12, video_frames=[(fr, 0.5)], preprocess=pre)
    idx = _restate(6, 0.5, 12)
    assert got.shape == (1, 1, max(5, len(idx)), 100, 900)
    assert torch.equal(got[0, 0, :len(idx)], torch.from_numpy(plan.preprocess_numpy(fr))[torch.tensor(idx)])
    data = np.load(v2a_amd.piano_frames_cache_path(vp))
    assert data["arr_0"].shape == (6, 100, 900, 1) and np.array_equal(data["arr_0"][..., 0], plan.preprocess_numpy(fr))


# ---- E2TTS and CLI wiring -----------------------------------------------------------------------------------------------------------
def _small_e2tts(**kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=128, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_encode_video_frames_return_convention(tmp_path):
    import inspect
    import v2a_amd
    m = _small_e2tts()
    assert m.encode_video_frames([str(tmp_path / "a.mp4")], 30, False) == (None, None)
    assert m.encode_video_frames([None, None], 30, True) == (None, None)
    assert m.encode_video_frames(None, 30, True) == (None, None)
    with pytest.raises(FileNotFoundError):
        m.encode_video_frames([str(tmp_path / "a.mp4")], 30, True)
    raw = np.random.default_rng(0).random((20, 100, 900, 1)).astype(np.float32)
    v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(str(tmp_path / "a.mp4")), raw, 1.0)
    frames, midis = m.encode_video_frames([str(tmp_path / "a.mp4"), None], 30, True)
    assert frames.shape == (2, 1, 11, 100, 900) and midis.shape == (2, 30, 51) and float(midis.abs().max()) == 0.0
    assert torch.equal(frames, v2a_amd.load_piano_frames([str(tmp_path / "a.mp4"), None], 30))
    sig = inspect.signature(v2a_amd.E2TTS.sample).parameters
    assert sig["piano"].default is False and sig["piano"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(v2a_amd.E2TTS.encode_video_frames).parameters["video_frames"].kind is inspect.Parameter.KEYWORD_ONLY


def test_cli_piano_frames_for(tmp_path):
    from v2a_amd import cli
    import v2a_amd
    vids = [str(tmp_path / "a.mp4"), str(tmp_path / "b.mp4")]
    v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(vids[0]), np.full((10, 4, 6, 1), 0.5, np.float32), 1.0)
    stub, seen = _Stub(), []

    def decode(vp):
        seen.append(vp)
        return _clip(12), 1.0

    got = cli.piano_frames_for(vids, 30, stub, decode)
    assert seen == [vids[1]] and stub.calls == 1 and stub.frames == 12 and got.shape[:2] == (2, 1)
    assert os.path.exists(v2a_amd.piano_frames_cache_path(vids[1]))
    assert torch.equal(cli.piano_frames_for(vids, 30, stub, decode), got) and seen == [vids[1]]          # both cached now

    def no_moviepy(vp):
        raise ImportError("No module named 'moviepy'")

    with pytest.raises(FileNotFoundError, match="no cached piano frames"):
        cli.piano_frames_for([str(tmp_path / "c.mp4")], 30, stub, no_moviepy)


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_piano_entries():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    _lib.build(verbose=False)
    for name in ("v2a_piano_resize_h", "v2a_piano_resize_v"):
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).restype is not None
    for name in ("PianoFramePlan", "PianoFramePreprocessor", "piano_frames_from_video"):
        import v2a_amd
        assert hasattr(v2a_amd, name)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    L = _lib.lib()
    # frames, F, H, W, sel, n, tmp, ldt, y0, rows, Wo, bounds, coef, ksize, stream
    assert L.v2a_piano_resize_h(None, 1, 8, 8, None, 1, None, 8, 0, 8, 8, None, None, 5, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_piano_resize_h(4096, 1, 8, 8, None, 1, 4096, 8, 4, 8, 8, 4096, 4096, 5, None) == -1 and b"rows" in L.v2a_last_error()
    assert L.v2a_piano_resize_h(4096, 1, 8, 8, None, 1, 4096, 10, 0, 8, 9, 4096, 4096, 5, None) == -1 and b"ldt" in L.v2a_last_error()
    assert L.v2a_piano_resize_h(4096, 1, 8, 8, None, 2, 4096, 8, 0, 8, 8, 4096, 4096, 5, None) == -1 and b"sel" in L.v2a_last_error()
    assert L.v2a_piano_resize_h(4097, 1, 8, 8, None, 1, 4096, 8, 0, 8, 8, 4096, 4096, 5, None) == -1 and b"aligned" in L.v2a_last_error()
    # tmp, n, rows, ldt, Ho, Wo, bounds, coef, ksize, lut, out, stream
    assert L.v2a_piano_resize_v(None, 1, 8, 8, 4, 8, None, None, 5, None, None, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_piano_resize_v(4096, 1, 8, 6, 4, 8, 4096, 4096, 5, 4096, 4096, None) == -1 and b"ldt" in L.v2a_last_error()
    assert L.v2a_piano_resize_v(4096, 1, 8, 8, 4, 8, 4096, 4096, 5, 4096, 4100, None) == -1 and b"aligned" in L.v2a_last_error()


def test_piano_device_assembly_has_no_scratch():
    """The rule of test_isa_guard.py (whose source list is fixed) for csrc/piano_frames.hip."""
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    paths = glob.glob(os.path.join(build, "piano_frames-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert paths, "no device assembly for piano_frames.hip: csrc/build.sh must compile it with -save-temps=obj"
    blocks = open(paths[0]).read().split("- .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert sum("piano_resize_" in n for n in names) == 2, names
    for b, n in zip(blocks, names):
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
