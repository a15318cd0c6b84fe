"""CPU: the host half of the reference's 88-key piano configuration (e2_tts_crossatt3_2.py, `x3_2`): the two `PianoConfig`
records, frame selection at 2.5 latent frames per video frame, the 88-key MIDI ground truth, state-dict shapes, `piano_keys`
refusals, the CLI flag, the portrait restatement of the frame preprocessing against Pillow and tests/golden/piano_frames_portrait.npz
(scripts/make_golden_piano_frames_portrait.py), and the two new exports of the header."""
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "piano_frames_portrait.npz")
SIZES = [(360, 640), (640, 360), (97, 131), (40, 50), (1080, 1920), (1000, 80)]          # the sizes the issue sets
SMALL = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256)


def _model(**kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True, **SMALL),
                         num_channels=16, if_cond_proj_in=False, device="cpu", **kw)


# ---- the configurations ------------------------------------------------------------------------------------------------------------
def test_piano_51_reproduces_todays_constants():
    import v2a_amd
    from v2a_amd import features, video2roll
    p = features.PIANO_51
    assert tuple(p) == (51, 15, 65, 3.0, (3, 1), "landscape")
    assert tuple(features.PIANO_88) == (88, 0, 87, 2.5, (5, 2), "portrait")
    assert p.notes == v2a_amd.NOTES == video2roll.NOTES == v2a_amd.DiTConfig().notes == p.note_max - p.note_min + 1
    assert (features.NOTE_MIN, features.NOTE_MAX) == (p.note_min, p.note_max)
    assert features.PIANO_88.notes == features.PIANO_88.note_max - features.PIANO_88.note_min + 1
    assert features.piano_config(51) is p and features.piano_config(88) is features.PIANO_88 and features.piano_config(p) is p
    with pytest.raises(AttributeError):
        p.notes = 88                                                   # immutable
    # the defaults every caller had before are the 51-key values
    import inspect
    assert inspect.signature(features.piano_frame_indices).parameters["video_multi"].default == p.video_multi
    assert inspect.signature(features.load_piano_frames).parameters["video_multi"].default == p.video_multi
    assert inspect.signature(video2roll.Video2RollEngine.__init__).parameters["expand"].default == p.expand


def _reference_loop(n_frames, duration, l, start_sample=0, max_sample=None, video_multi=2.5):
    """x3_2:1926-1940, literally: the indices j of the frames the loop appends."""
    if max_sample is None:
        max_sample = int(duration * 24000)
    out = []
    frame_size_video = int(video_multi * 320)
    for i in range(start_sample, max_sample + frame_size_video, frame_size_video):
        j = min(round(i / 24000 / (duration / (n_frames - 0))), n_frames - 1)
        out.append(j)
        if len(out) >= math.floor(l / video_multi) + 1:
            break
    return out


@pytest.mark.parametrize("duration,n_frames", [(1.0, 30), (9.97, 299), (10.0, 300)])
@pytest.mark.parametrize("span", [None, (24000 // 4, 24000 * 3 // 4), (0, 100000), (4800, 240000)])
def test_frame_selection_at_2p5_equals_the_reference_loop(duration, n_frames, span):
    """`piano_frame_indices` took `video_multi` before the 88-key configuration existed, so this one pins behaviour that the
    configuration relies on rather than behaviour it adds."""
    from v2a_amd.features import piano_frame_indices
    for l in (75, 750, 748, 40):
        args = () if span is None else span
        got = piano_frame_indices(n_frames, duration, l, *args, video_multi=2.5)
        assert got == _reference_loop(n_frames, duration, l, *args), (duration, n_frames, span, l)
        assert len(got) <= math.floor(l / 2.5) + 1
    if span is None:
        assert int(2.5 * 320) == 800
        full = piano_frame_indices(n_frames, duration, 750, video_multi=2.5)
        assert len(full) == min(301, -(-int(duration * 24000) // 800) + 1)          # floor(l / 2.5) + 1 = 301, or the clip's end
        if n_frames == 300:
            assert full[:300] == list(range(300))                          # 30 fps: every frame once, none repeated


def test_load_piano_frames_pads_to_the_configurations_length(tmp_path):
    import v2a_amd
    vp = str(tmp_path / "p.mp4")
    raw = torch.rand(30, 100, 900, 1, generator=torch.Generator().manual_seed(1))
    v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(vp), raw, 1.0)
    for vm, t in ((3.0, 51), (2.5, 61)):
        fr = v2a_amd.load_piano_frames([vp, (vp, 2400, 12000)], 150, video_multi=vm)
        assert fr.shape == (2, 1, t, 100, 900)                          # floor(150 / video_multi) + 1
        i0 = v2a_amd.piano_frame_indices(30, 1.0, 150, video_multi=vm)
        i1 = v2a_amd.piano_frame_indices(30, 1.0, 150, 2400, 12000, video_multi=vm)
        assert torch.equal(fr[0, 0, :len(i0)], raw[i0, :, :, 0]) and torch.all(fr[0, 0, len(i0):] == 0)
        assert torch.equal(fr[1, 0, :len(i1)], raw[i1, :, :, 0]) and torch.all(fr[1, 0, len(i1):] == 0)


def test_midi_ground_truth_with_88_keys(tmp_path):
    from v2a_amd.features import PIANO_88, load_midi_ground_truth, midi_ground_truth_path
    rs = np.random.RandomState(3)
    vps = [str(tmp_path / f"m{i}.mp4") for i in range(2)]
    gts = [(rs.rand(n, 88) > 0.9).astype(np.uint8) for n in (12, 30)]
    for vp, gt in zip(vps, gts):
        np.save(midi_ground_truth_path(vp), gt)
    got = load_midi_ground_truth([vps[0], None, (vps[1], 0, 100)], 20, 88)
    assert got.shape == (2, 20, 88) and got.dtype == torch.float32
    assert np.array_equal(got[0, :12].numpy(), gts[0]) and float(got[0, 12:].abs().max()) == 0          # zero padded
    assert np.array_equal(got[1].numpy(), gts[1][:20])                                                   # cut
    assert torch.equal(load_midi_ground_truth(vps, 20, PIANO_88), load_midi_ground_truth(vps, 20, 88))
    old = load_midi_ground_truth(vps, 20)
    assert old.shape == (2, 20, 51) and torch.equal(old, load_midi_ground_truth(vps, 20, 88)[:, :, 15:66])
    with pytest.raises(ValueError, match="piano_keys"):
        load_midi_ground_truth(vps, 20, 52)


# ---- E2TTS -------------------------------------------------------------------------------------------------------------------------
def test_state_dict_shapes_and_refusals():
    import v2a_amd
    from v2a_amd import features
    from v2a_amd.synth import random_video2roll_state_dict
    from v2a_amd.video2roll import expected_state_dict_shapes as v2r_shapes
    m51, m88 = _model(), _model(piano_keys=88)
    assert m51.piano is features.PIANO_51 and m51.cfg.notes == 51 and m88.piano is features.PIANO_88 and m88.cfg.notes == 88
    s51, s88 = v2a_amd.expected_state_dict_shapes(m51.cfg), v2a_amd.expected_state_dict_shapes(m88.cfg)
    assert s88["proj_frames.weight"] == (64, 88) and s51["proj_frames.weight"] == (64, 51)
    assert {k for k in s51 if s51[k] != s88[k]} == {"proj_frames.weight"} and set(s51) == set(s88)
    v51, v88 = v2r_shapes(), v2r_shapes(88)
    assert v88["fc.weight"] == (88, 128) and v88["fc.bias"] == (88,)
    assert {k for k in v51 if v51[k] != v88[k]} == {"fc.weight", "fc.bias"}
    # seeded weights: the default draw is unchanged by the new argument, and the 88-class draw shares everything in front of fc.*
    a, b, c = random_video2roll_state_dict(7), random_video2roll_state_dict(7, 51), random_video2roll_state_dict(7, 88)
    assert list(a) == list(b) == list(c) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(a[k], c[k]) for k in a if not k.startswith("fc."))
    assert c["fc.weight"].shape == (88, 128) and torch.equal(c["fc.weight"][:51], a["fc.weight"])       # the same stream, drawn further
    for bad in (52, 0, "88", None, True, 88.5):
        with pytest.raises(ValueError, match="piano_keys"):
            _model(piano_keys=bad)
    with pytest.raises(ValueError, match="notes"):
        v2a_amd.E2TTS(transformer=dict(if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True, notes=51, **SMALL),
                      num_channels=16, device="cpu", piano_keys=88)
    # a checkpoint of the other configuration is refused when it is loaded
    with pytest.raises(RuntimeError, match="fc.weight"):
        m88.load_state_dict({"video2roll_net." + k: v for k, v in a.items()}, strict=False)
    with pytest.raises(RuntimeError, match="fc.weight"):
        m51.load_state_dict({"video2roll_net." + k: v for k, v in c.items()}, strict=False)
    m88.load_state_dict({"video2roll_net." + k: v for k, v in c.items()}, strict=False)
    g = torch.Generator().manual_seed(0)
    with pytest.raises(RuntimeError, match="proj_frames.weight"):
        m88.load_state_dict({"proj_frames.weight": torch.randn(64, 51, generator=g)}, strict=False)


def test_collate_clips_takes_the_note_count():
    """The CLI hands `extras` to `sample()`: the zero roll (and a clip's own roll) must have the model's keys."""
    import v2a_amd
    reqs = [v2a_amd.ClipRequest(f"v{i}.mp4", "p", 10 + i, torch.zeros(10 + i, 192), torch.zeros(3, 128)) for i in range(2)]
    assert v2a_amd.collate_clips(reqs, 16)[1]["frames_embed"].shape == (2, 11, 51)
    batch8, extras = v2a_amd.collate_clips(reqs, 16, notes=88)
    assert extras["frames_embed"].shape == (2, 11, 88) and batch8[7] is None
    reqs[1].roll = torch.ones(11, 88)
    batch8, extras = v2a_amd.collate_clips(reqs, 16, notes=88)
    assert batch8[7].shape == (2, 11, 88) and float(extras["frames_embed"][1].min()) == 1.0 and float(extras["frames_embed"][0].max()) == 0.0
    with pytest.raises(AssertionError, match="keys"):
        v2a_amd.collate_clips(reqs, 16)


def test_synthetic_conditioning_follows_the_configuration():
    from v2a_amd.synth import synthetic_conditioning
    m = _model(piano_keys=88)
    roll = synthetic_conditioning(m.cfg, 2, n=40, nc=4, seed=1, piano=True)[2]
    assert roll.shape == (2, 40, 88) and 0 < float((roll > 0).float().mean()) < 0.2


def test_encode_video_frames_reads_caches_at_the_configurations_rate(tmp_path):
    """No frames to preprocess, so no GPU: the stack of a cached clip is the loop's selection at 2.5, and midis follow notes."""
    import v2a_amd
    vp = str(tmp_path / "c.mp4")
    raw = torch.rand(30, 100, 900, 1, generator=torch.Generator().manual_seed(2))
    v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(vp), raw, 1.0)
    for keys, t in ((51, 26), (88, 31)):
        m = _model(piano_keys=keys)
        frames, midis = m.encode_video_frames([vp], 75, True)
        assert frames.shape == (1, 1, t, 100, 900) and midis.shape == (1, 75, keys)
        idx = v2a_amd.piano_frame_indices(30, 1.0, 75, video_multi=m.piano.video_multi)
        assert torch.equal(frames[0, 0, :len(idx)], raw[idx, :, :, 0])


def test_cli_flag():
    from v2a_amd import cli
    ap = cli.build_parser()
    base = ["ckpt.pt", "0", "test.scp", "0", "1", "out"]
    assert ap.parse_args(base).piano_keys == 51
    assert ap.parse_args(base + ["--piano-keys", "88"]).piano_keys == 88
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--piano-keys", "61"])
    helptext = ap.format_help()
    assert "--piano-keys" in helptext and "generated_frames_raw.2.npz" in helptext and "--piano-keys" in cli.__doc__
    import inspect
    assert inspect.signature(cli.piano_frames_for).parameters["video_multi"].default == 3.0


# ---- portrait preprocessing ----------------------------------------------------------------------------------------------------------
def _fx():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _case_frames(case):
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    _, H, W, ns, ne, seed, _ = case
    return np.concatenate(([synthetic_video_frames(ns, H, W, seed)] if ns else []) + ([synthetic_edge_frames(ne, H, W, seed + 100)] if ne else []))


def _md5s(a):
    return [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in a]


def _pillow_portrait(frames):
    """The four calls of `transform` (x3_2:65-68) behind the grey conversion of x3_2:1901-1903, on Pillow itself."""
    from PIL import Image
    out = []
    for f in frames:
        x = Image.fromarray(np.array(Image.fromarray(f).convert("L")).astype(np.uint8))
        x = x.resize((100, 900))
        x = np.reshape(x, (900, 100, 1))
        x = np.transpose(x, [2, 1, 0])
        x = x / 255.
        out.append(x)
    return np.concatenate(out).astype(np.float32)


def test_portrait_fixture_covers_the_sizes():
    _, meta = _fx()
    assert [(c[1], c[2], c[3] + c[4]) for c in meta["cases"]] == [(360, 640, 2), (640, 360, 1), (97, 131, 1), (40, 50, 1), (1080, 1920, 1),
                                                                 (1000, 80, 1), (360, 640, 1)]
    assert meta["cases"][-1][4] == 1 and meta["cases"][-1][6]            # the hard-edged frame, overshoot asserted by the script


@pytest.mark.parametrize("ci", range(7))
def test_portrait_numpy_equals_fixture(ci):
    from v2a_amd.piano_frames import PianoFramePlan
    z, meta = _fx()
    case = meta["cases"][ci]
    name, H, W = case[:3]
    fr = _case_frames(case)
    assert _md5s(fr) == list(z[name + "_frames_md5"]), f"{name}: the seeded frames differ from the ones the fixture was made from"
    plan = PianoFramePlan(H, W, layout="portrait")
    got = plan.preprocess_numpy(fr)
    assert got.dtype == np.float32 and got.shape == (len(fr), 100, 900) and got.flags["C_CONTIGUOUS"]
    assert (plan.Ho, plan.Wo, plan.out_hw) == (900, 100, (100, 900))
    samp = got.reshape(len(fr), -1)[:, z[name + "_idx"]]
    assert np.array_equal(samp, z[name + "_vals"]), (name, int((samp != z[name + "_vals"]).sum()))
    assert _md5s(got) == list(z[name + "_out_md5"]), name
    if case[6]:                                                         # both clips act in both passes
        hs, vs = plan.integer_passes(fr)
        assert hs.min() < 0 and hs.max() > 255 and vs.min() < 0 and vs.max() > 255


@pytest.mark.parametrize("hw", SIZES)
def test_portrait_numpy_equals_live_pillow(hw):
    import PIL  # noqa: F401  (the fixture script needs it too; a missing Pillow is a failure here, not a skip)
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    H, W = hw
    fr = np.concatenate([synthetic_video_frames(1, H, W, 21), synthetic_edge_frames(1, H, W, 22)])
    got = PianoFramePlan(H, W, layout="portrait").preprocess_numpy(fr)
    assert np.array_equal(got, _pillow_portrait(fr)), hw
    # and it is not the landscape result transposed in some other way: out[f, i, j] = resized[j, i]
    land = PianoFramePlan(H, W, 900, 100).preprocess_numpy(fr)           # the 900 x 100 image itself
    assert np.array_equal(got, land.transpose(0, 2, 1))


def test_layout_is_checked():
    from v2a_amd.piano_frames import PianoFramePlan
    with pytest.raises(ValueError, match="layout"):
        PianoFramePlan(64, 64, layout="sideways")
    assert PianoFramePlan(64, 64).layout == "landscape"


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_exports():
    from v2a_amd import _lib
    text = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int v2a_roll_expand_ratio(const float* roll, float* out, int32_t B, int32_t t, int32_t notes, int32_t rep, int32_t group, "
            "int32_t l, v2a_stream_t stream);") in flat
    assert ("int v2a_piano_resize_vt(const uint8_t* tmp, int32_t n, int32_t rows, int32_t ldt, int32_t Ho, int32_t Wo, const int32_t* bounds, "
            "const int32_t* coef, int32_t ksize, const float* lut, float* out, v2a_stream_t stream);") in flat
    for name in ("v2a_roll_expand_ratio", "v2a_piano_resize_vt"):
        assert name in _lib.EXPORTS
        doc = text[:text.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "x3_2" in doc, f"{name}: the declaration cites the lines of e2_tts_crossatt3_2.py it replaces"
    assert "int v2a_roll_expand(const float* roll, float* out, int32_t B, int32_t t, int32_t notes, int32_t rep, int32_t l, v2a_stream_t stream);" in flat
    assert _lib.ABI_VERSION == 9                                        # additive change
