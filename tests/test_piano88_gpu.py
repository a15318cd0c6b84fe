"""GPU: the reference's 88-key piano configuration (e2_tts_crossatt3_2.py, `x3_2`) through `E2TTS(piano_keys=88)`.

Roll expansion by 5 / 2 (`v2a_roll_expand_ratio`): bit-equal to the torch expression of x3_2:1546-1554 evaluated on the CPU in fp32.
Portrait frame preprocessing (`v2a_piano_resize_vt`): bit-equal to Pillow's bytes (tests/golden/piano_frames_portrait.npz).
Video2Roll with 88 classes: against the reference module in float64 (tests/golden/video2roll_88.npz) at the bars that the header of
tests/test_video2roll_gpu.py and its tests state for the 51-key encoder -- fp32 and bf16x3: logits 2e-3 abs, probabilities 1e-4
abs; bf16: logits max 0.35 / mean 0.08, probabilities max 0.03 / mean 0.004.
DiT with notes = 88: against the CPU oracle at the bars of tests/test_sampler_gpu.py -- fp32 and bf16x3 1e-3, bf16 max 0.06 / mean 0.013.
Validation and MIDI: `forward(val=True)` equals `v2a_roll_metrics` by hand, `frames_to_midi` equals the 51-key engine on columns 15..65."""
import dataclasses
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import make_model
from oracle import e2_cfm_oracle as O
from oracle import video2roll_oracle as VO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
V2R_SEED, V2R_INPUT_SEED = 8801, 88          # scripts/make_golden_video2roll_88.py


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ---- roll expansion ------------------------------------------------------------------------------------------------------------------
def _expand_reference(x, l, notes):
    """x3_2:1546-1554 on the CPU in fp32, literally."""
    b, t = x.shape[:2]
    t5 = (t * 5 // 2) * 2
    x = x.reshape(b, t, 1, notes).repeat(1, 1, 5, 1).reshape(b, t * 5, notes)[:, :t5, :].reshape(b, t5 // 2, 2, notes).mean(2)
    b, d, _ = x.shape
    if d > l:
        x = x[:, :l, :]
    elif d < l:
        x = torch.cat((x, torch.zeros(b, l - d, notes, device=x.device)), 1)
    return x


def _roll(B, t, notes, seed):
    x = torch.rand(B, t, notes, generator=torch.Generator().manual_seed(seed))
    x[0, 0, 0], x[-1, -1, -1] = 0.0, 1.0
    return x


@pytest.mark.parametrize("notes", [88, 51])
@pytest.mark.parametrize("t", [1, 2, 7, 251])
def test_roll_expand_ratio_equals_the_reference_expression(L, notes, t):
    B, d = 2, 5 * t // 2
    x = _roll(B, t, notes, 100 * t + notes)
    xd = x.to(DEV)
    for l in (d - 3, d, d + 5):
        if l <= 0:                                   # t = 1: d - 3 = -1 frames is no output at all
            with pytest.raises(L.V2AError, match="v2a_roll_expand_ratio"):
                L.roll_expand_ratio(xd, torch.empty(B, 1, notes, device=DEV), B=B, t=t, notes=notes, rep=5, group=2, l=l)
            continue
        out = torch.full((B, l, notes), float("nan"), device=DEV)
        L.roll_expand_ratio(xd, out, B=B, t=t, notes=notes, rep=5, group=2, l=l)
        want = _expand_reference(x, l, notes)
        got = out.cpu()
        assert got.shape == want.shape == (B, l, notes)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (notes, t, l, float((got - want).abs().max()))
        if l > d:
            assert torch.all(got[:, d:] == 0)


@pytest.mark.parametrize("notes,t", [(88, 7), (51, 251), (51, 1)])
def test_roll_expand_ratio_group_1_is_roll_expand(L, notes, t):
    B = 2
    x = _roll(B, t, notes, t).to(DEV)
    for l in (3 * t - 2, 3 * t, 3 * t + 5):
        a, b = (torch.full((B, l, notes), float("nan"), device=DEV) for _ in range(2))
        L.roll_expand(x, a, B=B, t=t, notes=notes, rep=3, l=l)
        L.roll_expand_ratio(x, b, B=B, t=t, notes=notes, rep=3, group=1, l=l)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (notes, t, l)


def test_roll_expand_ratio_refuses_bad_arguments(L):
    x, out = torch.zeros(2, 4, 88, device=DEV), torch.zeros(2, 10, 88, device=DEV)
    ok = dict(B=2, t=4, notes=88, rep=5, group=2, l=10)
    L.roll_expand_ratio(x, out, **ok)
    for bad in (dict(group=3), dict(group=0), dict(rep=0), dict(t=0), dict(l=0), dict(notes=0), dict(B=0), dict(l=-1)):
        with pytest.raises(L.V2AError, match="v2a_roll_expand_ratio"):
            L.roll_expand_ratio(x, out, **{**ok, **bad})
    with pytest.raises(L.V2AError, match="null"):
        L.check(L.lib().v2a_roll_expand_ratio(None, out.data_ptr(), 2, 4, 88, 5, 2, 10, L.stream_ptr()))


# ---- portrait preprocessing ------------------------------------------------------------------------------------------------------------
def _fx():
    z = np.load(os.path.join(GOLD, "piano_frames_portrait.npz"))
    return z, json.loads(str(z["meta"]))


def _case_frames(case, z):
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    name, H, W, ns, ne, seed, _ = case
    fr = np.concatenate(([synthetic_video_frames(ns, H, W, seed)] if ns else []) + ([synthetic_edge_frames(ne, H, W, seed + 100)] if ne else []))
    md5 = [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr]
    assert md5 == list(z[name + "_frames_md5"]), f"{name}: the seeded frames differ from the ones the fixture was made from"
    return fr


def _check(got, z, name, frames):
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
def test_portrait_kernels_equal_pillow_bit_for_bit(ci):
    """Every fixture case: all frames in one launch pair, chunks of 1 and 4, and a `select` list that repeats and reorders."""
    from v2a_amd.piano_frames import PianoFramePreprocessor
    z, meta = _fx()
    case = meta["cases"][ci]
    name = case[0]
    fr = _case_frames(case, z)
    F = len(fr)
    pre = PianoFramePreprocessor(DEV, layout="portrait")
    whole = pre(fr)
    _check(whole, z, name, list(range(F)))
    frd = torch.from_numpy(fr).to(DEV)
    sel = [F - 1, 0, 1 % F, 0, F - 1]
    for chunk in (1, 4):
        assert torch.equal(pre(frd, chunk=chunk), whole), (name, chunk)
        for src in (fr, frd):
            _check(pre(src, select=sel, chunk=chunk), z, name, sel)
    assert pre(frd, select=[]).shape == (0, 100, 900)


def test_portrait_other_sizes_and_unaligned_heights():
    """Output shapes whose run length along y is no multiple of 4 or of the band (scalar stores, a short last band), a width that
    is no multiple of 4 (padded tmp rows), against the host restatement."""
    from v2a_amd.piano_frames import PianoFramePlan, PianoFramePreprocessor
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    for (H, W, Ho, Wo) in ((121, 203, 41, 37), (64, 97, 50, 333), (90, 70, 100, 30), (33, 45, 7, 64)):
        fr = np.concatenate([synthetic_video_frames(2, H, W, 3), synthetic_edge_frames(3, H, W, 4)])
        want = PianoFramePlan(H, W, Ho, Wo, layout="portrait").preprocess_numpy(fr)
        assert want.shape == (5, Ho, Wo)
        pre = PianoFramePreprocessor(DEV, Ho, Wo, chunk=2, layout="portrait")
        assert np.array_equal(pre(fr).cpu().numpy(), want), (H, W, Ho, Wo)
        assert np.array_equal(pre(fr, select=[4, 1, 1]).cpu().numpy(), want[[4, 1, 1]]), (H, W, Ho, Wo)


def test_piano_resize_vt_refuses_bad_arguments(L):
    lib, s = L.lib(), L.stream_ptr()
    tmp = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    tab = torch.zeros(64, dtype=torch.int32, device=DEV)
    lut, out = torch.zeros(256, device=DEV), torch.zeros(64, device=DEV)
    args = lambda **k: [k.get("tmp", tmp.data_ptr()), k.get("n", 1), 8, k.get("ldt", 8), 8, k.get("Wo", 8), tab.data_ptr(), tab.data_ptr(),
                        k.get("ksize", 4), lut.data_ptr(), k.get("out", out.data_ptr()), s]
    for bad in (dict(tmp=None), dict(n=0), dict(ldt=6), dict(Wo=9), dict(ksize=0), dict(out=out.data_ptr() + 4), dict(Wo=489, ldt=492)):
        with pytest.raises(L.V2AError, match="v2a_piano_resize_vt"):
            L.check(lib.v2a_piano_resize_vt(*args(**bad)))


# ---- Video2Roll, 88 classes ------------------------------------------------------------------------------------------------------------
V2R_BARS = {"fp32": dict(logit_max=2e-3, prob_max=1e-4), "bf16x3": dict(logit_max=2e-3, prob_max=1e-4),
            "bf16": dict(logit_max=0.35, logit_mean=0.08, prob_max=0.03, prob_mean=0.004)}


@pytest.fixture(scope="module")
def v2r88():
    from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames
    return dict(sd=random_video2roll_state_dict(V2R_SEED, 88), x=synthetic_piano_frames(1, 6, seed=V2R_INPUT_SEED),
                gold=np.load(os.path.join(GOLD, "video2roll_88.npz")))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_video2roll_88_against_the_reference_module(v2r88, mode):
    from v2a_amd.video2roll import Video2RollEngine
    g, x, bars = v2r88["gold"], v2r88["x"], V2R_BARS[mode]
    eng = Video2RollEngine(v2r88["sd"], DEV, compute=mode, expand=(5, 2))
    assert eng.notes == 88
    logits = eng.forward_windows(VO.frame_windows(x)).cpu().double().numpy()
    assert logits.shape == g["logits"].shape == (6, 88)
    le = np.abs(logits - g["logits"])
    probs = eng.frame_probs(x)
    pe = np.abs(probs.cpu().double().numpy() - g["probs"])
    print(f"video2roll 88 [{mode}]: logits max |d| = {le.max():.3e} mean {le.mean():.3e} (|logit| max {np.abs(g['logits']).max():.1f}); "
          f"probabilities max |d| = {pe.max():.3e} mean {pe.mean():.3e}")
    assert le.max() < bars["logit_max"] and le.mean() < bars.get("logit_mean", np.inf)
    assert probs.shape == (1, 6, 88) and pe.max() < bars["prob_max"] and pe.mean() < bars.get("prob_mean", np.inf)
    for l in (13, 15, 20):
        roll = eng.encode_frames(x, l)
        assert roll.shape == (1, l, 88) and roll.dtype == torch.float32 and roll.is_cuda
        re_ = np.abs(roll.cpu().double().numpy() - g[f"roll_l{l}"])
        print(f"  encode_frames l={l}: max |d| = {re_.max():.3e} mean {re_.mean():.3e}")
        assert re_.max() < bars["prob_max"] and re_.mean() < bars.get("prob_mean", np.inf)
        assert torch.equal(roll.cpu(), _expand_reference(probs.cpu(), l, 88))          # the expansion itself adds no difference
        if l > 15:
            assert torch.all(roll[:, 15:] == 0)


# ---- DiT with notes = 88 ------------------------------------------------------------------------------------------------------------------
SAMPLE_KW = dict(steps=4, cfg_strength=2.0, remove_parallel_component=False)
DIT_BARS = {"fp32": (1e-3, np.inf), "bf16x3": (1e-3, np.inf), "bf16": (0.06, 0.013)}          # (max, mean) of tests/test_sampler_gpu.py


@pytest.fixture(scope="module")
def dit88(small):
    cfg = dataclasses.replace(small["cfg"], notes=88)
    P = O.init_params(cfg, small["meta"]["param_seed"])
    assert P["proj_frames.weight"].shape == (cfg.dim_frames, 88)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=99, piano=True)
    assert roll.shape == (2, 40, 88)
    with torch.no_grad():
        ref = O.sample(P, cfg, y0, text, roll, ctx, cm, **SAMPLE_KW)
    return dict(cfg=cfg, P=P, y0=y0, text=text, roll=roll, ctx=ctx, cm=cm, ref=ref)


def _kw(d):
    return dict(y0=d["y0"], text_embed=d["text"], context=d["ctx"], context_mask=d["cm"], return_raw_output=True, **SAMPLE_KW)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_dit_with_88_notes_against_the_oracle(dit88, mode):
    d = dit88
    m = make_model(d["cfg"], d["P"], mode, piano_keys=88, device=DEV)
    assert m.cfg.notes == 88
    got = m.sample(torch.zeros(2, 40, 16), frames_embed=d["roll"], **_kw(d))
    err = (got - d["ref"]).abs()
    print(f"DiT notes=88 [{mode}]: 2 clips x 40 frames, 4 steps: max |delta| = {float(err.max()):.3e}, mean {float(err.mean()):.3e}")
    assert float(err.max()) < DIT_BARS[mode][0] and float(err.mean()) < DIT_BARS[mode][1]
    assert float((got - m.sample(torch.zeros(2, 40, 16), **_kw(d))).abs().max()) > 0          # the 88-key roll does condition the result


@pytest.fixture(scope="module")
def model88(dit88, v2r88):
    return make_model(dit88["cfg"], {**dit88["P"], **{"video2roll_net." + k: v for k, v in v2r88["sd"].items()}}, "fp32", piano_keys=88, device=DEV,
                      audiocond_drop_prob=1.1)          # the shipped configuration: no audio condition (predict.py:71-72)


def test_sample_frames_is_sample_of_encode_frames(dit88, model88):
    from v2a_amd.synth import synthetic_piano_frames
    m, d = model88, dit88
    x = synthetic_piano_frames(2, 17, seed=3)                            # floor(40 / 2.5) + 1 frames
    roll = m.encode_frames(x, 40)
    assert roll.shape == (2, 40, 88)
    assert torch.equal(roll.cpu(), _expand_reference(m._video2roll().frame_probs(x).cpu(), 40, 88))
    cond = torch.zeros(2, 40, 16)
    a = m.sample(cond, frames=x, **_kw(d))
    b = m.sample(cond, frames_embed=roll, **_kw(d))
    assert torch.equal(a, b)
    assert float((a - m.sample(cond, **_kw(d))).abs().max()) > 0


def test_sample_video_frames_piano_is_the_explicit_portrait_stack(dit88, model88, tmp_path):
    from v2a_amd.features import piano_frame_indices, piano_frames_cache_path
    from v2a_amd.piano_frames import PianoFramePlan
    from v2a_amd.synth import synthetic_edge_frames, synthetic_video_frames
    m, d, l = model88, dit88, 40
    # 30 frames over 1.0 s (30 fps: no frame repeats) and 9 frames over 0.9 s (10 fps: frames repeat); different sizes
    clips = [(np.concatenate([synthetic_video_frames(26, 72, 128, 1), synthetic_edge_frames(4, 72, 128, 2)]), 1.0),
             (synthetic_video_frames(9, 90, 160, 3), 0.9)]
    idx = [piano_frame_indices(len(f), dur, l, video_multi=2.5) for f, dur in clips]
    t = max(int(l // 2.5) + 1, max(map(len, idx)))
    assert t == 17
    stack = torch.zeros(2, 1, t, 100, 900)
    for b, ((f, _), ix) in enumerate(zip(clips, idx)):
        stack[b, 0, :len(ix)] = torch.from_numpy(PianoFramePlan(*f.shape[1:3], layout="portrait").preprocess_numpy(f))[torch.tensor(ix)]
    cond = torch.zeros(2, l, 16)
    ref = m.sample(cond, frames=stack, **_kw(d))
    got = m.sample(cond, video_frames=clips, piano=True, **_kw(d))
    assert torch.equal(got, ref)
    pre = m.piano_frame_preprocessor()
    assert pre.layout == "portrait" and pre.frames_done == sum(len(set(ix)) for ix in idx)
    frames, midis = m.encode_video_frames(None, l, True, video_frames=clips)
    assert frames.device.type == "cuda" and torch.equal(frames.cpu(), stack)
    assert midis.shape == (2, l, 88) and float(midis.abs().max()) == 0.0
    # with paths: the cache in the reference's layout, portrait content, honoured by the second call
    paths = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    first = m.sample(cond, video_paths=paths, video_frames=clips, piano=True, **_kw(d))
    assert torch.equal(first, ref)
    for p, (f, dur) in zip(paths, clips):
        data = np.load(piano_frames_cache_path(p))
        assert data["arr_0"].shape == (len(f), 100, 900, 1) and data["arr_0"].dtype == np.float32 and data["arr_1"].item() == dur
        assert np.array_equal(data["arr_0"][..., 0], PianoFramePlan(*f.shape[1:3], layout="portrait").preprocess_numpy(f))
    done = pre.frames_done
    fr2, _ = m.encode_video_frames(paths, l, True)
    assert pre.frames_done == done and torch.equal(fr2, stack)


# ---- validation and MIDI ------------------------------------------------------------------------------------------------------------------
def test_forward_val_with_88_key_midis(L, dit88, model88):
    from v2a_amd.synth import synthetic_piano_frames
    m, d, n = model88, dit88, 40
    g = torch.Generator().manual_seed(5)
    x = synthetic_piano_frames(2, 17, seed=7)
    midis = (torch.rand(2, 17, 88, generator=g) > 0.6).float().repeat_interleave(3, dim=1)[:, :n].contiguous()
    lens = torch.tensor([40, 31])
    x1, x0 = torch.randn(2, n, 16, generator=g), torch.randn(2, n, 16, generator=g)
    r = m.forward(x1, text=d["text"], times=torch.tensor([0.3, 0.7]), lens=lens, val=True, frames=x, midis=midis, x0=x0,
                  context=d["ctx"], context_mask=d["cm"])
    fe = m.encode_frames(x, n)
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    L.roll_metrics(fe, midis.to(DEV), O.lens_to_mask(lens, n).to(DEV, torch.uint8).contiguous(), out)
    s, cnt, tp, fp, fn, tn = out.cpu().tolist()
    assert cnt == 71 * 88 and tp + fp + fn + tn > 0 and min(tp, fp, fn, tn) > 0
    ratio = lambda num, den: num / den if den != 0 else 0.0
    want = [ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, tp + fp + fn)]
    got = [float(v) for v in r.loss_breakdown]
    print(f"forward(val=True), 88 keys: loss {float(r.loss):.6f}, roll loss {m.val_stats['roll']:.6f}, precision / recall / f1 / acc {got}")
    assert all(np.isfinite(got)) and bool(torch.isfinite(r.loss)) and bool(torch.isfinite(r.pred_flow).all())
    assert got == [float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in want]
    st = m.val_stats
    assert (st["tp"], st["fp"], st["fn"], st["tn"]) == (tp, fp, fn, tn) and st["roll"] == s / cnt
    assert float(r.loss) == float(torch.tensor(st["flow"] + 10.0 * st["roll"], dtype=torch.float64).to(torch.float32))
    with pytest.raises(ValueError, match="midis"):
        m.forward(x1, text=d["text"], times=0.5, val=True, frames=x, midis=midis[..., 15:66].contiguous(), x0=x0, context=d["ctx"],
                  context_mask=d["cm"])


def test_frames_to_midi_on_88_keys_is_the_51_key_engine_on_columns_15_to_65(model88, v2r88):
    from v2a_amd.roll2midi import Roll2MidiEngine
    from v2a_amd.synth import random_roll2midi_state_dict, synthetic_piano_frames
    from v2a_amd.video2roll import Video2RollEngine
    m = model88
    gsd = random_roll2midi_state_dict(3)
    x = synthetic_piano_frames(1, 7, seed=9)
    m.load_roll2midi({"state_dict_G": gsd})
    probs, midi = m.frames_to_midi(x)
    assert probs.shape == midi.shape == (1, 7, 51) and midi.dtype == torch.uint8
    fp = Video2RollEngine(v2r88["sd"], DEV, compute="fp32").frame_probs(x)
    assert fp.shape == (1, 7, 88)
    want_p, want_m = Roll2MidiEngine(gsd, DEV).refine(fp[..., 15:66].contiguous())
    assert torch.equal(probs, want_p) and torch.equal(midi, want_m)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_with_88_keys_end_to_end(tmp_path, v2r88):
    """`python -m v2a_amd.cli ... --piano --piano-keys 88` on cached CLIP / T5 / portrait-frame files and a checkpoint with
    `proj_frames (df, 88)` and `video2roll_net.fc (88, 128)`.  The CLI draws y0 from torch's global generator of the device, so the
    same seed in front of two runs gives them the same noise: with it two --piano runs are equal and the frames must change the
    latents against a run without --piano.  Without --piano the 88-key model samples on a zero roll of 88 keys."""
    import v2a_amd
    from v2a_amd import cli
    from v2a_amd.synth import random_state_dict, synthetic_piano_frames
    mc = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, dim_head=64, frames_heads=1, num_registers=4, max_seq_len=256,
              num_channels=16)
    cfg = v2a_amd.DiTConfig(notes=88, **mc)
    sd = random_state_dict(cfg, seed=3)
    assert sd["proj_frames.weight"].shape == (64, 88)
    ck = tmp_path / "v2p88.pt"
    torch.save({"model_state_dict": {**sd, **{"video2roll_net." + k: v for k, v in v2r88["sd"].items()}}}, ck)
    vids = [str(tmp_path / f"piano{i}.mp4") for i in range(2)]
    (tmp_path / "list.scp").write_text("".join(f"{v}\tpiano {i}\n" for i, v in enumerate(vids)))
    g = torch.Generator().manual_seed(8)
    for i, v in enumerate(vids):
        dur = 0.5 + 0.02 * i
        v2a_amd.save_clip_cache(v2a_amd.feature_cache_path(v), torch.randn(15 + i, cfg.dim_text, generator=g), dur)
        np.savez(v.replace(".mp4", ".t5.npz"), (0.2 * torch.randn(4, cfg.dim, generator=g)).numpy())
        v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(v), synthetic_piano_frames(1, 15 + i, seed=i)[0, 0][..., None], dur)
    common = ["--batch", "2", "--steps", "3", "--frames", "40", "--dtype", "fp32", "--bucket-frames", "0", "--bucket-ctx", "0",
              "--model-config", json.dumps(mc), "--piano-keys", "88"]

    def run(name, *flags):
        torch.manual_seed(4321)
        return [np.load(p) for p in cli.main([str(ck), "0", str(tmp_path / "list.scp"), "0", "2", str(tmp_path / name), *common, *flags])]

    piano, again, plain = run("a", "--piano"), run("b", "--piano"), run("c")
    assert len(piano) == 2 and all(p.shape == (40, 16) and np.isfinite(p).all() for p in piano + plain)
    assert all(np.array_equal(a, b) for a, b in zip(piano, again))                       # the same seed: the same run
    d = max(float(np.abs(a - b).max()) for a, b in zip(piano, plain))
    print(f"cli --piano-keys 88: max |latent with --piano - without| = {d:.3e}")
    assert d > 1e-3                                                                       # the 88-key roll conditions the sample
    # the frames the CLI selected: one per 2.5 latent frames of the longest clip of the batch
    from v2a_amd.features import load_piano_frames
    n = [int((0.5 + 0.02 * i) * 24000) // 320 for i in range(2)]
    stack = load_piano_frames(vids, max(n), video_multi=2.5)
    assert stack.shape[2] == int(max(n) // 2.5) + 1
    roll = v2a_amd.Video2RollEngine(v2r88["sd"], DEV, compute="fp32", expand=(5, 2)).encode_frames(stack, max(n))
    assert roll.shape == (2, max(n), 88) and float(roll.abs().max()) > 0
