"""GPU: the Roll2Midi generator (roll2midi.py, csrc/roll2midi.hip) against the REFERENCE module's float64 run.

Weights random_roll2midi_state_dict(4321), inputs synthetic_key_roll, expected values tests/golden/roll2midi.npz (written by
scripts/make_golden_roll2midi.py from src/audeo/Roll2MidiNet.py of the reference in float64).  Bars:
  * the three kernels against float64 torch: stem and head within 1e-5 of the output's magnitude (the project's kernel bar),
    v2a_leaky_shadow bit-equal to torch's fp32 leaky_relu, shadows bit-equal to `split_planes` / `.to(bfloat16)`, border zero;
  * forward, fp32 and bf16x3: probabilities within 1e-4 absolute (the bar Video2Roll's probabilities carry), taps d1..d6, u1..u5
    within 1e-4 rel / abs; logits: fp32 within 8x the reference's own fp32-vs-float64 deviation stored in the fixture (a different
    summation order over K up to 13 824), bf16x3 within 2e-3 absolute (Video2Roll's logit bar);
  * bf16: probabilities within 1e-2, Video2Roll's figure for that mode;
  * midi == (fixture probability >= 0.5) wherever the fixture probability is more than 1e-4 from 0.5; at most 1 % of the cells may
    be that close.
Measured on an MI355X (profiles/roll2midi.txt): stem 1.4e-7 and head 3.0e-7 of scale; at 51x100 probabilities 1.2e-6 (fp32), 6.3e-6
(bf16x3), 3.6e-3 (bf16), logits 9.2e-6 (fp32, bar 7.3e-5) and 3.7e-5 (bf16x3), worst tap 0.06 of its bar, no thresholded cell wrong."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "roll2midi.npz")
PARAM_SEED, INPUT_SEED, REFINE_SEED = 4321, 77, 79
KEYS = 51
SHAPES = ((2, 7), (1, 50), (1, 100))
TAPS = [f"d{i}" for i in range(1, 7)] + [f"u{i}" for i in range(1, 6)]


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


@pytest.fixture(scope="module")
def params():
    from v2a_amd.synth import random_roll2midi_state_dict
    return random_roll2midi_state_dict(PARAM_SEED)


@pytest.fixture(scope="module")
def engines(params):
    """One engine per compute mode, made on first use and shared by the tests of this module."""
    from v2a_amd.roll2midi import Roll2MidiEngine
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = Roll2MidiEngine(params, DEV, compute=mode)
        return made[mode]
    return get


def forward_input(n, w):
    from v2a_amd.synth import synthetic_key_roll
    return synthetic_key_roll(n, w, KEYS, INPUT_SEED + w).transpose(1, 2)[:, None].contiguous()


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


# geometry of the kernel tests: (n, H, W, channels of the whole map, channel offset of the slice, border)
GEOMS = [(2, 51, 7, 192, 64, 1), (3, 5, 3, 136, 8, 1), (2, 51, 7, 64, 0, 0)]


def _bordered(n, H, W, pitch, b, dtype=torch.float32, planes=1):
    shp = ((planes,) if planes > 1 else ()) + (n, H + 2 * b, W + 2 * b, pitch)
    return torch.zeros(shp, device=DEV, dtype=dtype)


def _interior(t, b):
    return t if b == 0 else t[..., b:-b, b:-b, :]


def _check_shadow_and_border(L, f32, sh, mode, b, off, C):
    """The slice's shadow is the bf16 / hi | lo copy of its fp32 values bit for bit, and nothing outside the slice's interior was written."""
    got = _interior(f32, b)[..., off:off + C].cpu()
    if mode == L.SH_BF16:
        assert torch.equal(_interior(sh, b)[..., off:off + C].cpu(), got.to(torch.bfloat16))
    elif mode == L.SH_SPLIT:
        planes = L.split_planes(got.reshape(-1, C))
        assert torch.equal(_interior(sh[0], b)[..., off:off + C].cpu().reshape(-1, C), planes[:, :C])
        assert torch.equal(_interior(sh[1], b)[..., off:off + C].cpu().reshape(-1, C), planes[:, C:])
    for t in (f32,) + ((sh,) if sh is not None else ()):
        z = t.clone()
        _interior(z, b)[..., off:off + C] = 0
        assert not bool(z.any()), "written outside the slice's interior"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS)
def test_stem_kernel(L, geom, mode):
    n, H, W, pitch, off, b = geom
    co = 64
    x = torch.rand(n, H, W, generator=_g(1))
    w = torch.randn(co, 1, 3, 3, generator=_g(2)) * 0.5
    ref = F.leaky_relu(F.conv2d(x[:, None].double(), w.double(), padding=1), 0.2).permute(0, 2, 3, 1)       # NHWC
    f32 = _bordered(n, H, W, pitch, b)
    sh = None if mode == 0 else _bordered(n, H, W, pitch, b, torch.bfloat16, 2 if mode == 2 else 1)
    L.roll2midi_stem(x.to(DEV), w.reshape(co, 9).t().contiguous().to(DEV), f32.view(-1)[off:], None if sh is None else sh.view(-1)[off:],
                     n=n, H=H, W=W, co=co, shadow_mode=mode, lo_offset=f32.numel() if mode == 2 else 0, pitch=pitch, border=b)
    torch.cuda.synchronize()
    got = _interior(f32, b)[..., off:off + co].cpu().double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"stem {geom} mode {mode}: max |d| / max |ref| = {err:.2e}")
    assert err < 1e-5
    _check_shadow_and_border(L, f32, sh, mode, b, off, co)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS)
def test_leaky_shadow_kernel(L, geom, mode):
    n, H, W, pitch, off, b = geom
    C = 64 if pitch < 192 else 128
    x = torch.randn(n, H, W, C, generator=_g(3))
    x[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    f32 = _bordered(n, H, W, pitch, b)
    _interior(f32, b)[..., off:off + C] = x.to(DEV)
    sh = None if mode == 0 else _bordered(n, H, W, pitch, b, torch.bfloat16, 2 if mode == 2 else 1)
    L.leaky_shadow(f32.view(-1)[off:], None if sh is None else sh.view(-1)[off:], n=n, H=H, W=W, C_=C, shadow_mode=mode,
                   lo_offset=f32.numel() if mode == 2 else 0, pitch=pitch, border=b)
    torch.cuda.synchronize()
    got = _interior(f32, b)[..., off:off + C].cpu()
    assert torch.equal(got.view(torch.int32), F.leaky_relu(x, 0.2).view(torch.int32)), "not bit-equal to torch's fp32 leaky_relu"
    _check_shadow_and_border(L, f32, sh, mode, b, off, C)


@pytest.mark.parametrize("geom", GEOMS)
def test_head_kernel(L, geom):
    n, H, W, pitch, off, b = geom
    u = _bordered(n, H, W, pitch, b)
    d = _bordered(n, H, W, 128, b)
    uv, dv = torch.randn(n, H, W, 16, generator=_g(4)), torch.randn(n, H, W, 64, generator=_g(5))
    _interior(u, b)[..., off:off + 16] = uv.to(DEV)
    _interior(d, b)[..., 64:128] = dv.to(DEV)
    w = torch.randn(80, generator=_g(6)) * 0.5
    bias, thr = 0.3, 0.4
    ref = torch.cat([uv, dv], -1).double() @ w.double() + bias
    logits, probs = (torch.empty(n, H, W, device=DEV) for _ in range(2))
    midi = torch.empty(n, H, W, device=DEV, dtype=torch.uint8)
    L.roll2midi_head(u.view(-1)[off:], d.view(-1)[64:], w.to(DEV), u_pitch=pitch, nu=16, d_pitch=128, nd=64, bias=bias, threshold=thr,
                     n=n, H=H, W=W, border=b, logits=logits, probs=probs, midi=midi)
    torch.cuda.synchronize()
    err = float((logits.cpu().double() - ref).abs().max() / ref.abs().max())
    # the sigmoid of the kernel's own fp32 logit: expf within 2 ulp (2^-22 relative), one add and one division at 2^-24 each, of a
    # value <= 1: under 6 x 2^-24
    perr = float((probs.cpu().double() - torch.sigmoid(logits.cpu().double())).abs().max())
    print(f"head {geom}: logits max |d| / max |ref| = {err:.2e}, probabilities vs the sigmoid of its logits max |d| = {perr:.2e}")
    assert err < 1e-5 and perr < 8 * 2.0 ** -24
    assert torch.equal(midi.cpu(), (probs.cpu() >= thr).to(torch.uint8))
    assert 0 < int(midi.sum()) < midi.numel()
    # each output alone: the others are optional
    only = torch.empty(n, H, W, device=DEV, dtype=torch.uint8)
    L.roll2midi_head(u.view(-1)[off:], d.view(-1)[64:], w.to(DEV), u_pitch=pitch, nu=16, d_pitch=128, nd=64, bias=bias, threshold=thr,
                     n=n, H=H, W=W, border=b, midi=only)
    assert torch.equal(only, midi)


# ------------------------------------------------------------------------------------------------ the network
def _midi_rule(midi, ref_probs, what):
    """midi == (ref >= 0.5) wherever ref is more than 1e-4 from 0.5; at most 1 % of the cells may be excluded."""
    ref_probs = np.asarray(ref_probs)
    clear = np.abs(ref_probs - 0.5) > 1e-4
    excluded = 1.0 - clear.mean()
    wrong = int(((midi != (ref_probs >= 0.5)) & clear).sum())
    print(f"{what}: {wrong} wrong cells of {clear.sum()}, {excluded:.4%} excluded")
    assert excluded <= 0.01
    assert wrong == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_forward_matches_the_float64_reference(engines, gold, mode, shape):
    n, w = shape
    tag = f"{n}x{w}"
    eng = engines(mode)
    x = forward_input(n, w)
    taps = {}
    probs = eng.forward(x, taps=taps).cpu().double().numpy()
    logits = eng.forward(x, return_logits=True).cpu().double().numpy()
    assert probs.shape == (n, 1, KEYS, w)
    worst = {}
    for k in TAPS:
        t = torch.cat(taps[k]).cpu().double().numpy()
        assert tuple(t.shape) == tuple(gold[f"{k}_{tag}_shape"]), k
        ref = gold[f"{k}_{tag}_val"]
        got = t[tuple(gold[f"{k}_{tag}_idx"].T)]
        worst[k] = float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
        st = np.array([t.mean(), np.abs(t).mean(), t.max(), t.min()])
        assert np.allclose(st, gold[f"{k}_{tag}_stats"], rtol=1e-4, atol=1e-4), (k, st, gold[f"{k}_{tag}_stats"])
    perr = float(np.abs(probs - gold[f"probs_{tag}"]).max())
    lerr = float(np.abs(logits - gold[f"logits_{tag}"]).max())
    ref32 = float(np.abs(gold[f"logits32_{tag}"] - gold[f"logits_{tag}"]).max())
    lbar = 8.0 * ref32 if mode == "fp32" else 2e-3
    print(f"forward {mode} {tag}: probabilities {perr:.2e} (1e-4), logits {lerr:.2e} (bar {lbar:.2e}; reference fp32 {ref32:.2e}), "
          f"taps |d| / (1e-4 + 1e-4 |ref|): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert perr < 1e-4
    assert max(worst.values()) < 1.0, worst
    assert lerr < lbar
    _midi_rule((probs >= 0.5), gold[f"probs_{tag}"], f"forward {mode} {tag} thresholded")


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_bf16(engines, gold, shape):
    n, w = shape
    tag = f"{n}x{w}"
    probs = engines("bf16").forward(forward_input(n, w)).cpu().double().numpy()
    perr = float(np.abs(probs - gold[f"probs_{tag}"]).max())
    flips = int(((probs >= 0.5) != (gold[f"probs_{tag}"] >= 0.5)).sum())
    print(f"forward bf16 {tag}: probabilities {perr:.2e} (1e-2), {flips} of {probs.size} thresholded cells differ")
    assert perr < 1e-2


def _refine_input():
    from v2a_amd.synth import synthetic_key_roll
    return torch.sigmoid(synthetic_key_roll(1, 130, KEYS, REFINE_SEED, logits=True))          # Roll2Midi_inference.py:58


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_refine_pad_matches_the_literal_rerun(engines, gold, mode):
    probs, midi = engines(mode).refine(_refine_input(), window=100, threshold=0.5, tail="pad")
    assert probs.shape == midi.shape == (1, 130, KEYS) and midi.dtype == torch.uint8
    perr = float(np.abs(probs[0].cpu().double().numpy() - gold["refine_pad_probs"]).max())
    print(f"refine pad {mode}: probabilities {perr:.2e} (1e-4)")
    assert perr < 1e-4
    _midi_rule(midi[0].cpu().numpy().astype(bool), gold["refine_pad_probs"], f"refine pad {mode}")
    clear = np.abs(gold["refine_pad_probs"] - 0.5) > 1e-4
    assert np.array_equal(midi[0].cpu().numpy()[clear], gold["refine_pad_midi"][clear])
    assert torch.equal(midi, (probs >= 0.5).to(torch.uint8))


def test_refine_own_equals_forward_on_the_slices(engines):
    eng = engines("bf16x3")
    from v2a_amd.synth import synthetic_key_roll
    roll = synthetic_key_roll(2, 17, KEYS, 5)
    probs, midi = eng.refine(roll, window=7, threshold=0.3, tail="own")
    for s, e in ((0, 7), (7, 14), (14, 17)):
        want = eng.forward(roll[:, s:e].transpose(1, 2)[:, None])[:, 0].transpose(1, 2)
        assert torch.equal(probs[:, s:e], want), (s, e)
    assert torch.equal(midi, (probs >= 0.3).to(torch.uint8))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_chunk_independence(params, engines, mode):
    from v2a_amd.roll2midi import Roll2MidiEngine
    x = forward_input(3, 9)
    one = Roll2MidiEngine(params, DEV, compute=mode, chunk=1).forward(x, return_logits=True)
    three = Roll2MidiEngine(params, DEV, compute=mode, chunk=3).forward(x, return_logits=True)
    assert torch.equal(one, three)


def test_odd_geometry_runs(engines):
    """keys = 1 and w = 1: the net is fully convolutional."""
    for mode in ("fp32", "bf16x3"):
        y = engines(mode).forward(torch.full((2, 1, 1, 1), 0.25))
        assert y.shape == (2, 1, 1, 1) and bool(((y > 0) & (y < 1)).all())
    a, b = (engines(m).forward(torch.full((2, 1, 1, 1), 0.25), return_logits=True) for m in ("fp32", "bf16x3"))
    assert float((a - b).abs().max()) < 2e-3


@pytest.fixture(scope="module")
def piano_model(params):
    import v2a_amd
    from v2a_amd.synth import random_video2roll_state_dict
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                       if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=16, if_cond_proj_in=False, compute_dtype="bf16x3", frames_compute_dtype="bf16x3", device=DEV)
    m.load_state_dict({"video2roll_net." + k: v for k, v in random_video2roll_state_dict(PARAM_SEED).items()}, strict=False)
    return m


def test_frames_to_midi_is_refine_of_frame_probs(piano_model, params):
    from v2a_amd.roll2midi import Roll2MidiEngine
    from v2a_amd.synth import synthetic_piano_frames
    from v2a_amd.video2roll import Video2RollEngine
    m = piano_model
    x = synthetic_piano_frames(1, 7, seed=INPUT_SEED)
    with pytest.raises(NotImplementedError, match="load_roll2midi"):
        m.frames_to_midi(x)
    m.load_roll2midi({"state_dict_G": params})
    probs, midi = m.frames_to_midi(x)
    assert probs.shape == midi.shape == (1, 7, KEYS)
    fp = Video2RollEngine(m._v2r_sd, DEV, compute="bf16x3").frame_probs(x)
    want_p, want_m = Roll2MidiEngine(params, DEV).refine(fp)
    assert torch.equal(probs, want_p) and torch.equal(midi, want_m)


def test_frame_probs_repeated_is_encode_frames(params):
    from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames
    from v2a_amd.video2roll import Video2RollEngine
    eng = Video2RollEngine(random_video2roll_state_dict(PARAM_SEED), DEV, compute="bf16x3")
    x = synthetic_piano_frames(2, 4, seed=INPUT_SEED + 1)
    fp = eng.frame_probs(x)
    assert fp.shape == (2, 4, KEYS)
    for l in (10, 14):
        want = fp.repeat_interleave(3, 1)[:, :l]
        if l > 12:
            want = torch.cat([want, torch.zeros(2, l - 12, KEYS, device=want.device)], 1)
        assert torch.equal(eng.encode_frames(x, l), want)
