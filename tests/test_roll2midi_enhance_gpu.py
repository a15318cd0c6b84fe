"""GPU: the attention-gated Roll2Midi generator (roll2midi.py: Roll2MidiEnhanceEngine; csrc/roll2midi.hip: v2a_roll2midi_gate) against
the REFERENCE module's float64 run.

Weights random_roll2midi_enhance_state_dict(4321), inputs synthetic_key_roll, expected values tests/golden/roll2midi_enhance.npz
(written by scripts/make_golden_roll2midi_enhance.py from src/audeo/Roll2MidiNet_enhance.py of the reference in float64).  Bars:
  * the gate kernel alone: logits within 1e-5 of the float64 dot's magnitude (the project's kernel bar, the one head_kernel
    carries); alpha within 8 x 2^-24 of the float64 sigmoid of the kernel's own logit (the derivation in test_roll2midi_gpu.py's head
    test); the stored map bit-equal to torch's fp32 `x * alpha` with the kernel's alpha; shadows bit-equal to `.to(bfloat16)` /
    `split_planes` of the stored values; every element outside the segments' interiors keeps the sentinel it was filled with;
  * forward, fp32 and bf16x3: the plain net's bars -- probabilities 1e-4, taps d1..d6, u1..u5, a1..a4 within 1e-4 rel / abs, logits
    within 8x the reference's own fp32-vs-float64 deviation (fp32) or 2e-3 (bf16x3); bf16: probabilities 1e-2;
  * midi == (fixture probability >= 0.5) wherever the fixture probability is more than 1e-4 from 0.5; at most 1 % excluded.
Measured on an MI355X (profiles/roll2midi_enhance.txt): gate logits 7.9e-8 .. 1.3e-7 of scale (7.9e-8 at 1024 + 1024), alpha 3.3e-8 ..
7.5e-8; at 51x100 probabilities 2.4e-6 (fp32), 1.0e-5 (bf16x3), 4.0e-3 (bf16), logits 9.5e-6 (fp32, bar 3.2e-5) and 4.5e-5 (bf16x3),
worst tap 0.01 (fp32) / 0.06 (bf16x3) of its bar, no thresholded cell wrong.  Every bar holds as stated: none was replaced by the
fixture's fp32 deviation (the `_val32` samples; the forward test prints them beside the engine's for comparison).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "roll2midi_enhance.npz")
PARAM_SEED, INPUT_SEED, REFINE_SEED = 4321, 77, 79
KEYS = 51
SHAPES = ((2, 7), (1, 50), (1, 100))
TAPS = [f"d{i}" for i in range(1, 7)] + [f"u{i}" for i in range(1, 6)] + [f"a{i}" for i in range(1, 5)]
SENTINEL = 7.0


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
    from v2a_amd.synth import random_roll2midi_enhance_state_dict
    return random_roll2midi_enhance_state_dict(PARAM_SEED)


@pytest.fixture(scope="module")
def engines(params):
    """One engine per compute mode, made on first use and shared by the tests of this module."""
    from v2a_amd.roll2midi import Roll2MidiEnhanceEngine
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = Roll2MidiEnhanceEngine(params, DEV, compute=mode)
        return made[mode]
    return get


def forward_input(n, w):
    from v2a_amd.synth import synthetic_key_roll
    return synthetic_key_roll(n, w, KEYS, INPUT_SEED + w).transpose(1, 2)[:, None].contiguous()


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the gate kernel alone
# geometry of the kernel tests: (n, H, W, channels of the whole map, channel offset of the slice, border)
GEOMS = [(2, 51, 7, 192, 64, 1), (3, 5, 3, 136, 8, 1), (2, 51, 7, 64, 0, 0)]


def _interior(t, b):
    return t if b == 0 else t[..., b:-b, b:-b, :]


class _Seg:
    """C channels at channel offset off of a sentinel-filled (n, H + 2b, W + 2b, pitch) fp32 buffer of its own, with its shadow."""

    def __init__(self, x, pitch, off, b, mode):
        n, H, W, C = x.shape
        self.x, self.C, self.pitch, self.off, self.b, self.mode = x, C, pitch, off, b, mode
        shp = (n, H + 2 * b, W + 2 * b, pitch)
        self.f32 = torch.full(shp, SENTINEL, device=DEV)
        _interior(self.f32, b)[..., off:off + C] = x.to(DEV)
        self.sh = None if mode == 0 else torch.full(((2,) if mode == 2 else ()) + shp, SENTINEL, device=DEV, dtype=torch.bfloat16)
        self.lo = self.f32.numel() if mode == 2 else 0

    def arg(self):
        return (self.f32.view(-1)[self.off:], self.pitch, self.C, None if self.sh is None else self.sh.view(-1)[self.off:], self.lo)

    def check(self, L, alpha):
        got = _interior(self.f32, self.b)[..., self.off:self.off + self.C].cpu()
        want = self.x * alpha[..., None]                                  # torch's fp32 multiply of the stored x by the kernel's alpha
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the stored map is not bit-equal to fp32 x * alpha"
        C = self.C
        if self.mode == L.SH_BF16:
            assert torch.equal(_interior(self.sh, self.b)[..., self.off:self.off + C].cpu(), got.to(torch.bfloat16))
        elif self.mode == L.SH_SPLIT:
            planes = L.split_planes(got.reshape(-1, C))
            assert torch.equal(_interior(self.sh[0], self.b)[..., self.off:self.off + C].cpu().reshape(-1, C), planes[:, :C])
            assert torch.equal(_interior(self.sh[1], self.b)[..., self.off:self.off + C].cpu().reshape(-1, C), planes[:, C:])
        for t in (self.f32,) + ((self.sh,) if self.sh is not None else ()):
            z = t.clone()
            _interior(z, self.b)[..., self.off:self.off + C] = SENTINEL
            assert bool((z == SENTINEL).all()), "written outside the segment's interior"


def _run_gate(L, segs, n, H, W, b, mode, seed):
    """The gate over the concatenation of segs, weights ~ 1 / sqrt(C) so that z spreads over about +-2; checks every bar of the
    module docstring and returns (logit error, alpha error)."""
    C = sum(s.C for s in segs)
    w = torch.randn(C, generator=_g(seed)) / C ** 0.5
    bias = 0.3
    x = torch.cat([s.x for s in segs], -1)
    ref = x.double() @ w.double() + bias
    logits, alpha = (torch.full((n, H, W), SENTINEL, device=DEV) for _ in range(2))
    L.roll2midi_gate(segs[0].arg(), segs[1].arg() if len(segs) > 1 else None, w.to(DEV), bias=bias, shadow_mode=mode, n=n, H=H, W=W,
                     border=b, logits=logits, alpha=alpha)
    torch.cuda.synchronize()
    logits, alpha = logits.cpu(), alpha.cpu()
    err = float((logits.double() - ref).abs().max() / ref.abs().max())
    # the sigmoid of the kernel's own fp32 logit: expf within 2 ulp (2^-22 relative), one add and one division at 2^-24 each, of a
    # value <= 1: under 6 x 2^-24
    aerr = float((alpha.double() - torch.sigmoid(logits.double())).abs().max())
    assert err < 1e-5, err
    assert aerr < 8 * 2.0 ** -24, aerr
    assert float(ref.std()) > 0.5 and float(alpha.min()) < 0.4 and float(alpha.max()) > 0.6      # the inputs make the gate gate
    for s in segs:
        s.check(L, alpha)
    return err, aerr


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS)
def test_gate_kernel_one_segment(L, geom, mode):
    n, H, W, pitch, off, b = geom
    C = 64 if pitch < 192 else 128
    seg = _Seg(torch.randn(n, H, W, C, generator=_g(3)), pitch, off, b, mode)
    err, aerr = _run_gate(L, [seg], n, H, W, b, mode, 4)
    print(f"gate {geom} mode {mode}, one segment of {C}: logits max |d| / max |ref| = {err:.2e}, alpha vs the sigmoid of its logit {aerr:.2e}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS)
def test_gate_kernel_two_segments_in_two_buffers(L, geom, mode):
    """Segment 1 lives in another buffer with another pitch and offset (fp32 mode's p_k and d_(6-k)); its 40 channels are no multiple of 16."""
    n, H, W, pitch, off, b = geom
    C0 = 64 if pitch < 192 else 128
    s0 = _Seg(torch.randn(n, H, W, C0, generator=_g(5)), pitch, off, b, mode)
    s1 = _Seg(torch.randn(n, H, W, 40, generator=_g(6)), 56, 16, b, mode)
    err, aerr = _run_gate(L, [s0, s1], n, H, W, b, mode, 7)
    print(f"gate {geom} mode {mode}, segments {C0} + 40: logits max |d| / max |ref| = {err:.2e}, alpha vs the sigmoid of its logit {aerr:.2e}")


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("widths", [(1024, 1024), (512, 512), (520, 264)])
def test_gate_kernel_wide(L, widths, mode):
    """att1's real width (four 512-channel chunks per wave), att2's (two), and one whose second chunk is partial and holds the segment
    boundary; both segments in ONE bordered map, as the implicit-GEMM modes lay u_k out.  n*H*W = 15 pixels: the last block is partial."""
    n, H, W, b = 1, 5, 3, 1
    C0, C1 = widths
    x = torch.randn(n, H, W, C0 + C1, generator=_g(8))
    whole = _Seg(x, C0 + C1 + 8, 8, b, mode)
    s0, s1 = (_Seg.__new__(_Seg) for _ in range(2))
    for s, o, c in ((s0, 0, C0), (s1, C0, C1)):
        s.__dict__.update(whole.__dict__)
        s.x, s.C, s.off = x[..., o:o + c], c, 8 + o
    C = C0 + C1
    w = torch.randn(C, generator=_g(9)) / C ** 0.5
    ref = x.double() @ w.double() + 0.3
    logits, alpha = (torch.empty(n, H, W, device=DEV) for _ in range(2))
    L.roll2midi_gate(s0.arg(), s1.arg(), w.to(DEV), bias=0.3, shadow_mode=mode, n=n, H=H, W=W, border=b, logits=logits, alpha=alpha)
    torch.cuda.synchronize()
    logits, alpha = logits.cpu(), alpha.cpu()
    err = float((logits.double() - ref).abs().max() / ref.abs().max())
    aerr = float((alpha.double() - torch.sigmoid(logits.double())).abs().max())
    print(f"gate {C0} + {C1} mode {mode}: logits max |d| / max |ref| = {err:.2e}, alpha vs the sigmoid of its logit {aerr:.2e}")
    assert err < 1e-5 and aerr < 8 * 2.0 ** -24
    whole.x = x
    whole.check(L, alpha)                                                # the whole map: both segments, and the sentinel everywhere else
    # a pixel's bits do not depend on what else is in the launch, nor on where the segments part: the last pixel alone, as one segment
    one = _Seg(x[:, -1:, -1:].contiguous(), C, 0, 0, 0)
    z1 = torch.empty(1, 1, 1, device=DEV)
    L.roll2midi_gate(one.arg(), None, w.to(DEV), bias=0.3, shadow_mode=0, n=1, H=1, W=1, border=0, logits=z1)
    assert torch.equal(z1.cpu()[0, 0, 0], logits[0, -1, -1])


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
    worst, ref32 = {}, {}
    for k in TAPS:
        t = torch.cat(taps[k]).cpu().double().numpy()
        assert tuple(t.shape) == tuple(gold[f"{k}_{tag}_shape"]), k
        ref = gold[f"{k}_{tag}_val"]
        got = t[tuple(gold[f"{k}_{tag}_idx"].T)]
        worst[k] = float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
        ref32[k] = float((np.abs(gold[f"{k}_{tag}_val32"] - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
        st = np.array([t.mean(), np.abs(t).mean(), t.max(), t.min()])
        assert np.allclose(st, gold[f"{k}_{tag}_stats"], rtol=1e-4, atol=1e-4), (k, st, gold[f"{k}_{tag}_stats"])
    perr = float(np.abs(probs - gold[f"probs_{tag}"]).max())
    lerr = float(np.abs(logits - gold[f"logits_{tag}"]).max())
    l32 = float(np.abs(gold[f"logits32_{tag}"] - gold[f"logits_{tag}"]).max())
    lbar = 8.0 * l32 if mode == "fp32" else 2e-3
    print(f"forward {mode} {tag}: probabilities {perr:.2e} (1e-4), logits {lerr:.2e} (bar {lbar:.2e}; reference fp32 {l32:.2e}), "
          f"taps |d| / (1e-4 + 1e-4 |ref|): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    print(f"    the reference's own fp32 run on the same scale: " + ", ".join(f"{k} {v:.3f}" for k, v in ref32.items()))
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
def test_chunk_independence(params, mode):
    from v2a_amd.roll2midi import Roll2MidiEnhanceEngine
    x = forward_input(3, 9)
    one = Roll2MidiEnhanceEngine(params, DEV, compute=mode, chunk=1).forward(x, return_logits=True)
    three = Roll2MidiEnhanceEngine(params, DEV, compute=mode, chunk=3).forward(x, return_logits=True)
    assert torch.equal(one, three)


def test_odd_geometry_runs(engines):
    """keys = 1 and w = 1: the net is fully convolutional."""
    for mode in ("fp32", "bf16x3"):
        y = engines(mode).forward(torch.full((2, 1, 1, 1), 0.25))
        assert y.shape == (2, 1, 1, 1) and bool(((y > 0) & (y < 1)).all())
    a, b = (engines(m).forward(torch.full((2, 1, 1, 1), 0.25), return_logits=True) for m in ("fp32", "bf16x3"))
    assert float((a - b).abs().max()) < 2e-3


def test_frames_to_midi_is_refine_of_frame_probs(params):
    import v2a_amd
    from v2a_amd.roll2midi import Roll2MidiEnhanceEngine
    from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames
    from v2a_amd.video2roll import Video2RollEngine
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                       if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=16, if_cond_proj_in=False, compute_dtype="bf16x3", frames_compute_dtype="bf16x3", device=DEV)
    m.load_state_dict({"video2roll_net." + k: v for k, v in random_video2roll_state_dict(PARAM_SEED).items()}, strict=False)
    x = synthetic_piano_frames(1, 7, seed=INPUT_SEED)
    eng = m.load_roll2midi({"state_dict_G": params})
    assert type(eng) is Roll2MidiEnhanceEngine
    probs, midi = m.frames_to_midi(x)
    assert probs.shape == midi.shape == (1, 7, KEYS)
    fp = Video2RollEngine(m._v2r_sd, DEV, compute="bf16x3").frame_probs(x)
    want_p, want_m = Roll2MidiEnhanceEngine(params, DEV).refine(fp)
    assert torch.equal(probs, want_p) and torch.equal(midi, want_m)
