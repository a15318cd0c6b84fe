"""CPU: the host side of the Roll2Midi generator (roll2midi.py): ABI agreement of its three entry points, the state-dict layout,
the BatchNorm fold (eps = 0.8), the transposed-convolution weight transform, refine's window cutting, the refusal of the
attention-gate variant and the CLI wiring.  No GPU is touched.  The offset tables are conv2d.py's: test_conv2d_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "roll2midi.npz")
ENTRY_POINTS = ("v2a_roll2midi_stem", "v2a_leaky_shadow", "v2a_roll2midi_head")


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


@pytest.fixture(scope="module")
def params():
    from v2a_amd.synth import random_roll2midi_state_dict
    return random_roll2midi_state_dict(4321)


def test_header_ctypes_and_exports_agree(lib):
    src = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "v2a_stream_t": ctypes.c_void_p}
    L = lib.lib()
    for name in ENTRY_POINTS:
        assert name in lib.EXPORTS
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, re.S)
        assert proto, f"{name} is not declared in include/v2a_cfm.h"
        want = []
        for arg in proto.group(1).split(","):
            arg = arg.strip()
            want.append(ctypes.c_void_p if "*" in arg else ctype[arg.replace("const ", "").split()[0]])
        fn = getattr(L, name)
        assert fn.argtypes == want, (name, fn.argtypes, want)
        assert fn.restype is ctypes.c_int
    assert L.v2a_abi_version() == lib.ABI_VERSION == 9              # the entry points are additive


def test_entry_points_validate_on_cpu(lib):
    """Bad arguments are refused before any HIP call."""
    L = lib.lib()
    assert L.v2a_roll2midi_stem(16, 16, 1, 5, 3, 60, 16, None, 0, 0, 64, 1, None) == -1 and b"geometry" in L.v2a_last_error()
    assert L.v2a_roll2midi_stem(16, 16, 1, 5, 3, 64, 16, None, 0, 0, 60, 1, None) == -1 and b"pitch" in L.v2a_last_error()
    assert L.v2a_leaky_shadow(16, None, 1, 0, 1, 5, 3, 64, 64, 1, None) == -1 and b"shadow" in L.v2a_last_error()
    assert L.v2a_leaky_shadow(16, 32, 2, 64, 1, 5, 3, 64, 64, 1, None) == -1 and b"lo_offset" in L.v2a_last_error()
    assert L.v2a_leaky_shadow(16, 32, 1, 8, 1, 5, 3, 64, 64, 1, None) == -1 and b"lo_offset" in L.v2a_last_error()
    assert L.v2a_leaky_shadow(8, None, 0, 0, 1, 5, 3, 64, 64, 1, None) == -1 and b"misaligned" in L.v2a_last_error()
    assert L.v2a_roll2midi_head(16, 64, 16, 16, 64, 64, 16, 0.0, 0.5, 1, 5, 3, 1, None, None, None, None) == -1 and b"no output" in L.v2a_last_error()
    assert L.v2a_roll2midi_head(16, 8, 16, 16, 64, 64, 16, 0.0, 0.5, 1, 5, 3, 1, 16, None, None, None) == -1 and b"pitches" in L.v2a_last_error()
    assert L.v2a_roll2midi_head(16, 64, 16, None, 64, 64, 16, 0.0, 0.5, 1, 5, 3, 1, 16, None, None, None) == -1 and b"null" in L.v2a_last_error()


def test_expected_shapes_are_the_reference_modules_key_list(params):
    from v2a_amd.roll2midi import expected_state_dict_shapes
    g = np.load(GOLD, allow_pickle=False)
    want = {str(k): tuple(int(d) for d in str(s).split("x") if d) for k, s in zip(g["state_dict_keys"], g["state_dict_shapes"])}
    assert expected_state_dict_shapes() == want
    assert list(expected_state_dict_shapes()) and set(params) == set(want)
    assert all(tuple(params[k].shape) == shp for k, shp in want.items())


def test_bn_fold_uses_eps_0_8(params):
    from v2a_amd import roll2midi as R
    assert R.BN_EPS == 0.8
    for name in ("down2", "down6", "up1", "up5"):
        w, b = R.folded_conv(params, name)
        w0 = params[f"{name}.model.0.weight"].double()
        if name.startswith("up"):
            w0 = w0.permute(1, 0, 2, 3).flip(2, 3)
        bn = {k: params[f"{name}.model.1.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")}
        s = bn["weight"] / torch.sqrt(bn["running_var"] + 0.8)
        assert torch.allclose(w.double(), w0 * s[:, None, None, None], rtol=1e-6, atol=1e-9)
        assert torch.allclose(b.double(), bn["bias"] - bn["running_mean"] * s, rtol=1e-6, atol=1e-8)
        wrong = w0 * (bn["weight"] / torch.sqrt(bn["running_var"] + 1e-5))[:, None, None, None]
        assert not torch.allclose(w.double(), wrong, rtol=1e-2)          # the usual eps gives another network
    w, b = R.folded_conv(params, "down1")
    assert b is None and torch.equal(w, params["down1.model.0.weight"])


def test_transposed_conv_is_a_plain_conv_of_the_transformed_weight():
    from v2a_amd.conv2d import gemm_weight
    from v2a_amd.roll2midi import transposed_conv_weight
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 6, 5, 4, generator=g, dtype=torch.float64)
    w = torch.randn(6, 3, 3, 3, generator=g, dtype=torch.float64)              # ConvTranspose2d layout [ci][co][ky][kx]
    ref = F.conv_transpose2d(x, w, stride=1, padding=1)
    wc = transposed_conv_weight(w)
    assert wc.shape == (3, 6, 3, 3)
    assert torch.allclose(F.conv2d(x, wc, padding=1), ref, rtol=0, atol=1e-12)
    # the GEMM rows: K in (ky, kx, c) order over an NHWC patch; two segments = the patch matrices of the two concatenated maps
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1)                             # NHWC, zero border
    patch = torch.stack([xp[:, ky:ky + 5, kx:kx + 4] for ky in range(3) for kx in range(3)], 3)        # (n, H, W, tap, c)
    assert torch.allclose((patch.reshape(2, 5, 4, 54) @ gemm_weight(wc).t()).permute(0, 3, 1, 2), ref, atol=1e-12)
    two = torch.cat([patch[..., :2].reshape(2, 5, 4, 18), patch[..., 2:].reshape(2, 5, 4, 36)], -1)
    assert torch.allclose((two @ gemm_weight(wc, (2, 4)).t()).permute(0, 3, 1, 2), ref, atol=1e-12)
    assert gemm_weight(wc, None, 8).shape == (8, 54) and not bool(gemm_weight(wc, None, 8)[3:].any())


class _FakeRun:
    """Roll2MidiEngine.refine without a device: `_run` replaced by a function of the window's content and width."""

    def __init__(self):
        from v2a_amd.roll2midi import Roll2MidiEngine
        self.dev = torch.device("cpu")
        self.refine = Roll2MidiEngine.refine.__get__(self)
        self.calls = []

    @staticmethod
    def f(x):                                                      # (n, keys, w): depends on the position inside the window and on w
        w = x.shape[2]
        return (x * 0.5 + 0.25 * torch.arange(w)[None, None, :] / w).float()

    def _run(self, x, threshold, want_logits=False, want_midi=False, taps=None):
        self.calls.append(tuple(x.shape))
        p = self.f(x)
        return p, (p >= threshold).to(torch.uint8)


@pytest.mark.parametrize("t", [100, 130, 250])
@pytest.mark.parametrize("tail", ["own", "pad"])
def test_refine_window_cutting(t, tail):
    from v2a_amd.roll2midi import window_spans
    from v2a_amd.synth import synthetic_key_roll
    roll = synthetic_key_roll(2, t, 51, 3)
    eng = _FakeRun()
    probs, midi = eng.refine(roll, window=100, threshold=0.4, tail=tail)
    want = np.empty((2, t, 51), np.float32)
    r = roll.numpy()
    spans = [(s, min(s + 100, t)) for s in range(0, t, 100)]
    assert window_spans(t, 100) == spans
    for b in range(2):
        for s, e in spans:
            win = r[b, s:e]
            if tail == "pad" and e - s < 100:
                win = np.concatenate([win, np.full((100 - (e - s), 51), 0.5, np.float32)])
            out = _FakeRun.f(torch.from_numpy(win.T.copy())[None]).numpy()[0].T
            want[b, s:e] = out[:e - s]
    assert np.array_equal(probs.numpy(), want)
    assert np.array_equal(midi.numpy(), (want >= 0.4).astype(np.uint8)) and midi.dtype == torch.uint8
    assert {c[2] for c in eng.calls} == ({100} if tail == "pad" else {e - s for s, e in spans})
    with pytest.raises(ValueError, match="tail"):
        eng.refine(roll, tail="zero")


def test_attention_gate_variant_and_bad_state_dicts_are_refused(params):
    from v2a_amd.roll2midi import Roll2MidiEngine, check_state_dict
    check_state_dict(params)
    with pytest.raises(NotImplementedError, match="Roll2MidiNet_enhance"):
        Roll2MidiEngine({**params, "att1.W_g.0.weight": torch.zeros(4)}, "cpu")
    lacking = {k: v for k, v in params.items() if k != "up3.model.1.running_var"}
    with pytest.raises(KeyError, match="up3.model.1.running_var"):
        Roll2MidiEngine(lacking, "cpu")
    with pytest.raises(ValueError, match="conv1d.weight"):
        Roll2MidiEngine({**params, "conv1d.weight": torch.zeros(1, 96, 1, 1)}, "cpu")
    with pytest.raises(ValueError, match="compute"):
        Roll2MidiEngine(params, "cpu", compute="fp16")


def test_e2tts_surface_raises_without_the_networks(lib):
    import v2a_amd
    assert v2a_amd.Roll2MidiEngine is v2a_amd.roll2midi.Roll2MidiEngine
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                       if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=16, if_cond_proj_in=False, device="cpu")
    with pytest.raises(NotImplementedError, match="video2roll_net"):
        m.frames_to_midi(torch.zeros(1, 1, 2, 100, 900))
    with pytest.raises(TypeError, match="load_roll2midi"):
        m.load_roll2midi(3)


def test_cli_argument_wiring(tmp_path, monkeypatch):
    from v2a_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(["ck.pt", "0", "t.scp", "0", "1", "out", "--piano", "--roll2midi", "g.tar"])
    assert a.roll2midi == "g.tar" and a.roll2midi_dtype == "bf16x3" and a.piano
    assert ap.parse_args(["ck.pt", "0", "t.scp", "0", "1", "out"]).roll2midi is None
    with pytest.raises(SystemExit):
        cli.main(["ck.pt", "0", "t.scp", "0", "1", "out", "--roll2midi", "g.tar"])          # without --piano

    class Model:
        def frames_to_midi(self, frames):
            t = frames.shape[2]
            p = torch.arange(2 * t * 51, dtype=torch.float32).reshape(2, t, 51) / (2 * t * 51)
            return p, (p >= 0.5).to(torch.uint8)

    paths = cli.write_midi_rolls(Model(), torch.zeros(2, 1, 4, 100, 900), ["/x/a.mp4", "/y/b.mp4"], str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["a.midi.npz", "b.midi.npz"]
    z = np.load(paths[1])
    assert z["midi"].shape == (4, 51) and z["midi"].dtype == np.uint8 and z["prob"].shape == (4, 51) and z["prob"].dtype == np.float32
    assert np.array_equal(z["midi"], (z["prob"] >= 0.5).astype(np.uint8)) and z["midi"].all()
