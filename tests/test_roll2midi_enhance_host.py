"""CPU: the host side of the attention-gated Roll2Midi generator (roll2midi.py: Roll2MidiEnhanceEngine, folded_gate, engine_for): the
state-dict layout against the reference module's key list, the gate fold against its unfused float64 composition, ABI agreement and
argument checks of `v2a_roll2midi_gate`, the choice of the engine class, and the launch sequence of one pass against a recording
library.  No GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "roll2midi_enhance.npz")


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


@pytest.fixture(scope="module")
def params():
    from v2a_amd.synth import random_roll2midi_enhance_state_dict
    return random_roll2midi_enhance_state_dict(4321)


def test_expected_shapes_are_the_reference_modules_key_list(params):
    from v2a_amd.roll2midi import expected_enhance_state_dict_shapes
    g = np.load(GOLD, allow_pickle=False)
    want = {str(k): tuple(int(d) for d in str(s).split("x") if d) for k, s in zip(g["state_dict_keys"], g["state_dict_shapes"])}
    got = expected_enhance_state_dict_shapes()
    assert got == want
    assert list(got) == [str(k) for k in g["state_dict_keys"]]          # the module's own order: the seeded draw depends on it
    assert got["att1.theta_x.weight"] == (512, 2048, 1, 1) and got["att1.phi_g.weight"] == (512, 1024, 1, 1)
    assert got["att1.psi.weight"] == (1, 512, 1, 1) and got["conv1d.weight"] == (1, 128, 1, 1)
    assert list(params) == list(want) and all(tuple(params[k].shape) == shp for k, shp in want.items())
    assert float(params["conv1d.bias"][0]) == -2.0


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_folded_gate_is_the_unfused_composition(params, k):
    """w . x + b against psi(theta_x(x) + phi_g(g)) in float64 on random pixels, g the last Cg channels of x (enh:49-53, 96)."""
    from v2a_amd.roll2midi import folded_gate
    g = torch.Generator().manual_seed(k)
    sd = {n: torch.randn(v.shape, generator=g, dtype=torch.float64) for n, v in params.items() if n.startswith(f"att{k}.")}
    theta, phi, psi = (sd[f"att{k}.{n}.weight"].flatten(1) for n in ("theta_x", "phi_g", "psi"))
    C, Cg = theta.shape[1], phi.shape[1]
    x = torch.randn(200, C, generator=g, dtype=torch.float64)
    f = x @ theta.t() + sd[f"att{k}.theta_x.bias"] + x[:, C - Cg:] @ phi.t() + sd[f"att{k}.phi_g.bias"]
    ref = (f @ psi.t() + sd[f"att{k}.psi.bias"])[:, 0]
    # folded_gate rounds w to fp32 once; the fold itself is checked on its float64 form, so compute it as folded_gate does
    w64 = (psi @ theta)[0]
    w64[C - Cg:] += (psi @ phi)[0]
    b64 = float(psi[0] @ (sd[f"att{k}.theta_x.bias"] + sd[f"att{k}.phi_g.bias"]) + sd[f"att{k}.psi.bias"][0])
    w, b = folded_gate(sd, k)
    assert w.dtype == torch.float32 and w.shape == (C,) and isinstance(b, float)
    assert torch.equal(w, w64.float()) and b == b64                       # float64, rounded once
    err = float(((x @ w64 + b) - ref).abs().max() / ref.abs().max())
    print(f"gate {k}: folded vs unfused, max |d| / max |ref| = {err:.2e}")
    assert err < 1e-12


def test_header_ctypes_and_exports_agree(lib):
    src = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "v2a_stream_t": ctypes.c_void_p}
    L = lib.lib()
    name = "v2a_roll2midi_gate"
    assert name in lib.EXPORTS
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, re.S)
    assert proto, f"{name} is not declared in include/v2a_cfm.h"
    want = []
    for arg in proto.group(1).split(","):
        arg = arg.strip()
        want.append(ctypes.c_void_p if "*" in arg else ctype[arg.replace("const ", "").split()[0]])
    fn = getattr(L, name)
    assert fn.argtypes == want, (fn.argtypes, want)
    assert fn.restype is ctypes.c_int
    assert L.v2a_abi_version() == lib.ABI_VERSION == 9              # the entry point is additive


def test_gate_entry_point_validates_on_cpu(lib):
    """Bad arguments are refused before any HIP call.  (x0, pitch0, C0, shadow0, lo0, x1, pitch1, C1, shadow1, lo1, w, bias, mode, n, H,
    W, border, logits, alpha, stream)"""
    L = lib.lib()
    gate = L.v2a_roll2midi_gate
    assert gate(None, 64, 64, None, 0, None, 0, 0, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"null" in L.v2a_last_error()
    assert gate(16, 64, 60, None, 0, None, 0, 0, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"geometry" in L.v2a_last_error()
    assert gate(16, 128, 64, None, 0, 32, 64, 60, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"geometry" in L.v2a_last_error()
    assert gate(16, 64, 64, 32, 0, None, 0, 0, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"shadow" in L.v2a_last_error()
    assert gate(16, 64, 64, None, 0, None, 0, 0, None, 0, 16, 0.0, 1, 1, 5, 3, 1, None, None, None) == -1 and b"shadow" in L.v2a_last_error()
    assert gate(16, 128, 64, 32, 0, 48, 128, 64, None, 0, 16, 0.0, 1, 1, 5, 3, 1, None, None, None) == -1 and b"shadow" in L.v2a_last_error()
    assert gate(16, 4096, 2056, None, 0, None, 0, 0, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"2048" in L.v2a_last_error()
    assert gate(16, 2048, 1032, None, 0, 32, 2048, 1024, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"at most" in L.v2a_last_error()
    assert gate(16, 64, 64, None, 0, 32, 0, 0, None, 0, 16, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"second segment" in L.v2a_last_error()
    assert gate(16, 64, 64, None, 0, None, 0, 0, None, 0, None, 0.0, 0, 1, 5, 3, 1, None, None, None) == -1 and b"weight" in L.v2a_last_error()
    assert gate(16, 64, 64, 32, 8, None, 0, 0, None, 0, 16, 0.0, 2, 1, 5, 3, 1, None, None, None) == -1 and b"lo_offset" in L.v2a_last_error()


def test_engine_for_picks_the_class(params, monkeypatch):
    from v2a_amd import roll2midi as R
    from v2a_amd.synth import random_roll2midi_state_dict
    made = []
    monkeypatch.setattr(R.Roll2MidiEngine, "__init__", lambda self, sd, device="cuda:0", **kw: made.append((type(self), device, kw)))
    plain = random_roll2midi_state_dict(1)
    assert type(R.engine_for(plain, "cpu", compute="fp32")) is R.Roll2MidiEngine
    assert type(R.engine_for(params, "cpu", chunk=3)) is R.Roll2MidiEnhanceEngine
    assert type(R.engine_for({"g." + k: v for k, v in params.items()}, "cpu", prefix="g.")) is R.Roll2MidiEnhanceEngine
    assert made == [(R.Roll2MidiEngine, "cpu", dict(compute="fp32")), (R.Roll2MidiEnhanceEngine, "cpu", dict(chunk=3)),
                    (R.Roll2MidiEnhanceEngine, "cpu", dict(prefix="g."))]
    assert issubclass(R.Roll2MidiEnhanceEngine, R.Roll2MidiEngine)


def test_plain_engine_still_refuses_the_gates_and_the_new_one_checks_its_layout(params, lib):
    import v2a_amd
    from v2a_amd.roll2midi import Roll2MidiEngine, Roll2MidiEnhanceEngine
    assert v2a_amd.Roll2MidiEnhanceEngine is Roll2MidiEnhanceEngine and "Roll2MidiEnhanceEngine" in v2a_amd.__all__
    with pytest.raises(NotImplementedError, match="Roll2MidiNet_enhance.*Roll2MidiEnhanceEngine"):
        Roll2MidiEngine(params, "cpu")
    lacking = {k: v for k, v in params.items() if k != "att3.phi_g.bias"}
    with pytest.raises(KeyError, match="att3.phi_g.bias"):
        Roll2MidiEnhanceEngine(lacking, "cpu")
    with pytest.raises(ValueError, match="conv1d.weight"):
        Roll2MidiEnhanceEngine({**params, "conv1d.weight": torch.zeros(1, 80, 1, 1)}, "cpu")
    with pytest.raises(ValueError, match="compute"):
        Roll2MidiEnhanceEngine(params, "cpu", compute="fp16")


def test_load_roll2midi_rejects_non_dicts_and_takes_either_engine(lib):
    import v2a_amd
    from v2a_amd.roll2midi import Roll2MidiEnhanceEngine
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                       if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=16, if_cond_proj_in=False, device="cpu")
    with pytest.raises(TypeError, match="load_roll2midi"):
        m.load_roll2midi(3)
    with pytest.raises(TypeError, match="load_roll2midi"):
        m.load_roll2midi([1, 2])
    eng = Roll2MidiEnhanceEngine.__new__(Roll2MidiEnhanceEngine)          # an instance is taken as it is
    assert m.load_roll2midi(eng) is eng and m._r2m is eng


# ---- the launch sequence of one pass, against a library that records instead of launching ------------------------------------------
class _Recorder:
    def __init__(self, L):
        self.calls = []
        for name in L.EXPORTS:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_launch_sequence_of_one_pass(lib, mode, monkeypatch):
    """stem, (down_k, leaky) x 5, (up_k, gate_k) x 4, up5, head; a gated up block asks its GEMM for no shadow, up5 does; the gate's two
    segments are up_k's output and d_(6-k), inside one concatenated bordered map (implicit GEMM) or two dense buffers (fp32)."""
    from v2a_amd.roll2midi import Roll2MidiEnhanceEngine, expected_enhance_state_dict_shapes
    L = lib
    rec = _Recorder(L)
    monkeypatch.setattr(L, "_lib", rec)
    monkeypatch.setattr(L, "stream_ptr", lambda: 0)
    eng = Roll2MidiEnhanceEngine({k: torch.zeros(s) for k, s in expected_enhance_state_dict_shapes().items()}, "cpu", compute=mode)
    assert eng.chunk == (2 if mode == "fp32" else 8)
    n, H, W = 2, 6, 5
    taps = {}
    eng.forward(torch.zeros(n, 1, H, W), taps=taps)
    names = [c[0] for c in rec.calls]
    conv = ["v2a_gemm"] if mode != "fp32" else ["v2a_im2col", "v2a_gemm"]
    conv2 = ["v2a_gemm"] if mode != "fp32" else ["v2a_im2col", "v2a_im2col", "v2a_gemm"]
    want = ["v2a_roll2midi_stem"] + (conv + ["v2a_leaky_shadow"]) * 5 + conv + ["v2a_roll2midi_gate"] + (conv2 + ["v2a_roll2midi_gate"]) * 3 \
        + conv2 + ["v2a_roll2midi_head"]
    assert names == want
    gemms = [c[1][0]._obj for c in rec.calls if c[0] == "v2a_gemm"]
    assert [g.N for g in gemms] == [128, 256, 512, 1024, 1024, 1024, 512, 256, 128, 64]
    assert [sum(g.ka[:g.nseg]) for g in gemms[5:]] ==[9 * c for c in (1024, 2048, 1024, 512, 256)]
    shadows = [bool(g.out_bf16) for g in gemms]
    assert shadows == [False] * 9 + [mode != "fp32"]                     # only up5's epilogue writes a shadow
    gates = [c[1] for c in rec.calls if c[0] == "v2a_roll2midi_gate"]
    b = 0 if mode == "fp32" else 1
    sm = {"fp32": 0, "bf16": 1, "bf16x3": 2}[mode]
    for k, (g, (cu, cd)) in enumerate(zip(gates, ((1024, 1024), (512, 512), (256, 256), (128, 128))), 1):
        x0, p0, c0, s0, l0, x1, p1, c1, s1, l1, w, bias, smode, gn, gH, gW, border, logits, alpha, stream = g
        assert (c0, c1, smode, gn, gH, gW, border) == (cu, cd, sm, n, H, W, b)
        assert w == eng.gate_w[k].data_ptr() and eng.gate_w[k].shape == (cu + cd,) and logits == 0 and alpha != 0
        if mode == "fp32":
            assert (p0, p1, s0, s1, l0, l1) == (cu, cd, 0, 0, 0, 0) and x0 != x1
        else:
            plane = n * (H + 2) * (W + 2) * (cu + cd)
            assert p0 == p1 == cu + cd and x1 - x0 == 4 * cu and s1 - s0 == 2 * cu          # one map: d_(6-k) behind up_k's channels
            assert l0 == l1 == (plane if mode == "bf16x3" else 0)
    head = rec.calls[-1][1]
    assert (head[2], head[5]) == (64, 64)                               # nu, nd
    assert sorted(taps) == sorted([f"d{i}" for i in range(1, 7)] + [f"u{i}" for i in range(1, 6)] + [f"a{i}" for i in range(1, 5)])
    assert [tuple(taps[f"u{i}"][0].shape) for i in range(1, 6)] == [(n, c, H, W) for c in (2048, 1024, 512, 256, 128)]
    assert all(tuple(taps[f"a{i}"][0].shape) == (n, 1, H, W) for i in range(1, 5))
    # without taps no alpha map is asked for
    rec.calls.clear()
    eng.forward(torch.zeros(n, 1, H, W))
    assert all(c[1][18] == 0 for c in rec.calls if c[0] == "v2a_roll2midi_gate")
