"""CPU: who takes the one-launch step seam (DiTEngine.fuse_step_seam), with the recorder of tests/test_launch_trace.py.

With the switch on (it is off by default) an armed evaluation without APG ends with ONE v2a_gemm_cfg_euler in place of to_pred's v2a_gemm, v2a_cfg_euler_planes and v2a_step_advance, with
the GEMM arguments of the to_pred launch; everything in front of it is launched as before.  APG, the switch off (the default: test_default_is_the_three_launches), and every caller that
is not armed (prepare() -> euler_step(), bf16, fp32) keep the three launches, launch for launch."""
import pytest

import test_launch_trace as LT
from v2a_amd import _lib as L
from v2a_amd.dit import DiTConfig, DiTEngine

T, NC, S = 150, 16, 4


def _evaluation(mode, B, *, attrs=None, apg=False, arm=True):
    """(calls of one euler_step, armed, launch signature) after setup -> prepare -> [begin_steps]."""
    out = {}

    def run(roots):
        cfg = DiTConfig(**LT.SHIPPED)
        eng = DiTEngine(cfg, LT._state_dict(cfg), device="cpu", compute=mode)
        for k, v in (attrs or {}).items():
            setattr(eng, k, v)
        i = LT._inputs(cfg, B, T, NC, S)
        roots += [eng, i]
        eng.setup(B, T, NC, S)
        eng.prepare(i["text"], i["roll"], i["ctx"], i["ctx_mask"], i["t"], dt=i["dt"], fold_embed=arm)
        y = eng.begin_steps(i["y"]) if arm else i["y"]
        out.update(armed=eng.plan["armed"], sig=eng.launch_signature(), n=None)
        out["mark"] = len(tr_calls())
        eng.euler_step(y, 2.0, apg)

    box = []
    tr_calls = lambda: box[0].calls if box else []
    orig = LT._Trace

    class _T(orig):
        def __init__(self):
            super().__init__()
            box.append(self)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(LT, "_Trace", _T)
        calls = LT._traced(run)
    return calls[out["mark"]:], out


def _names(calls):
    return [c["fn"] for c in calls]


@pytest.mark.parametrize("B", [1, 2])
def test_armed_evaluation_ends_with_one_launch(B):
    on, o = _evaluation("bf16x3", B, attrs=dict(fuse_step_seam=True))
    off, o_off = _evaluation("bf16x3", B, attrs=dict(fuse_step_seam=False))
    assert o["armed"] and o_off["armed"] and o["sig"] != o_off["sig"]
    assert _names(off[-3:]) == ["v2a_gemm", "v2a_cfg_euler_planes", "v2a_step_advance"]
    assert _names(on[-1:]) == ["v2a_gemm_cfg_euler"] and len(on) == len(off) - 2
    assert on[:-1] == off[:-3]
    g, s = on[-1]["args"][0], on[-1]["args"][1]
    assert g == off[-3]["args"][0]                                                    # the to_pred GEMM, argument for argument
    pl = off[-2]["args"][12]
    rows = 2 * B * (T + 32)
    assert g["M"] == rows and g["N"] == 128 and g["epilogue"] == L.EPI_STORE and g["a_dtype"] == L.BF16_SPLIT
    assert (s["planes"], s["ld"], s["lo_offset"], s["row_off"], s["rows_per_seq"]) == (pl["planes"], pl["ld"], pl["lo_offset"], pl["row_off"], pl["rows_per_seq"])
    assert (s["B"], s["T"], s["cfg_strength"]) == (B, T, 2.0) and s["y"] == off[-2]["args"][0] and s["step"] == off[-1]["args"][0]
    assert s["arrive"] is not None and s["arrive"] != s["step"]


def test_apg_keeps_the_three_launches():
    on, o = _evaluation("bf16x3", 1, apg=True, attrs=dict(fuse_step_seam=True))
    off, _ = _evaluation("bf16x3", 1, apg=True, attrs=dict(fuse_step_seam=False))
    assert o["armed"] and on == off
    assert _names(on[-4:]) == ["v2a_gemm", "v2a_apg_reduce", "v2a_cfg_euler_planes", "v2a_step_advance"]


@pytest.mark.parametrize("mode", LT.MODES)
def test_unarmed_callers_keep_the_three_launches(mode):
    on, o = _evaluation(mode, 1, arm=False, attrs=dict(fuse_step_seam=True))
    off, _ = _evaluation(mode, 1, arm=False, attrs=dict(fuse_step_seam=False))
    assert not o["armed"] and on == off and "v2a_gemm_cfg_euler" not in _names(on)
    assert _names(on[-2:]) == ["v2a_cfg_euler", "v2a_step_advance"]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_plain_modes_are_never_armed(mode):
    on, o = _evaluation(mode, 1, attrs=dict(fuse_step_seam=True))
    assert not o["armed"] and "v2a_gemm_cfg_euler" not in _names(on) and _names(on[-2:]) == ["v2a_cfg_euler", "v2a_step_advance"]


def test_default_is_the_three_launches():
    default, o = _evaluation("bf16x3", 1)
    off, _ = _evaluation("bf16x3", 1, attrs=dict(fuse_step_seam=False))
    assert o["armed"] and default == off and _names(default[-3:]) == ["v2a_gemm", "v2a_cfg_euler_planes", "v2a_step_advance"]
