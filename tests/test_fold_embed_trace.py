"""CPU: the launch sequence of the folded embed (DiTEngine.fold_embed / begin_steps), with the recorder of tests/test_launch_trace.py.

An ARMED evaluation -- setup, prepare(fold_embed=True), begin_steps(y0), euler_step(plan["y"]) as E2TTS.sample runs them -- has no
v2a_linear_small / v2a_split_bf16, opens with layer 0's three cross-condition GEMMs as one-segment K = num_channels launches with the RESID
epilogue on the offset tables, runs the rest of the evaluation as before and ends with v2a_cfg_euler_planes.  An UNARMED one -- prepare()
and euler_step() without begin_steps, the sequence tests/golden/launch_trace.json.gz pins -- does not depend on the switch; where the fold
does not apply (bf16, fp32, num_channels % 64 != 0, a tensor that is not the plan's y) begin_steps arms nothing and the launches are today's."""
import pytest
import torch

import test_launch_trace as LT
from v2a_amd import _lib as L
from v2a_amd.dit import DiTConfig, DiTEngine

T, NC, S = 150, 16, 4


def _names(calls):
    return [c["fn"] for c in calls]


def _sampled(cfg_kw, mode, B, *, attrs=None, evaluate=True, own_y=True, fold=True):
    """(calls of prepare + begin_steps, calls of the evaluation, armed) of one sample()-like sequence."""
    out = {}

    def run(roots):
        cfg = DiTConfig(**cfg_kw)
        eng = DiTEngine(cfg, LT._state_dict(cfg), device="cpu", compute=mode)
        for k, v in (attrs or {}).items():
            setattr(eng, k, v)
        i = LT._inputs(cfg, B, T, NC, S)
        roots += [eng, i]
        eng.setup(B, T, NC, S)
        eng.prepare(i["text"], i["roll"], i["ctx"], i["ctx_mask"], i["t"], dt=i["dt"], fold_embed=fold)
        y = eng.begin_steps(i["y"])
        out["armed"] = eng.plan["armed"]
        out["sig"] = eng.launch_signature()
        if evaluate:
            eng.euler_step(y if own_y else i["y"], 2.0)

    calls = LT._traced(run)
    return calls, out


def _split(cfg_kw, mode, B, **kw):
    head, o = _sampled(cfg_kw, mode, B, evaluate=False, **kw)
    full, o2 = _sampled(cfg_kw, mode, B, **kw)
    assert _names(full[:len(head)]) == _names(head) and o["armed"] == o2["armed"]
    return head, full[len(head):], o2


@pytest.mark.parametrize("B", [1, 2])
def test_armed_evaluation(B):
    head, ev, o = _split(LT.SHIPPED, "bf16x3", B)
    assert o["armed"]
    names = _names(ev)
    assert "v2a_linear_small" not in names and "v2a_split_bf16" not in names and "v2a_cfg_euler" not in names
    assert names[-2:] == ["v2a_cfg_euler_planes", "v2a_step_advance"]
    rows = 2 * B * (T + 32)
    k128 = [c for c in ev if c["fn"] == "v2a_gemm" and c["args"][0]["nseg"] == 1 and c["args"][0]["ka"][0] == 128]
    assert ev[:3] == k128 and len(k128) == 3
    assert [c["args"][0]["N"] for c in k128] == [1024, 1280, 512]
    for c in k128:
        g = c["args"][0]
        assert g["M"] == rows and g["epilogue"] == L.EPI_RESID and g["a_dtype"] == L.BF16_SPLIT and g["lda"][0] == 256 and g["resid"] is not None
        assert g["a"][0] == k128[0]["args"][0]["a"][0]                  # one operand buffer for the three
    assert k128[0]["args"][0]["out_bf16"] is not None and k128[1]["args"][0]["out_bf16"] is None     # skips[0] keeps its shadow
    pl = ev[-2]["args"][12]
    assert pl["planes"] == k128[0]["args"][0]["a"][0] and (pl["ld"], pl["lo_offset"], pl["row_off"], pl["rows_per_seq"], pl["copies"]) == (256, 128, 32, T + 32, 2)
    # prepare ran the unfolded head once, at y = 0, into the tables the three GEMMs add; begin_steps wrote the planes of both halves
    hn = _names(head)
    assert hn.count("v2a_linear_small") == 2 and hn[-2 * B:] == ["v2a_split_bf16"] * (2 * B)
    tables = [c["args"][0]["out"] for c in head if c["fn"] == "v2a_gemm"][-3:]
    assert tables == [c["args"][0]["resid"] for c in k128]
    # the rest of the evaluation is the unarmed one's
    _, ev_off, o_off = _split(LT.SHIPPED, "bf16x3", B, attrs=dict(fold_embed=False))
    assert not o_off["armed"] and o_off["sig"] != o["sig"]
    assert _names(ev_off[:5]) == ["v2a_linear_small", "v2a_split_bf16", "v2a_gemm", "v2a_gemm", "v2a_gemm"]
    assert [c["args"][0]["ka"] for c in ev_off[2:5]] == [[1024, 1280, 512], [1024, 1280, 0], [1024, 512, 0]]
    key = lambda c: (c["fn"], c["prof"] and c["prof"][0])
    assert [key(c) for c in ev[3:-2]] == [key(c) for c in ev_off[5:-2]]
    assert _names(ev_off[-2:]) == ["v2a_cfg_euler", "v2a_step_advance"]


@pytest.mark.parametrize("mode", LT.MODES)
def test_unarmed_sequence_does_not_depend_on_the_switch(mode):
    """prepare() -> euler_step() without begin_steps(): the pinned sequence, whatever the switch says."""
    on = LT._dit_case(LT.SHIPPED, mode, 1, T=T, nc=NC)()
    off = LT._dit_case(LT.SHIPPED, mode, 1, T=T, nc=NC, attrs=dict(fold_embed=False))()
    assert on == off and "v2a_cfg_euler_planes" not in _names(on)


@pytest.mark.parametrize("why,cfg_kw,mode,kw", [
    ("bf16", LT.SHIPPED, "bf16", {}),
    ("fp32", LT.SHIPPED, "fp32", {}),
    ("C=16", LT.SMALL, "bf16x3", {}),                      # num_channels % 64 != 0: G is not packed
    ("not the plan's y", LT.SHIPPED, "bf16x3", dict(own_y=False)),
    ("prepare() without fold_embed", LT.SHIPPED, "bf16x3", dict(fold=False)),
])
def test_fallbacks_issue_todays_launches(why, cfg_kw, mode, kw):
    head, ev, o = _split(cfg_kw, mode, 1, **kw)
    plain = LT._dit_case(cfg_kw, mode, 1, T=T, nc=NC)()
    if why == "not the plan's y":
        assert o["armed"]
        n_prep = len(plain) - len(ev)
    else:
        assert not o["armed"]
        n_prep = len(head)
        assert _names(head) == _names(plain[:n_prep])      # no table launches, no plane launches
    assert _names(ev) == _names(plain[n_prep:])
    assert "v2a_cfg_euler_planes" not in _names(ev) and _names(ev)[0] == "v2a_linear_small"
