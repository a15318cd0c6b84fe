"""GPU: DiTEngine.late_ex moves a wait and nothing else, so the latents must not move.

Engine of depth 4 at the shipped widths, T = 75 (N = 107 rows per sequence: one full and one ragged 64-row band), one and two clips, bf16x3 and
bf16, three streams, captured graph and eager loop.  A sample() of four consecutive evaluations with `late_ex` on must equal the one with it
off under torch.equal, three times over: both issue the same launches with the same arguments per stream, so anything but equality is a race
between the streams (tests/test_schedule_hazards.py checks the same schedule on the CPU, edge by edge)."""
import pytest
import torch

from conftest import make_model
from oracle import e2_cfm_oracle as O

pytestmark = pytest.mark.gpu

T_, NC, STEPS = 75, 8, 5            # S = 4 evaluations
_MODELS = {}


@pytest.fixture(scope="module")
def case():
    cfg = O.DiTConfig(depth=4, max_seq_len=128)
    P = O.init_params(cfg, 31)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, T_, nc=NC, seed=5, piano=True)
    yield dict(cfg=cfg, P=P, y0=y0, text=text, roll=roll, ctx=ctx, cm=cm)
    _MODELS.clear()


def _model(case, mode, use_graph):
    if (mode, use_graph) not in _MODELS:
        _MODELS[(mode, use_graph)] = make_model(case["cfg"], case["P"], mode, use_graph=use_graph)
    return _MODELS[(mode, use_graph)]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_latents_equal_with_late_ex_on_and_off(case, mode, B, use_graph):
    c = case
    m = _model(c, mode, use_graph)
    eng = m.engine()
    assert eng.multi_stream and not eng.cross_on_main
    kw = dict(y0=c["y0"][:B], text_embed=c["text"][:B], context=c["ctx"][:B], context_mask=c["cm"][:B], frames_embed=c["roll"][:B], steps=STEPS,
              cfg_strength=2.0, remove_parallel_component=False, return_raw_output=True)
    run = lambda: m.sample(torch.zeros(B, T_, c["cfg"].num_channels), **kw).float().cpu()
    try:
        for rep in range(3):
            eng.late_ex = True
            on = run()
            assert eng.plan.get("st") is not None, "the plan runs on three streams"
            eng.late_ex = False
            off = run()
            assert torch.isfinite(on).all() and not torch.equal(on, c["y0"][:B])
            assert torch.equal(on, off), (mode, B, use_graph, rep, float((on - off).abs().max()))
    finally:
        eng.late_ex = True
