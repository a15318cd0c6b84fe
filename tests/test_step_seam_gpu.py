"""GPU: the step seam in one launch (DiTEngine.fuse_step_seam, v2a_gemm_cfg_euler in csrc/gemm.hip) against the three launches it replaces.

Engine of depth 4 at the shipped widths, bf16x3, T = 75 (N = 107 rows per sequence) and T = 96 (N = 128), one and two clips.  An armed plan runs
three consecutive evaluations with the fused seam and three with to_pred, v2a_cfg_euler_planes and v2a_step_advance; after every evaluation y,
the whole of `ybuf` (hi and lo planes of both halves, register rows included), plan["pred"] (all rows) and the step counter must be equal bit
for bit, and the arrival counter must be back at zero.  The register rows of `ybuf` carry a sentinel that no launch may touch.  With APG
requested the evaluation must issue the old launches."""
import pytest
import torch

from conftest import make_model
from oracle import e2_cfm_oracle as O

pytestmark = pytest.mark.gpu

NC, S = 8, 4
SENTINEL = 0.5


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def model():
    cfg = O.DiTConfig(depth=4, max_seq_len=128)
    P = O.init_params(cfg, 41)
    return cfg, make_model(cfg, P, "bf16x3", use_graph=False)


def _armed(model, B, T, fused):
    cfg, m = model
    eng = m.engine()
    eng.fuse_step_seam = fused
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, B, T, nc=NC, seed=7, piano=True)
    t = O.sway_grid(S + 1)
    eng.setup(B, T, NC, S)
    eng.prepare(text, roll, ctx, cm, t[:-1], dt=t[1:] - t[:-1], fold_embed=True)
    y = eng.begin_steps(y0)
    p = eng.plan
    assert p["armed"]
    R, N, C_ = cfg.num_registers, p["N"], cfg.num_channels
    planes = p["ybuf"].t.view(p["Bt"], N, 2 * C_)
    planes[:, :R] = SENTINEL
    return eng, p, y, planes, R


def _three_steps(model, B, T, fused, apg=False):
    eng, p, y, planes, R = _armed(model, B, T, fused)
    snaps = []
    for k in range(3):
        eng.euler_step(y, 2.0, apg)
        torch.cuda.synchronize()
        assert int(p["arrive"].item()) == 0, "the arrival counter is back at zero after every step"
        assert int(p["step"].item()) == k + 1
        assert bool((planes[:, :R] == SENTINEL).all()), "register rows of the planes are not touched"
        snaps.append(dict(y=y.clone(), ybuf=p["ybuf"].t.clone(), pred=p["pred"].clone(), step=p["step"].clone()))
    return snaps


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [75, 96])
def test_fused_seam_equals_three_launches(model, T, B):
    try:
        a, b = _three_steps(model, B, T, True), _three_steps(model, B, T, False)
    finally:
        model[1].engine().fuse_step_seam = False
    for k, (x, z) in enumerate(zip(a, b)):
        assert torch.isfinite(x["y"]).all() and torch.isfinite(x["pred"]).all()
        for name in ("y", "ybuf", "pred", "step"):
            assert torch.equal(x[name], z[name]), (T, B, k, name, float((x[name].float() - z[name].float()).abs().max()))
    assert not torch.equal(a[0]["y"], a[1]["y"])
    planes = a[2]["ybuf"].view(2, B, -1, a[2]["ybuf"].shape[-1])
    assert torch.equal(planes[0], planes[1]) and bool(planes[:, :, model[0].num_registers:].any())     # both halves hold the planes of y


def _launches(L, run):
    prof = L.KernelProfiler()
    L.set_profiler(prof)
    try:
        run()
    finally:
        L.set_profiler(None)
    s = prof.summary()
    n = lambda pred: sum(v["launches"] for k, v in s.items() if pred(k))
    return dict(fused=n(lambda k: k.startswith("gemm<") and "cfg_euler" in k), cfg_euler=n(lambda k: k.startswith("cfg_euler")),
                gemm=n(lambda k: k.startswith("gemm<")))


def test_apg_keeps_the_three_launches(L, model):
    eng, p, y, planes, R = _armed(model, 1, 75, True)
    plain = _launches(L, lambda: eng.euler_step(y, 2.0, False))
    apg = _launches(L, lambda: eng.euler_step(y, 2.0, True))
    eng.fuse_step_seam = False
    off = _launches(L, lambda: eng.euler_step(y, 2.0, False))
    torch.cuda.synchronize()
    assert plain == dict(fused=1, cfg_euler=0, gemm=off["gemm"]), (plain, off)
    assert apg == off == dict(fused=0, cfg_euler=1, gemm=off["gemm"]), (apg, off)
    assert int(p["step"].item()) == 3 and int(p["arrive"].item()) == 0


def test_fused_seam_graph_equals_eager(L):
    """Depth-2 engine at the SMALL widths of tests/test_fold_embed_gpu.py with the fused seam: the captured armed evaluation replayed S = 4 times
    against the eager loop -- y, the planes of both halves, the predictions, the step and the arrival counter, bit for bit (as
    test_graph_equals_eager there does for the three launches)."""
    from test_fold_embed_gpu import SMALL
    cfg = O.DiTConfig(**SMALL)
    P = O.init_params(cfg, 11)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 37, nc=NC, seed=3, piano=True)
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, steps=S + 1, cfg_strength=2.0,
              remove_parallel_component=False, return_raw_output=True)
    models = [make_model(cfg, P, "bf16x3"), make_model(cfg, P, "bf16x3", use_graph=False)]
    got, fused = [], []
    try:
        for m, eager in zip(models, (False, True)):
            m.engine().fuse_step_seam = True
            run = lambda: got.append((m.sample(torch.zeros(2, 37, cfg.num_channels), **kw).float().cpu(),))      # noqa: E731
            fused.append(_launches(L, run)["fused"] if eager else run())        # launches are counted on the eager loop only
            torch.cuda.synchronize()
            p = m.engine().plan
            assert p["armed"]
            got[-1] += (dict(y=p["y"].clone(), ybuf=p["ybuf"].t.clone(), pred=p["pred"].clone(), step=p["step"].clone(), arrive=p["arrive"].clone()),)
    finally:
        for m in models:
            m.engine().fuse_step_seam = False
    (ya, a), (yb, b) = got
    assert models[0].graph_captures == 1 and models[1].graph_captures == 0
    assert fused[1] == S, "the eager loop issues the one-launch seam in every evaluation"
    assert torch.isfinite(ya).all() and torch.equal(ya, yb) and not torch.equal(ya, y0)
    for name in ("y", "ybuf", "pred", "step", "arrive"):
        assert torch.equal(a[name], b[name]), (name, float((a[name].float() - b[name].float()).abs().max()))
    assert int(a["step"].item()) == S and int(a["arrive"].item()) == 0
