"""GPU: the folded embed of the bf16x3 sampler (DiTEngine.fold_embed, begin_steps; v2a_cfg_euler_planes in csrc/rowops.hip).

(a) test_cfg_euler_planes     the launch with plane outputs against the plain one on the same inputs: y equal bit for bit, the frame rows of
                              both halves of the operand buffer equal to L.split_planes(y), register rows and the columns behind the planes
                              untouched.  B in {1, 2}, T in {5, 70}, C in {64, 128}, device step first / last, cfg strength 0 / 2, APG on / off.
(b) test_layer0_outputs       engine, depth 2, dim 512 / 256 / 128, T = 37, nc = 8, S = 4: skips[0], tbuf[0], fbuf[0] of an armed evaluation
                              against float64 of the straightforward formula on the device's own tL0 / fL0.  Bar: the one
                              tests/test_gemm_split_ring_gpu.py applies to a split GEMM, 3e-5 max(max |acc|, 1) with acc the float64 product
                              -- for the armed path the sum of the two launches' bars (the K = D + Dt + Df table launch at y = 0 and the K = C
                              launch).  The unfolded path is held to ITS bar by the same code, so the comparison is as tight as the kernel tests'.
(c) test_three_steps          three armed Euler steps against three unfolded ones: max |delta y| reported, and inside twice the unfolded path's
                              own distance to the float64 three-step result of the oracle.
(d) test_graph_equals_eager   the captured armed evaluation replayed S times equals the eager loop bit for bit.
(e) test_rearming             a second sample() with another y0, then another text, equals a fresh engine bit for bit, across a plan switch and back.
(f) test_audio_prompt         cond_proj_in + step_cond: armed against unfolded as in (c).
(g) test_fallbacks            bf16, fp32, cfg_mode=False and per_sample_t keep today's launches, counted through L.KernelProfiler."""
import pytest
import torch
import torch.nn.functional as F

from conftest import make_model
from oracle import e2_cfm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
R_EULER = 4
SENTINEL = -3.0


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------------------- (a) the kernel
@pytest.mark.parametrize("apg_on", [False, True])
@pytest.mark.parametrize("strength", [0.0, 2.0])
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("C_", [64, 128])
@pytest.mark.parametrize("T", [5, 70])
@pytest.mark.parametrize("B", [1, 2])
def test_cfg_euler_planes(L, B, T, C_, step, strength, apg_on):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + C_ + step)
    R, N, S, pad = R_EULER, R_EULER + T, 4, 8
    y0 = torch.randn(B, T, C_, generator=g).to(DEV)
    pred = torch.randn(2 * B, N, C_, generator=g).to(DEV)
    dt = (0.05 + 0.2 * torch.rand(S, generator=g)).to(DEV)
    st = torch.tensor([step], dtype=torch.int32, device=DEV)
    kw = dict(B=B, T=T, C_=C_, pred_batch_stride=N * C_, row_off=R)
    apg = None
    if apg_on:
        apg = torch.zeros(2 * B, dtype=torch.float64, device=DEV)
        L.apg_reduce(pred, apg, **kw)
    plain, withp = y0.clone(), y0.clone()
    L.cfg_euler(plain, pred, cfg_strength=strength, dt=dt, step=st, apg=apg, keep=0.3, **kw)
    buf = torch.zeros(2 * B * N, 2 * C_ + pad, dtype=torch.bfloat16, device=DEV)
    buf[:, 2 * C_:] = SENTINEL
    L.cfg_euler(withp, pred, cfg_strength=strength, dt=dt, step=st, apg=apg, keep=0.3,
                planes=dict(out=buf, ld=2 * C_ + pad, lo_offset=C_, row_off=R, rows_per_seq=N, copies=2), **kw)
    torch.cuda.synchronize()
    assert torch.equal(plain, withp) and not torch.equal(plain, y0)
    v = buf.cpu().reshape(2, B, N, 2 * C_ + pad)
    assert not bool(v[:, :, :R, :2 * C_].any())                                   # register rows still zero
    assert bool((v[..., 2 * C_:] == SENTINEL).all())                              # nothing behind the planes
    want = L.split_planes(plain.cpu().reshape(B * T, C_)).reshape(B, T, 2 * C_)
    assert torch.equal(v[0, :, R:, :2 * C_], want) and torch.equal(v[1, :, R:, :2 * C_], want)


def test_cfg_euler_planes_refuses_rows_that_do_not_fit(L):
    y, pred, dt = torch.zeros(1, 5, 64, device=DEV), torch.zeros(2, 9, 64, device=DEV), torch.zeros(1, device=DEV)
    buf = torch.zeros(2 * 9, 128, dtype=torch.bfloat16, device=DEV)
    kw = dict(B=1, T=5, C_=64, pred_batch_stride=9 * 64, row_off=4, cfg_strength=1.0, dt=dt)
    for bad in (dict(rows_per_seq=8), dict(lo_offset=32), dict(ld=120), dict(copies=3)):
        with pytest.raises(L.V2AError, match="v2a_cfg_euler_planes"):
            L.cfg_euler(y, pred, planes=dict(dict(out=buf, ld=128, lo_offset=64, row_off=4, rows_per_seq=9, copies=2), **bad), **kw)


# ------------------------------------------------------------------------------------------------------------- the engine cases
SMALL = dict(depth=2, dim=512, dim_text=256, dim_frames=128, heads=8, frames_heads=2, num_registers=4, num_channels=128, max_seq_len=128)
T_, NC, STEPS = 37, 8, 5            # S = 4 evaluations


@pytest.fixture(scope="module")
def case():
    cfg = O.DiTConfig(**SMALL)
    P = O.init_params(cfg, 11)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, T_, nc=NC, seed=3, piano=True)
    return dict(cfg=cfg, P=P, y0=y0, text=text, roll=roll, ctx=ctx, cm=cm)


def _d(x):
    return x.double() if x.is_floating_point() else x


def _kw(c, steps=STEPS, **over):
    kw = dict(y0=c["y0"], text_embed=c["text"], context=c["ctx"], context_mask=c["cm"], frames_embed=c["roll"], steps=steps, cfg_strength=2.0,
              remove_parallel_component=True, return_raw_output=True)
    kw.update(over)
    return kw


def _sample(m, kw):
    y0 = kw["y0"]
    return m.sample(torch.zeros(y0.shape[0], y0.shape[1], y0.shape[2]), **kw).float().cpu()


def _oracle64(c, kw, cfg=None, P=None, **extra):
    P64 = {k: v.double() for k, v in (P or c["P"]).items()}
    return O.sample(P64, cfg or c["cfg"], _d(kw["y0"]), _d(kw["text_embed"]), _d(kw["frames_embed"]), _d(kw["context"]), kw["context_mask"],
                    steps=kw["steps"], cfg_strength=kw["cfg_strength"], remove_parallel_component=kw["remove_parallel_component"], **extra)


# ------------------------------------------------------------------------------------------------------------- (b) layer 0
def test_layer0_outputs(case):
    c = case
    cfg, P = c["cfg"], c["P"]
    B, R, N, D, Dt, Df = 2, cfg.num_registers, cfg.num_registers + T_, cfg.dim, cfg.dim_text, cfg.dim_frames
    m = make_model(cfg, P, "bf16x3")
    eng = m.engine()
    t = O.sway_grid(STEPS)
    P64 = {k: v.double() for k, v in P.items()}
    W = {n: P64[f"transformer.layers.0.1.5.{n}.weight"] for n in ("text_frames_to_audio", "audio_to_text", "audio_to_frames")}
    bars = {}
    for armed in (True, False):
        eng.fold_embed = armed
        eng.setup(B, T_, NC, STEPS - 1)
        eng.prepare(c["text"], c["roll"], c["ctx"], c["cm"], t[:-1], dt=t[1:] - t[:-1], fold_embed=True)
        y = eng.begin_steps(c["y0"])
        p = eng.plan
        assert p["armed"] == armed
        tl, fl = p["tL0"].x.cpu().double(), p["fL0"].x.cpu().double()
        eng.euler_step(y, 2.0, True)
        torch.cuda.synchronize()
        got = dict(a=p["skips"][0].x.cpu().double(), t=p["tA"].x.cpu().double(), f=p["fA"].x.cpu().double())

        def x0(lat):
            h = F.linear(_d(lat), P64["proj_in.weight"], P64["proj_in.bias"]) + P64["transformer.abs_pos_emb.weight"][:T_]
            h = torch.cat((P64["transformer.registers"][None].expand(B, -1, -1), h), 1)
            return torch.cat((h, h), 0)

        x, xz = x0(c["y0"]), x0(torch.zeros_like(c["y0"]))
        ops = dict(a=(torch.cat((x, tl, fl), -1), torch.cat((xz, tl, fl), -1), W["text_frames_to_audio"], x),
                   t=(torch.cat((x, tl), -1), torch.cat((xz, tl), -1), W["audio_to_text"], tl),
                   f=(torch.cat((x, fl), -1), torch.cat((xz, fl), -1), W["audio_to_frames"], fl))
        bar = lambda acc: 3e-5 * max(float(acc.abs().max()), 1.0)              # _check_f32 of tests/test_gemm_split_ring_gpu.py
        for s, (a, az, w, res) in ops.items():
            acc = a @ w.t()
            ref = res + acc
            acc0 = az @ w.t()
            b = bar(acc0) + bar(acc - acc0) if armed else bar(acc)
            err = float((got[s] - ref).abs().max())
            print("fold-embed layer 0 %s stream %s: err %.3g bar %.3g (%.2f)" % ("armed" if armed else "unfolded", s, err, b, err / b))
            bars[(armed, s)] = (err, b)
            assert torch.isfinite(got[s]).all() and err < b, (armed, s, err, b)
    eng.fold_embed = True


# ------------------------------------------------------------------------------------------------------------- (c), (d) steps, graph
def _on_off(m, kw):
    eng = m.engine()
    eng.fold_embed = True
    on = _sample(m, kw)
    assert eng.plan["armed"] and eng.plan["c0_ok"]
    eng.fold_embed = False
    off = _sample(m, kw)
    assert not eng.plan["armed"]
    eng.fold_embed = True
    return on, off


def test_three_steps(case):
    kw = _kw(case, steps=4)
    on, off = _on_off(make_model(case["cfg"], case["P"], "bf16x3"), kw)
    ref = _oracle64(case, kw)
    d_on_off, d_off, d_on = float((on - off).abs().max()), float((off.double() - ref).abs().max()), float((on.double() - ref).abs().max())
    print("fold-embed three Euler steps: max |armed - unfolded| = %.3e; unfolded vs float64 %.3e, armed vs float64 %.3e" % (d_on_off, d_off, d_on))
    assert torch.isfinite(on).all() and d_on_off <= 2 * d_off


def test_graph_equals_eager(case):
    kw = _kw(case)
    g = make_model(case["cfg"], case["P"], "bf16x3")
    e = make_model(case["cfg"], case["P"], "bf16x3", use_graph=False)
    a, b = _sample(g, kw), _sample(e, kw)
    assert g.engine().plan["armed"] and e.engine().plan["armed"] and g.graph_captures == 1
    assert torch.equal(a, b)
    assert torch.equal(_sample(g, kw), a) and g.graph_captures == 1                 # replayed again from a fresh begin_steps


# ------------------------------------------------------------------------------------------------------------- (e) re-arming
def test_rearming(case):
    c = case
    y1 = torch.randn(c["y0"].shape, generator=torch.Generator().manual_seed(21))
    text2 = 0.5 * torch.randn(c["text"].shape, generator=torch.Generator().manual_seed(22))
    short = lambda x: x[:, :23].contiguous()
    calls = [_kw(c), _kw(c, y0=y1), _kw(c, y0=y1, text_embed=text2),
             _kw(c, y0=short(y1), text_embed=short(text2), frames_embed=short(c["roll"])),            # another plan ...
             _kw(c, y0=y1, text_embed=text2), _kw(c)]                                                 # ... and back
    m = make_model(c["cfg"], c["P"], "bf16x3")
    outs = [_sample(m, kw) for kw in calls]
    assert len(m.engine().plans) == 2 and m.graph_captures == 2 and m.engine().plan["armed"]
    for i, kw in enumerate(calls):
        fresh = _sample(make_model(c["cfg"], c["P"], "bf16x3"), kw)
        assert torch.equal(outs[i], fresh), (i, float((outs[i] - fresh).abs().max()))
    assert torch.equal(outs[2], outs[4]) and torch.equal(outs[0], outs[5])
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


# ------------------------------------------------------------------------------------------------------------- (f) audio prompt
def test_audio_prompt(case):
    c = case
    cfg = O.DiTConfig(**SMALL, cond_proj_in=True)
    P = O.init_params(cfg, 12)
    cond = torch.randn(2, 8, cfg.num_channels, generator=torch.Generator().manual_seed(23))
    lens, dur = torch.tensor([8, 8]), torch.tensor([T_, 30])
    kw = _kw(c, steps=4, lens=lens, duration=dur)
    m = make_model(cfg, P, "bf16x3")
    run = lambda: m.sample(cond, **kw).float().cpu()
    eng = m.engine()
    on = run()
    assert eng.plan["armed"] and eng.plan["has_cond"]
    eng.fold_embed = False
    off = run()
    assert not eng.plan["armed"]
    ref = _oracle64(c, kw, cfg, P, cond=cond.double(), lens=lens, duration=dur)
    valid = lambda a, b: max(float((a[i, :int(n)].double() - b[i, :int(n)].double()).abs().max()) for i, n in enumerate(dur))
    d_on_off, d_off, d_on = valid(on, off), valid(off, ref), valid(on, ref)
    print("fold-embed audio prompt, three steps: max |armed - unfolded| = %.3e; unfolded vs float64 %.3e, armed vs float64 %.3e" % (d_on_off, d_off, d_on))
    assert torch.isfinite(on).all() and d_on_off <= 2 * d_off
    assert torch.equal(on[:, :8], cond) and torch.equal(off[:, :8], cond)          # the prompt frames come back unchanged


# ------------------------------------------------------------------------------------------------------------- (g) fallbacks
def _counts(L, run):
    prof = L.KernelProfiler()
    L.set_profiler(prof)
    try:
        run()
    finally:
        L.set_profiler(None)
    s = prof.summary()
    n = lambda key: sum(v["launches"] for k, v in s.items() if k.startswith(key))
    return dict(linear_small=n("linear_small"), split_bf16=n("split_bf16"), cfg_euler=n("cfg_euler"))


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp32"])
def test_fallbacks_sample(L, case, mode):
    """Launch counts of an eager sample() of S = 4 evaluations.  Unfolded: linear_small = proj_frames + one embed per evaluation; split_bf16 (bf16x3
    only) = the context + one per evaluation.  Armed: embed once (at y = 0) and 2 B plane launches per begin_steps."""
    S, B = STEPS - 1, 2
    m = make_model(case["cfg"], case["P"], mode, use_graph=False)
    got = _counts(L, lambda: _sample(m, _kw(case)))
    armed = m.engine().plan["armed"]
    assert armed == (mode == "bf16x3")
    if armed:
        assert got == dict(linear_small=2, split_bf16=1 + 1 + 2 * B, cfg_euler=S), got
        m.engine().fold_embed = False
        got = _counts(L, lambda: _sample(m, _kw(case)))
        assert not m.engine().plan["armed"]
    assert got == dict(linear_small=1 + S, split_bf16=(1 + S) if mode == "bf16x3" else 0, cfg_euler=S), got


@pytest.mark.parametrize("why", ["cfg_mode=False", "per_sample_t"])
def test_fallbacks_engine(L, case, why):
    c = case
    B = 2
    eng = make_model(c["cfg"], c["P"], "bf16x3").engine()
    assert eng.fold_embed
    if why == "cfg_mode=False":
        eng.setup(B, T_, NC, B, cfg_mode=False)
    else:
        eng.setup(B, T_, NC, 2 * B, cfg_mode=True)
    p = eng.plan
    p["per_sample_t"] = True            # one grid point per sequence, as E2TTS.transformer_with_pred_head prepares its plans
    eng.prepare(c["text"], c["roll"], c["ctx"], c["cm"], torch.linspace(0.1, 0.7, p["Bt"]), fold_embed=True)
    y = eng.begin_steps(c["y0"])
    assert not p["armed"] and not p["c0_ok"]

    def run():
        eng.embed(y)
        eng.forward()
        torch.cuda.synchronize()

    got = _counts(L, run)
    p["per_sample_t"] = False
    assert got == dict(linear_small=1, split_bf16=1, cfg_euler=0), got
    assert torch.isfinite(p["pred"]).all()
