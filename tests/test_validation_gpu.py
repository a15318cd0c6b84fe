"""GPU: `E2TTS.forward(val=True)`, the reference's validation pass (x3:2307-2588), and the three kernels of csrc/cfm_loss.hip.

Kernels: v2a_cfm_interp against torch's CPU fp32 ops bit for bit; v2a_masked_sqerr and v2a_roll_metrics against float64 torch on the
same fp32 inputs -- sums within 1e-9 relative (only the order of a double sum of at most 1e6 terms differs: ~1e-10), counts exact,
two runs identical bits.
End to end: against float64 -- the oracle's transformer_with_pred_head plus plain torch for the losses.  |pred - pred64| < tau with
tau = 1e-4 in fp32 mode (the bound tests/test_sampler_gpu.py holds one evaluation to) and, in bf16x3 mode, twice what
`transformer_with_pred_head` of the commit before this feature measures on these inputs (profiles/validation_forward.txt); the loss
within 2 tau sqrt(loss64) + tau^2 (Cauchy-Schwarz on a mean of squares under a perturbation of at most tau)."""
import dataclasses

import pytest
import torch

import v2a_amd
from v2a_amd import _lib as L
from oracle import e2_cfm_oracle as O
from conftest import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, LENS, TIMES = 3, 40, [40, 33, 21], [0.1, 0.37, 0.8]          # shared with tests/test_validation_host.py
BF = 2                                                              # frames for the last two clips only
# bf16x3: 2 x 3.849e-05, the larger max |pred - pred64| that transformer_with_pred_head measures on the inputs of the two cases
# (profiles/validation_forward.txt: 3.849e-05 `plain`, 3.647e-05 `cond`); the factor covers the launch-to-launch tile choice
TAU = {"fp32": 1e-4, "bf16x3": 2 * 3.849e-05}


# ---- kernels -------------------------------------------------------------------------------------------------------------
def _prefix_mask(b, t, empty_last=True):
    lens = torch.tensor([t, max(1, (2 * t) // 3), 0 if empty_last else max(1, t // 2)][:b])
    return torch.arange(t)[None, :] < lens[:, None]


@pytest.mark.parametrize("b,t,c", [(3, 1, 16), (3, 40, 16), (3, 40, 128), (3, 1564, 16), (2, 1564, 128)])
def test_cfm_interp_equals_torch_fp32_bit_for_bit(b, t, c):
    g = torch.Generator().manual_seed(t + c)
    x0, x1, tt = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g), torch.rand(b, generator=g)
    span = v2a_amd.val_span_mask(torch.tensor([t, max(1, (2 * t) // 3), max(1, t // 2)][:b]), t)
    tb = tt[:, None, None]
    w_ref, flow_ref = (1. - tb) * x0 + tb * x1, x1 - x0                  # x3:2394-2396, torch CPU fp32
    cond_ref = torch.where(span[..., None], torch.zeros_like(x1), x1)      # x3:2403-2407
    d = lambda v: v.to(DEV)
    w, flow, cond = (torch.full((b, t, c), float("nan"), device=DEV) for _ in range(3))
    L.cfm_interp(d(x0), d(x1), d(tt), d(span.to(torch.uint8)), w, flow, cond)
    assert torch.equal(w.cpu(), w_ref) and torch.equal(flow.cpu(), flow_ref) and torch.equal(cond.cpu(), cond_ref)
    # span = NULL: cond is x1; cond = NULL: only w and flow are written
    w2, flow2, cond2 = (torch.full((b, t, c), float("nan"), device=DEV) for _ in range(3))
    L.cfm_interp(d(x0), d(x1), d(tt), None, w2, flow2, cond2)
    assert torch.equal(w2.cpu(), w_ref) and torch.equal(flow2.cpu(), flow_ref) and torch.equal(cond2.cpu(), x1)
    w3, flow3 = (torch.full((b, t, c), float("nan"), device=DEV) for _ in range(2))
    L.cfm_interp(d(x0), d(x1), d(tt), d(span.to(torch.uint8)), w3, flow3, None)
    assert torch.equal(w3.cpu(), w_ref) and torch.equal(flow3.cpu(), flow_ref)


@pytest.mark.parametrize("t", [1, 40, 1564])
@pytest.mark.parametrize("c", [16, 128])
def test_masked_sqerr_against_float64(t, c):
    b = 3
    g = torch.Generator().manual_seed(7 * t + c)
    pred, target = torch.randn(b, t, c, generator=g), torch.randn(b, t, c, generator=g)
    # a span inside the first clip, a prefix of the second, nothing of the third
    mask = torch.stack([v2a_amd.val_span_mask(torch.tensor([t]), t)[0], _prefix_mask(3, t)[1], torch.zeros(t, dtype=torch.bool)])
    if t == 1:
        mask[0, 0] = True
    want_sum = ((pred.double() - target.double()) ** 2)[mask].sum()
    want_cnt = int(mask.sum()) * c
    outs = []
    for _ in range(2):
        out = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
        L.masked_sqerr(pred.to(DEV), target.to(DEV), mask.to(DEV, torch.uint8), out)
        outs.append(out.cpu())
    rel = abs(float(outs[0][0]) - float(want_sum)) / float(want_sum)
    print(f"masked_sqerr T={t} C={c}: sum {float(outs[0][0]):.12e} vs float64 {float(want_sum):.12e}, rel {rel:.2e}, count {int(outs[0][1])}")
    assert rel < 1e-9 and float(outs[0][1]) == want_cnt
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))                     # identical bits
    # an empty mask altogether: sum 0 over 0 elements (the caller's 0 / 0 is torch's mean of nothing)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    L.masked_sqerr(pred.to(DEV), target.to(DEV), torch.zeros(b, t, dtype=torch.uint8, device=DEV), out)
    assert out.cpu().tolist() == [0.0, 0.0]


def _pooled(x, t):
    b, _, f = x.shape
    return x[:, :(t // 3) * 3].reshape(b, t // 3, 3, f).mean(dim=2)        # x3:2437-2438


def _away_from(x, t, thr):
    """Nudges the frame triples of x whose 3-frame mean lies within 2e-3 of thr by 0.01: afterwards every mean is >= 1e-3 away, so
    an fp32 mean cannot fall on the other side of the threshold than the float64 one."""
    if t < 3:
        return x
    near = ((_pooled(x.double(), t) - thr).abs() < 2e-3).repeat_interleave(3, dim=1)
    x[:, :(t // 3) * 3] += 0.01 * near
    assert float((_pooled(x.double(), t) - thr).abs().min()) >= 1e-3
    return x


def roll_stats64(roll, midis, mask):
    """x3:2429-2443 in float64 on fp32 inputs: (weighted square sum, count, tp, fp, fn, tn); mask (b, t) bool of the same clips."""
    r, m = roll.double(), midis.double()
    per = ((r - m) ** 2 * (m - 0.10).abs())[mask]
    b, t, f = r.shape
    if t < 3:
        return [float(per.sum()), per.numel(), 0, 0, 0, 0]
    rt, mt = _pooled(r, t), _pooled(m, t)
    ok = mask[:, :(t // 3) * 3].reshape(b, t // 3, 3).to(torch.float32).mean(dim=2) >= 0.99
    cnt = lambda c: int(c[ok].sum())
    return [float(per.sum()), per.numel(), cnt((rt >= 0.4) & (mt >= 0.5)), cnt((rt >= 0.4) & (mt < 0.5)),
            cnt((rt < 0.4) & (mt >= 0.5)), cnt((rt < 0.4) & (mt < 0.5))]


@pytest.mark.parametrize("t", [1, 40, 1564])
def test_roll_metrics_against_float64(t):
    b, notes = 3, v2a_amd.NOTES
    g = torch.Generator().manual_seed(11 * t)
    roll = _away_from(torch.rand(b, t, notes, generator=g), t, 0.4)
    midis = _away_from((torch.rand(b, t, notes, generator=g) > 0.6).float() * torch.rand(b, t, notes, generator=g).clamp(min=0.3), t, 0.5)
    mask = _prefix_mask(b, t)                                               # full, two thirds (not a multiple of 3 at T = 40), empty
    want = roll_stats64(roll, midis, mask)
    outs = []
    for _ in range(2):
        out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
        L.roll_metrics(roll.to(DEV), midis.to(DEV), mask.to(DEV, torch.uint8), out)
        outs.append(out.cpu())
    got = outs[0].tolist()
    rel = abs(got[0] - want[0]) / want[0]
    print(f"roll_metrics T={t}: sum {got[0]:.12e} vs float64 {want[0]:.12e}, rel {rel:.2e}, count / tp / fp / fn / tn {got[1:]} vs {want[1:]}")
    assert rel < 1e-9 and got[1:] == [float(v) for v in want[1:]]
    if t >= 40:
        assert min(want[2:]) > 0                                            # all four cells of the confusion matrix are exercised
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def build_cases(small):
    """Inputs and parameters of the two configurations: `plain` is the shipped one (audiocond_drop_prob > 1: no audio condition),
    `cond` has cond_proj_in and conditions on the frames outside the span.  `ref` collects the float64 references, computed once."""
    from v2a_amd.synth import random_video2roll_state_dict, synthetic_piano_frames
    g = torch.Generator().manual_seed(2024)
    out = {}
    lens, times = torch.tensor(LENS), torch.tensor(TIMES)
    mask, span = O.lens_to_mask(lens, N), v2a_amd.val_span_mask(lens, N)
    vsd = random_video2roll_state_dict(5)
    frames = synthetic_piano_frames(BF, N // 3 + 1, seed=6)
    midis = (torch.rand(BF, N // 3 + 1, v2a_amd.NOTES, generator=g) > 0.6).float().repeat_interleave(3, dim=1)[:, :N].contiguous()
    for name in ("plain", "cond"):
        cfg = dataclasses.replace(small["cfg"], cond_proj_in=name == "cond")
        P = dict(O.init_params(cfg, small["meta"]["param_seed"]))
        P.update({"video2roll_net." + k: v for k, v in vsd.items()})
        _, text, _, ctx, cm = O.synthetic_inputs(cfg, B, N, nc=5, seed=31, piano=True)
        x1, x0 = torch.randn(B, N, cfg.num_channels, generator=g), torch.randn(B, N, cfg.num_channels, generator=g)
        out[name] = dict(cfg=cfg, P=P, text=text, ctx=ctx, cm=cm, x1=x1, x0=x0, lens=lens, times=times, mask=mask, span=span,
                         frames=frames, midis=midis, ref={})
    return out


@pytest.fixture(scope="module")
def cases(small):
    return build_cases(small)


def _model(c, mode):
    return make_model(c["cfg"], c["P"], mode, audiocond_drop_prob=0.3 if c["cfg"].cond_proj_in else 1.1)


def _reference64(c, roll):
    """forward(val=True) in float64 from the same x0, x1, times and the roll the engine's own frame encoder produced."""
    key = roll.numpy().tobytes()
    if key not in c["ref"]:
        P64 = {k: v.double() for k, v in c["P"].items() if not k.startswith("video2roll_net.")}
        t = c["times"].double()[:, None, None]
        x0, x1 = c["x0"].double(), c["x1"].double()
        w, flow = (1. - t) * x0 + t * x1, x1 - x0
        cond = torch.where(c["span"][..., None], torch.zeros_like(x1), x1) if c["cfg"].cond_proj_in else None
        with torch.no_grad():
            pred = O.transformer_with_pred_head(P64, c["cfg"], w, c["times"].double(), c["mask"], c["text"].double(), roll.double(), c["ctx"].double(),
                                                c["cm"], drop_text_cond=False, drop_text_prompt=False, cond=cond)
        c["ref"][key] = dict(pred=pred, w=w, cond=cond, loss=float(((pred - flow) ** 2)[c["span"]].mean()))
    return c["ref"][key]


@pytest.mark.parametrize("case", ["plain", "cond"])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_forward_val_against_float64(cases, mode, case):
    c, tau = cases[case], TAU[mode]
    m = _model(c, mode)
    r = m.forward(c["x1"], text=c["text"], times=c["times"], lens=c["lens"], val=True, frames=c["frames"], midis=c["midis"], x0=c["x0"],
                  context=c["ctx"], context_mask=c["cm"])
    assert isinstance(r, v2a_amd.E2TTSReturn) and isinstance(r.loss_breakdown, v2a_amd.LossBreakdown)
    roll_tail = m.encode_frames(c["frames"], N).cpu()                     # the engine's own frame encoder, again: the losses' input
    roll = torch.cat([torch.zeros(B - BF, N, v2a_amd.NOTES), roll_tail])    # x3:2469-2470
    ref = _reference64(c, roll)
    err = float((r.pred_flow.double() - ref["pred"]).abs().max())
    stats = m.val_stats
    lerr, lbound = abs(stats["flow"] - ref["loss"]), 2 * tau * ref["loss"] ** 0.5 + tau ** 2
    print(f"forward(val=True) [{mode}, {case}]: max |pred - pred64| = {err:.3e} (tau {tau:.1e}); flow loss {stats['flow']:.9f} vs float64 "
          f"{ref['loss']:.9f}: {lerr:.2e} (bound {lbound:.2e})")
    assert err < tau
    assert lerr <= lbound
    # what goes into and comes back from the DiT besides pred
    returned = ref["cond"] if case == "cond" else ref["w"]                 # x3:2588: cond when there is one, else w
    assert float((r.cond.double() - returned).abs().max()) < 1e-6
    assert torch.equal(r.pred_data, c["x0"] + r.pred_flow)
    if case == "cond":
        assert bool((r.cond[c["span"]] == 0).all()) and torch.equal(r.cond[~c["span"]], c["x1"][~c["span"]])
    # roll loss and metrics: kernel against float64 torch on the engine's own roll
    want = roll_stats64(roll_tail, c["midis"], c["mask"][B - BF:])
    pooled = _pooled(roll_tail.double(), N)
    assert float((pooled - 0.4).abs().min()) > 1e-6, "a pooled roll value sits on the threshold: an fp32 mean may fall on either side"
    assert [stats[k] for k in ("tp", "fp", "fn", "tn")] == [float(v) for v in want[2:]]
    roll_loss = want[0] / want[1]
    assert abs(stats["roll"] - roll_loss) <= 1e-9 * roll_loss
    tp, fp, fn = want[2:5]
    div = lambda a, b: a / b if b != 0 else 0.0
    metrics = [div(tp, tp + fp), div(tp, tp + fn), div(2 * tp, 2 * tp + fp + fn), div(tp, tp + fp + fn)]          # x3:2445-2448
    print(f"  roll loss {stats['roll']:.9f} vs float64 {roll_loss:.9f}; tp fp fn tn {want[2:]}; precision recall f1 acc {metrics}")
    for got, w_ in zip(r.loss_breakdown, metrics):
        assert abs(float(got) - w_) <= 1e-7                                # returned as fp32 scalars, as the reference's
    total = ref["loss"] + 10.0 * roll_loss                                  # x3:2574-2577
    assert abs(float(r.loss) - total) <= lbound + 1e-6 * total
    assert r.loss.dtype == torch.float32 and r.loss.device == c["x1"].device and r.pred_flow.shape == (B, N, c["cfg"].num_channels)


def test_forward_val_without_frames(cases):
    """frames=None: roll and midis are zero, so the roll loss and the four metrics are 0 (x3:2418-2420); the default noise comes from a
    generator seeded 0 on the model's device and leaves the global RNG alone; the module call is forward."""
    c = cases["plain"]
    m = _model(c, "fp32")
    kw = dict(text=c["text"], times=0.5, lens=c["lens"], val=True, context=c["ctx"], context_mask=c["cm"])
    state = torch.get_rng_state()
    r = m(c["x1"], **kw)
    assert torch.equal(torch.get_rng_state(), state)
    assert [float(v) for v in r.loss_breakdown] == [0.0] * 4 and m.val_stats["roll"] == 0.0
    assert float(r.loss) == pytest.approx(m.val_stats["flow"], rel=1e-6) and float(r.loss) > 0
    x0 = torch.randn(B, N, c["cfg"].num_channels, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)).cpu()
    ref = _reference64(dict(c, x0=x0, times=torch.full((B,), 0.5), ref={}), torch.zeros(B, N, v2a_amd.NOTES))
    assert float((r.pred_flow.double() - ref["pred"]).abs().max()) < TAU["fp32"]
    assert abs(m.val_stats["flow"] - ref["loss"]) <= 2 * TAU["fp32"] * ref["loss"] ** 0.5 + TAU["fp32"] ** 2
    r2 = m.forward(c["x1"], **kw)
    assert torch.equal(r2.pred_data, r.pred_data) and torch.equal(r2.loss, r.loss)


def test_cli_validate(tmp_path, cases, capsys):
    """CLI --validate --piano on a small checkpoint: ground-truth latents, cached CLIP features, T5 contexts, piano frames and MIDI
    rolls next to the videos -> one JSON line per batch, equal to forward(val=True) called by hand on the first batch."""
    import json
    import numpy as np
    from v2a_amd import cli
    c = cases["plain"]
    cfg = c["cfg"]
    ck = tmp_path / "small.pt"
    torch.save({"model_state_dict": c["P"]}, ck)
    vids = [str(tmp_path / f"clip{i}.mp4") for i in range(3)]
    (tmp_path / "list.scp").write_text("".join(f"{v}\tsound {i}\n" for i, v in enumerate(vids)))
    g = torch.Generator().manual_seed(5)
    rows = [37, 30, 37]                                                   # ground-truth latents: no longer than their clips (37, 38, 38 frames)
    for i, v in enumerate(vids):
        v2a_amd.save_clip_cache(v2a_amd.feature_cache_path(v), torch.randn(13 + i, cfg.dim_text, generator=g), 0.5 + 0.01 * i)
        np.savez(v.replace(".mp4", ".t5.npz"), (0.2 * torch.randn(4 + i, cfg.dim, generator=g)).numpy())
        np.save(v.replace(".mp4", ".latent.npy"), torch.randn(rows[i], cfg.num_channels, generator=g).numpy())
        v2a_amd.save_piano_frames_cache(v2a_amd.piano_frames_cache_path(v), torch.rand(12, 100, 900, 1, generator=g), 0.5 + 0.01 * i)
        np.save(v.replace(".mp4", ".3.npy"), (torch.rand(35 + 3 * i, 88, generator=g) > 0.6).double().numpy())
    mc = dict(dim=cfg.dim, dim_text=cfg.dim_text, dim_frames=cfg.dim_frames, depth=cfg.depth, heads=cfg.heads, dim_head=cfg.dim_head,
              frames_heads=cfg.frames_heads, num_registers=cfg.num_registers, max_seq_len=cfg.max_seq_len, num_channels=cfg.num_channels)
    written = cli.main([str(ck), "0", str(tmp_path / "list.scp"), "0", "3", str(tmp_path / "out"), "--batch", "2", "--frames", "40",
                        "--dtype", "fp32", "--model-config", json.dumps(mc), "--validate", "--piano"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert written == [] and [ln["batch"] for ln in lines] == [0, 1] and [ln["clips"] for ln in lines] == [2, 1]
    assert all(set(ln) == {"batch", "clips", "loss", "roll_loss", "precision", "recall", "f1", "acc"} for ln in lines)
    # the first batch by hand
    reqs = cli.build_requests(cli.read_scp(str(tmp_path / "list.scp"), 0, 2), False, 40)
    _, extras = v2a_amd.collate_clips(reqs, cfg.num_channels)
    n = extras["text_embed"].shape[1]
    lat = [torch.from_numpy(np.load(v.replace(".mp4", ".latent.npy"))) for v in vids[:2]]
    inp = torch.stack([torch.nn.functional.pad(x, (0, 0, 0, n - x.shape[0])) for x in lat])
    m = _model(c, "fp32")
    r = m.forward(inp, times=0.5, lens=torch.tensor(rows[:2]), val=True, frames=v2a_amd.load_piano_frames(vids[:2], n),
                  midis=v2a_amd.load_midi_ground_truth(vids[:2], n), text_embed=extras["text_embed"], context=extras["context"],
                  context_mask=extras["context_mask"])
    assert lines[0]["loss"] == float(r.loss) and lines[0]["roll_loss"] == m.val_stats["roll"] > 0
    assert [lines[0][k] for k in ("precision", "recall", "f1", "acc")] == [float(v) for v in r.loss_breakdown]
