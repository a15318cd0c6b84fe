"""The absorbed cross-attention (csrc/xattn_absorbed.hip; DiTEngine.absorb_xattn): the context K / V folded into to_q and to_out once
per sample() (v2a_xattn_absorb_prepare), an evaluation runs v2a_xattn_absorbed -- logits over KP = 16 / 32 key slots per head, soft
clamp, softmax, head gate -- and one K = H*KP out-projection per clip on the existing split GEMM.  The float64 references are the
helpers of tests/test_xattn_absorbed_refs.py, checked there on the CPU against oracle.e2_cfm_oracle.attention.

Weights and inputs follow tests/test_qproj_xattn_gpu.py: a ~ N(0, 1); K ~ N(0, 2.25), V ~ N(0, 1); to_q rows ~ N(0, 2.25 / K), gate rows
~ N(0, 1 / K), gate bias ~ N(0, 0.09) -- logits of spread 2.25 before the clamp.  The logits kernel is driven with Wqk rows drawn
directly, ~ N(0, (2.25 / scale)^2 / K): the same logit spread.

  test_prepare_vs_float64   D = 512 / H = 4 and D = 1024 / H = 16, nc = 1, 5, 16 (KP 16), 17, 32 (KP 32), two layers, two clips (the
                            second with an all-zero context), both layers checked: the column offsets into ctx_kv are exercised.
                            Bound per element: 2^-16 |value| for the planes + (64 + 4) 2^-24 sum |K| |W| for the fp32 fma chain (the
                            bound of tests/test_gemm_fp32_gpu.py); padding rows / columns == 0, gate rows == the planes of the gate weights
  test_logits_vs_float64    atol = rtol = 2e-4 (TOL of test_attention_paths_gpu.py) on hi + lo; rows_per_batch 23 / 150 / 782 over two
                            clips with different Wqk, ragged kv_len including 1, q_len < rows including 0 (exactly zero rows), folded row
                            scale on and off, logits driven to +-60 against clamps 50 (bounded weights), 80 (running maximum) and none,
                            nc = 17 with KP = 32; NaN in every key slot at or beyond kv_len[b] of the device copy of Wqk, NaN in the row
                            gaps of padded A / Wqk strides, SENTINEL in the pad columns of the output
  test_composite_vs_float64 the logits kernel followed by v2a_gemm(GATE_RESID) on split operands at device step 2 with the folded-norm
                            producer, K = H*KP = 64 / 256 / 512, against float64 at the same 2e-4
  test_engine_*             shipped widths, depth 2, T = 150, nc = 16, two ragged clips, 4-point grid, bf16x3
  test_launch_sequence_*    CPU, with the recorder of tests/test_launch_trace.py"""
import math

import pytest
import torch

from oracle import e2_cfm_oracle as O
from conftest import make_model
from test_xattn_absorbed_refs import absorbed_operands64, gated_p64, kp_of, planes, second_product64

DEV = "cuda"
NAN = float("nan")
TOL = 2e-4                  # the bar of the split attention kernels (TOL of tests/test_attention_paths_gpu.py)
SENTINEL = -777.0
SCALE = 64 ** -0.5
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _padded(L, x, pad, fill=NAN):
    """fp32 (rows, K) -> device bf16 rows [hi K | lo K | pad] with `fill` in the pad."""
    sp = L.split_planes(x)
    buf = torch.full((x.shape[0], sp.shape[1] + pad), fill, dtype=torch.bfloat16)
    buf[:, :sp.shape[1]] = sp
    return buf.to(DEV)


def _stored64(x):
    hi, lo = planes(x)
    return hi + lo


# --------------------------------------------------------------------------------------------------------------- prepare kernel
@gpu
@pytest.mark.parametrize("nc", [1, 5, 16, 17, 32])
@pytest.mark.parametrize("D,H", [(512, 4), (1024, 16)])
def test_prepare_vs_float64(L, D, H, nc):
    B, Ly, inner, KP = 2, 2, H * 64, kp_of(nc)
    g = _gen(100 * H + nc)
    kv = torch.randn(B, nc, 2 * Ly * inner, generator=g)
    kv[..., :Ly * inner] *= 1.5
    kv[1] = 0.0                                                    # a dropped context
    wq = torch.randn(Ly, inner + H, D, generator=g) / math.sqrt(D)
    wq[:, :inner] *= 1.5
    wo = torch.randn(Ly, D, inner, generator=g) / math.sqrt(inner)
    nr = H * KP + H
    wqk = torch.full((B, Ly, nr, 2 * D), NAN, dtype=torch.bfloat16, device=DEV)
    wvo = torch.full((B, Ly, D, 2 * H * KP), NAN, dtype=torch.bfloat16, device=DEV)
    L.xattn_absorb_prepare(kv.reshape(B * nc, -1).to(DEV), wq.to(DEV), wo.to(DEV), wqk, wvo, B=B, L=Ly, H=H, D=D, nc=nc, KP=KP,
                           k_col=0, v_col=Ly * inner)
    torch.cuda.synchronize()
    wqk, wvo = wqk.cpu(), wvo.cpu()
    assert torch.isfinite(wqk.float()).all() and torch.isfinite(wvo.float()).all()
    pad = torch.arange(KP) >= nc
    worst = 0.0
    for l in range(Ly):
        k, v = kv[..., l * inner:(l + 1) * inner], kv[..., (Ly + l) * inner:(Ly + l + 1) * inner]
        rq, ro = absorbed_operands64(k, v, wq[l, :inner], wq[l, inner:], wo[l], KP)
        aq, ao = absorbed_operands64(k.abs(), v.abs(), wq[l, :inner].abs(), wq[l, inner:].abs(), wo[l].abs(), KP)    # sum |K| |W|
        gq = wqk[:, l, :, :D].double() + wqk[:, l, :, D:].double()
        go = wvo[:, l, :, :H * KP].double() + wvo[:, l, :, H * KP:].double()
        for got, ref, mag in ((gq[:, :H * KP], rq[:, :H * KP], aq[:, :H * KP]), (go, ro, ao)):
            bound = 2.0 ** -16 * ref.abs() + 68 * 2.0 ** -24 * mag
            over = ((got - ref).abs() - bound).max()
            assert float(over) <= 0, (l, float(over))
            worst = max(worst, float(((got - ref).abs() / (bound + 1e-300)).max()))
        assert (wqk[:, l, :H * KP].reshape(B, H, KP, 2 * D)[:, :, pad] == 0).all()
        assert (wvo[:, l].reshape(B, D, 2, H, KP)[..., pad] == 0).all()
        assert (wqk[1, l, :H * KP] == 0).all() and (wvo[1, l] == 0).all()                   # zero context: zero operands
        want_gate = L.split_planes(wq[l, inner:])
        assert torch.equal(wqk[0, l, H * KP:], want_gate) and torch.equal(wqk[1, l, H * KP:], want_gate)
    print("prepare D=%d H=%d nc=%d: worst |err| / bound = %.3f" % (D, H, nc, worst))


# ---------------------------------------------------------------------------------------------------------------- logits kernel
def _lcase(rpb, H, K, nc, kv, ql, folded, clamp=50.0, drive=1.0, pad=0):
    return dict(rpb=rpb, H=H, K=K, nc=nc, kv=kv, ql=ql, folded=folded, clamp=clamp, drive=drive, pad=pad)


LOGIT_CASES = {
    "rows23": _lcase(23, 4, 512, 16, (16, 1), (23, 0), False),
    "rows150-folded-padded": _lcase(150, 8, 512, 16, (5, 16), (150, 77), True, pad=24),
    "rows150-nc5": _lcase(150, 4, 512, 5, (5, 3), (150, 150), False, pad=8),
    "rows782-shipped": _lcase(782, 16, 1024, 16, (16, 9), (782, 611), True),
    "nc17-kp32": _lcase(150, 4, 512, 17, (17, 3), (100, 150), True, pad=24),
    "nc32-kp32-K1536": _lcase(70, 2, 1536, 32, (32, 20), (70, 5), False),
    "drive60-clamp50": _lcase(150, 4, 512, 16, (16, 7), (150, 149), True, clamp=50.0, drive=60.0 / 6.75),
    "drive60-clamp80": _lcase(150, 4, 512, 16, (16, 7), (150, 149), False, clamp=80.0, drive=60.0 / 6.75),
    "drive60-noclamp": _lcase(150, 4, 512, 16, (16, 7), (150, 149), True, clamp=0.0, drive=60.0 / 6.75),
    "no-keys": _lcase(70, 4, 512, 16, (0, 16), (70, 70), True, clamp=80.0),
}


def _logit_problem(L, c, seed):
    """Operands of one launch and the float64 P sigmoid(gate) of the operands as stored."""
    B, rpb, H, K, nc = 2, c["rpb"], c["H"], c["K"], c["nc"]
    KP, M = kp_of(nc), 2 * c["rpb"]
    g = _gen(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(B, H * KP + H, K, generator=g) / math.sqrt(K)
    w[:, :H * KP] *= 2.25 / SCALE * c["drive"]                      # scale * logit ~ N(0, 2.25^2) x drive: 3 sigma = +-60 when driven
    w[:, :H * KP].reshape(B, H, KP, K)[:, :, nc:] = 0.0             # the padding slots as prepare leaves them
    bias = 0.3 * torch.randn(H, generator=g)
    ssq = rs = None
    if c["folded"]:
        parts = K // 32
        ssq = torch.full((M, 40 if parts <= 40 else (parts + 3) // 4 * 4), 1e30)
        ssq[:, :parts] = 64.0 * torch.rand(M, parts, generator=g)
        rs = (math.sqrt(K) / ssq[:, :parts].double().sum(1).sqrt()).reshape(B, rpb)
    ref = gated_p64(_stored64(a).reshape(B, rpb, K), _stored64(w.reshape(-1, K)).reshape(w.shape), H=H, KP=KP, kv_len=c["kv"],
                    q_len=c["ql"], gate_bias=bias, scale=SCALE, clamp=c["clamp"], row_scale=rs)
    wd = w.clone()
    for b in range(B):                                              # NaN in every key slot the kernel must not use
        wd[b, :H * KP].reshape(H, KP, K)[:, c["kv"][b]:] = NAN
    wdev = torch.stack([_padded(L, wd[b], c["pad"]) for b in range(B)])
    return dict(a=_padded(L, a, c["pad"]), w=wdev, bias=bias.to(DEV), ssq=None if ssq is None else ssq.to(DEV), ref=ref.reshape(M, H * KP),
                B=B, M=M, KP=KP)


def _run_logits(L, c, pr, out_pad=8):
    H, K, KP, M = c["H"], c["K"], pr["KP"], pr["M"]
    out = torch.full((M + 2, 2 * H * KP + out_pad), SENTINEL, dtype=torch.bfloat16, device=DEV)
    nk = dict(row_ssq=pr["ssq"], row_norm_dim=K) if pr["ssq"] is not None else {}
    L.xattn_absorbed(pr["a"], pr["a"].stride(0), K, pr["w"], out, ldw=pr["w"].stride(1), w_batch_stride=pr["w"].stride(0), ldo=out.stride(0),
                     M=M, rows_per_batch=c["rpb"], B=pr["B"], H=H, KP=KP, kv_len=torch.tensor(c["kv"], dtype=torch.int32, device=DEV),
                     q_len=torch.tensor(c["ql"], dtype=torch.int32, device=DEV), gate_bias=pr["bias"], scale=SCALE, softclamp=c["clamp"], **nk)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("name", list(LOGIT_CASES))
def test_logits_vs_float64(L, name):
    c = LOGIT_CASES[name]
    pr = _logit_problem(L, c, seed=len(name) + c["rpb"])
    out = _run_logits(L, c, pr).cpu()
    H, KP, M, rpb = c["H"], pr["KP"], pr["M"], c["rpb"]
    hk = H * KP
    assert (out[M:] == SENTINEL).all() and (out[:, 2 * hk:] == SENTINEL).all(), "wrote outside its rows / columns"
    live = out[:M, :2 * hk].float()
    assert torch.isfinite(live).all()
    got, ref = live[:, :hk].double() + live[:, hk:].double(), pr["ref"]
    err = (got - ref).abs()
    print("%s: max |got - ref| = %.2e, max |ref| = %.3f" % (name, float(err.max()), float(ref.abs().max())))
    assert bool((err <= TOL + TOL * ref.abs()).all()), float(err.max())
    assert float(ref.abs().max()) > 0.05
    for b in range(2):
        rows = live[b * rpb:(b + 1) * rpb]
        assert (rows[c["ql"][b]:] == 0).all(), "rows at or beyond q_len must be exactly zero"
        assert (rows.reshape(rpb, 2, H, KP)[..., c["kv"][b]:] == 0).all(), "masked key slots must be exactly zero"
    # the planes are a split of one fp32 value: |lo| <= ulp_bf16(hi) / 2, lo == 0 where hi == 0
    hi, lo = live[:, :hk], live[:, hk:]
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -8).all()) and bool((lo[hi == 0] == 0).all())
    if c["drive"] > 1 and c["clamp"]:           # the clamp bent something: the unclamped reference is elsewhere
        assert c["clamp"] * math.tanh(60.0 / c["clamp"]) < 59.0


# ------------------------------------------------------------------------------------------------------------------- composite
@gpu
@pytest.mark.parametrize("H,nc", [(4, 16), (16, 16), (16, 32)], ids=["K64", "K256", "K512"])
def test_composite_vs_float64(L, H, nc):
    """v2a_xattn_absorbed -> v2a_gemm(GATE_RESID, split operands, step 2 of 4, folded-norm producer) of one clip against float64."""
    D, rpb, S, step = 512, 150, 4, 2
    KP = kp_of(nc)
    hk = H * KP
    c = _lcase(rpb, H, D, nc, (nc, max(1, nc - 7)), (rpb, 97), True)
    pr = _logit_problem(L, c, seed=7 * H + nc)
    g = _gen(H + nc)
    wvo = torch.randn(2, D, hk, generator=g) * (4.0 / math.sqrt(hk))          # outputs of a few units, as to_out x V gives
    wvo.reshape(2, D, H, KP)[..., nc:] = 0.0
    gate = torch.randn(S, D, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(S, D, generator=g)
    resid = torch.randn(2 * rpb, D, generator=g)
    xp = _run_logits(L, c, pr, out_pad=0)
    x = resid.clone().to(DEV)
    shadow = torch.zeros(2 * rpb, 2 * D, dtype=torch.bfloat16, device=DEV)
    ssq = torch.zeros(2 * rpb, D // 32, device=DEV)
    stp = torch.full((1,), step, dtype=torch.int32, device=DEV)
    gd, gm = gate.to(DEV), gamma.to(DEV)
    for b in range(2):
        r = slice(b * rpb, (b + 1) * rpb)
        L.gemm([L.Operand(xp[r], xp.stride(0), hk)], L.split_planes(wvo[b]).to(DEV), x[r], M=rpb, N=D, compute=L.BF16, a_split=True,
               epilogue=L.EPI_GATE_RESID, resid=x[r], ldo=D, ldr=D, gate=gd, step=stp, gate_step_stride=D, rows_per_batch=rpb,
               norm_gamma=gm, norm_step_stride=D, norm_ssq=ssq[r], out_bf16=shadow[r], ld_out_bf16=2 * D, out_bf16_split=True)
    torch.cuda.synchronize()
    ref = resid.double() + gate[step].double() * second_product64(pr["ref"].reshape(2, rpb, hk), _stored64(wvo.reshape(-1, hk)).reshape(wvo.shape)).reshape(-1, D)
    got = x.cpu().double()
    delta = (got - resid.double()).abs()
    err = (got - ref).abs()
    print("composite K=%d: max |got - ref| = %.2e, attention part up to %.2f" % (hk, float(err.max()), float(delta.max())))
    assert bool((err <= TOL + TOL * ref.abs()).all()), float(err.max())
    assert float(delta.max()) > 1.0 and bool((got[rpb + 97:] == resid[rpb + 97:].double()).all())
    sh = shadow.cpu().float()
    want_sh = ref * gamma[step].double()
    assert bool(((sh[:, :D].double() + sh[:, D:].double() - want_sh).abs() <= 2 * TOL + 2 * TOL * want_sh.abs()).all())
    want_ssq = (ref ** 2).reshape(-1, D // 32, 32).sum(-1)
    assert bool(((ssq.cpu().double() - want_ssq).abs() <= 1e-3 * want_ssq + 1e-6).all())


# ---------------------------------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def eng_case():
    cfg = O.DiTConfig(depth=2)
    P = O.init_params(cfg, 0)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 150, nc=16, seed=5)
    cm = cm.clone()
    cm[1, 9:] = False
    dur = torch.tensor([150, 117])
    want = O.sample(P, cfg, y0, text, roll, ctx, cm, duration=dur, steps=4, cfg_strength=2.0, remove_parallel_component=False)
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, return_raw_output=True, steps=4, cfg_strength=2.0,
              remove_parallel_component=False, lens=dur, duration=dur)
    return dict(cfg=cfg, P=P, kw=kw, want=want, dur=dur)


def _run(m, kw, **over):
    k = dict(kw)
    k.update(over)
    return m.sample(torch.zeros(k["y0"].shape[0], k["y0"].shape[1], 128), **k).float().cpu()


def _valid_err(a, b, dur):
    return max(float((a[i, :int(d)] - b[i, :int(d)]).abs().max()) for i, d in enumerate(dur))


@gpu
def test_engine_absorbed_vs_oracle_and_unabsorbed(eng_case):
    e = eng_case
    m = make_model(e["cfg"], e["P"], "bf16x3")
    eng = m.engine()
    assert eng.absorb_xattn
    on = _run(m, e["kw"])
    assert eng.plan["xattn_kp"] == 16 and "wqk" in eng.plan
    eng.absorb_xattn = False
    off = _run(m, e["kw"])
    eng.fuse_xattn = False
    off2 = _run(m, e["kw"])
    eng.fuse_xattn, eng.absorb_xattn = True, True
    err_on, err_off = _valid_err(on, e["want"], e["dur"]), _valid_err(off, e["want"], e["dur"])
    print("engine depth 2, T=150, nc=16, two ragged clips, 4 points: absorbed vs oracle %.3e, unabsorbed vs oracle %.3e, on vs off max |delta| = %.3e"
          % (err_on, err_off, float((on - off).abs().max())))
    assert torch.isfinite(on).all() and err_on < 1e-3
    # absorption off: the one- and two-launch forms of the unabsorbed path are the same arithmetic
    assert torch.equal(off, off2), float((off - off2).abs().max())
    assert not torch.equal(on, off)


@gpu
def test_engine_second_context_equals_fresh_model_and_graph_equals_eager(eng_case):
    e = eng_case
    _, _, _, ctx2, _ = O.synthetic_inputs(e["cfg"], 2, 150, nc=16, seed=11)
    m = make_model(e["cfg"], e["P"], "bf16x3")
    first = _run(m, e["kw"])
    second = _run(m, e["kw"], context=ctx2)                       # same plan, same graph: the absorbed operands are re-armed
    fresh = make_model(e["cfg"], e["P"], "bf16x3")
    assert torch.equal(second, _run(fresh, e["kw"], context=ctx2))
    assert not torch.equal(first, second)
    eager = make_model(e["cfg"], e["P"], "bf16x3", use_graph=False)
    assert torch.equal(first, _run(eager, e["kw"]))


# ------------------------------------------------------------------------------------------------------------- launch sequence
def _trace(mode, B, nc, T=150, **kw):
    import test_launch_trace as LT
    return LT._dit_case(LT.SHIPPED, mode, B, T=T, nc=nc, **kw)()


def _names(calls):
    return [c["fn"] for c in calls]


@pytest.mark.parametrize("B", [1, 2])
def test_launch_sequence_absorbed(B):
    calls = _trace("bf16x3", B, 16)
    names = _names(calls)
    depth = 4
    assert names.count("v2a_xattn_absorb_prepare") == 1 and names.count("v2a_xattn_absorbed") == depth and "v2a_qproj_xattn" not in names
    k256 = [c for c in calls if c["fn"] == "v2a_gemm" and c["args"][0]["nseg"] == 1 and c["args"][0]["ka"][0] == 256]
    assert len(k256) == depth * B and all(c["args"][0]["epilogue"] == 4 and c["args"][0]["M"] == 182 for c in k256)
    # per layer: the logits launch, then the B out-projections of the clips, back to back
    for i, n in enumerate(names):
        if n == "v2a_xattn_absorbed":
            assert calls[i]["prof"][0] == "xattn_absorbed<bf16x3>" and not calls[i]["prof"][0].startswith("gemm")
            assert all(c in k256 for c in calls[i + 1:i + 1 + B])
    off = _names(_trace("bf16x3", B, 16, attrs=dict(absorb_xattn=False)))
    assert len(names) == len(off) + 1 + depth * (B - 1)            # + prepare; qproj_xattn -> absorbed; one out-projection -> B


@pytest.mark.parametrize("why,mode,B,nc,kw", [
    ("nc33", "bf16x3", 1, 33, {}),
    ("rope_cross", "bf16x3", 1, 16, dict(ctor=dict(rope_cross=True))),
    ("four-clips", "bf16x3", 4, 16, dict(T=778)),         # 4 x 13 x 16 = 832 workgroups of the one-launch form: beyond the 704 rule
    ("bf16", "bf16", 1, 16, {}),
    ("fp32", "fp32", 1, 16, {}),
])
def test_launch_sequence_unchanged_where_not_absorbed(why, mode, B, nc, kw):
    """Outside its conditions the switch changes nothing: the trace with absorb_xattn on equals the trace with it off, which is the
    code path of before (the pinned traces of tests/test_launch_trace.py hold that one in place)."""
    on = _trace(mode, B, nc, **kw)
    off = _trace(mode, B, nc, attrs=dict(absorb_xattn=False), **kw)
    assert on == off and not any(n.startswith("v2a_xattn") for n in _names(on))
