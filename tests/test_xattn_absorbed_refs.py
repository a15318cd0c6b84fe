"""The float64 restatement of the absorbed cross-attention (csrc/xattn_absorbed.hip) that tests/test_xattn_absorbed_gpu.py holds the
kernels to, checked on the CPU against oracle.e2_cfm_oracle.attention and against its own plane rounding.

Without rotary in cross-attention and with bias-free to_q / to_k / to_v / to_out, for clip b, head h and key slot j

    logits[n, h, j] = x[n, :] . Wqk[b][(h, j), :]        Wqk[(h, j), c] = sum_d K[b, j, h, d] Wq[h*64 + d, c]
    out[n, o]       = sum_{h, j} P[n, h, j] sigmoid(gate[n, h]) Wvo[b][o, (h, j)]     Wvo[o, (h, j)] = sum_d Wout[o, h*64 + d] V[b, j, h, d]

with KP = 16 / 32 key slots per head: slots nc .. KP-1 are zero rows of Wqk / zero columns of Wvo and masked like every slot at or
beyond kv_len[b]; the last H rows of Wqk are the head-gate rows.  The helpers work in float64 from whatever they are given -- exact
operands here, operands as stored (hi + lo planes) in the GPU tests."""
import math

import pytest
import torch

from oracle import e2_cfm_oracle as O


# ------------------------------------------------------------------------------------------------------------ the float64 helpers
def kp_of(nc):
    return 16 if nc <= 16 else 32


def planes(x):
    """fp32 -> (hi, lo) bf16 planes as float64: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi.double(), lo.double()


def absorbed_operands64(k, v, wq, wg, wout, KP):
    """k, v (B, nc, H*64), wq (H*64, D), wg (H, D), wout (D, H*64) -> Wqk (B, H*KP + H, D), Wvo (B, D, H*KP) in float64, key slots
    nc .. KP-1 zero."""
    B, nc, inner = k.shape
    H, D = inner // 64, wq.shape[1]
    k4, v4 = k.double().reshape(B, nc, H, 64), v.double().reshape(B, nc, H, 64)
    wqk = torch.zeros(B, H * KP + H, D, dtype=torch.float64)
    wvo = torch.zeros(B, wout.shape[0], H * KP, dtype=torch.float64)
    q = torch.einsum("bjhd,hdc->bhjc", k4, wq.double().reshape(H, 64, D))
    o = torch.einsum("ohd,bjhd->bohj", wout.double().reshape(-1, H, 64), v4)
    wqk[:, :H * KP].reshape(B, H, KP, D)[:, :, :nc] = q
    wqk[:, H * KP:] = wg.double()
    wvo.reshape(B, -1, H, KP)[..., :nc] = o
    return wqk, wvo


def gated_p64(x, wqk, *, H, KP, kv_len, q_len=None, gate_bias=None, scale=0.125, clamp=50.0, row_scale=None):
    """x (B, n, D), wqk (B, H*KP + H, D) -> P sigmoid(gate) (B, n, H*KP) in float64: logits x row_scale x scale, soft clamp, key slots
    >= kv_len[b] masked, softmax over the KP slots of a head, times sigmoid(gate logit x row_scale + bias); rows >= q_len[b] and
    clips without a key are zero."""
    B, n, _ = x.shape
    z = torch.einsum("bnc,brc->bnr", x.double(), wqk.double())
    if row_scale is not None:
        z = z * row_scale.double()[..., None]
    s = z[..., :H * KP].reshape(B, n, H, KP) * scale
    if clamp:
        s = torch.tanh(s / clamp) * clamp
    live = torch.arange(KP)[None] < torch.as_tensor(kv_len)[:, None]                 # (B, KP)
    s = s.masked_fill(~live[:, None, None, :], -math.inf)
    p = torch.nan_to_num(s.softmax(-1), nan=0.0)                                     # a clip without keys: all -inf -> 0
    g = z[..., H * KP:]
    if gate_bias is not None:
        g = g + gate_bias.double()
    p = p * torch.sigmoid(g)[..., None]
    if q_len is not None:
        p = p * (torch.arange(n)[None] < torch.as_tensor(q_len)[:, None])[..., None, None]
    return p.reshape(B, n, H * KP)


def second_product64(pg, wvo):
    return torch.einsum("bnr,bor->bno", pg.double(), wvo.double())


# ------------------------------------------------------------------------------------------------------------------------- tests
def _problem(D, H, n, nc, seed, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inner, pre = H * 64, "a"
    P = {f"{pre}.to_q.weight": r(inner, D) * (spread / math.sqrt(D)), f"{pre}.to_k.weight": r(inner, D) / math.sqrt(D),
         f"{pre}.to_v.weight": r(inner, D) / math.sqrt(D), f"{pre}.to_v_head_gate.weight": r(H, D) / math.sqrt(D),
         f"{pre}.to_v_head_gate.bias": 1.0 + r(H), f"{pre}.to_out.weight": r(D, inner) * (4.0 / math.sqrt(inner))}
    return P, pre, r(2, n, D), r(2, nc, D)


@pytest.mark.parametrize("nc,kv", [(16, (16, 5)), (5, (5, 1)), (17, (17, 9)), (32, (32, 20))])
@pytest.mark.parametrize("clamp", [50.0, 1.5, 0.0])
def test_absorbed_form_equals_the_oracle_attention(nc, kv, clamp):
    """D = 512, H = 8, n = 70, two clips with a ragged context mask and masked queries; clamp 1.5 bends logits of spread 3."""
    D, H, n = 512, 8, 70
    P, pre, x, ctx = _problem(D, H, n, nc, seed=nc)
    cm = torch.arange(nc)[None] < torch.tensor(kv)[:, None]
    q_len = (n, 33)
    mask = torch.arange(n)[None] < torch.tensor(q_len)[:, None]
    want = O.attention(P, pre, x, H, 64, None, mask, O.OracleOptions(softclamp=clamp), context=ctx, context_mask=cm)
    KP = kp_of(nc)
    k, v = ctx @ P[f"{pre}.to_k.weight"].t(), ctx @ P[f"{pre}.to_v.weight"].t()
    wqk, wvo = absorbed_operands64(k, v, P[f"{pre}.to_q.weight"], P[f"{pre}.to_v_head_gate.weight"], P[f"{pre}.to_out.weight"], KP)
    assert wqk.shape == (2, H * KP + H, D) and wvo.shape == (2, D, H * KP)
    pad = torch.arange(KP) >= nc
    assert (wqk[:, :H * KP].reshape(2, H, KP, D)[:, :, pad] == 0).all() and (wvo.reshape(2, D, H, KP)[..., pad] == 0).all()
    pg = gated_p64(x, wqk, H=H, KP=KP, kv_len=kv, q_len=q_len, gate_bias=P[f"{pre}.to_v_head_gate.bias"], scale=64 ** -0.5, clamp=clamp)
    assert (pg.reshape(2, n, H, KP)[0, :, :, kv[0]:] == 0).all() and (pg.reshape(2, n, H, KP)[1, :, :, kv[1]:] == 0).all()
    assert (pg[1, q_len[1]:] == 0).all()
    got = second_product64(pg, wvo)
    err = float((got - want).abs().max())
    print("nc=%d clamp=%g: max |absorbed - oracle| = %.2e on outputs up to %.2f" % (nc, clamp, err, float(want.abs().max())))
    assert err < 1e-12 and float(want.abs().max()) > 0.5
    if clamp == 1.5:        # the clamp must have bent something: the unclamped result differs
        free = second_product64(gated_p64(x, wqk, H=H, KP=KP, kv_len=kv, q_len=q_len, gate_bias=P[f"{pre}.to_v_head_gate.bias"],
                                          scale=64 ** -0.5, clamp=0.0), wvo)
        assert float((free - want).abs().max()) > 1e-3


def test_clip_without_keys_and_row_scale():
    D, H, n, nc = 512, 4, 9, 16
    P, pre, x, ctx = _problem(D, H, n, nc, seed=1)
    wqk, wvo = absorbed_operands64(ctx @ P[f"{pre}.to_k.weight"].t(), ctx @ P[f"{pre}.to_v.weight"].t(), P[f"{pre}.to_q.weight"],
                                   P[f"{pre}.to_v_head_gate.weight"], P[f"{pre}.to_out.weight"], 16)
    pg = gated_p64(x, wqk, H=H, KP=16, kv_len=(0, 16), scale=0.125)
    assert (pg[0] == 0).all() and torch.isfinite(pg).all() and float(pg[1].abs().max()) > 0
    rs = torch.rand(2, n, dtype=torch.float64) + 0.5
    a = gated_p64(x, wqk, H=H, KP=16, kv_len=(16, 16), scale=0.125, row_scale=rs)
    b = gated_p64(x * rs[..., None], wqk, H=H, KP=16, kv_len=(16, 16), scale=0.125)
    assert float((a - b).abs().max()) < 1e-13


def test_planes_equal_split_planes():
    from v2a_amd import _lib as L
    x = torch.randn(37, 24, generator=torch.Generator().manual_seed(0)) * torch.logspace(-6, 3, 24)
    hi, lo = planes(x)
    sp = L.split_planes(x)
    assert torch.equal(sp[:, :24].double(), hi) and torch.equal(sp[:, 24:].double(), lo)
    assert float((hi + lo - x.double()).abs().max() / x.abs().max()) < 2.0 ** -16
    assert L.xattn_kp(1) == 16 and L.xattn_kp(16) == 16 and L.xattn_kp(17) == 32 and L.xattn_kp(32) == 32 and kp_of(17) == 32
