"""CPU: the float64 reference of tests/test_qproj_xattn_gpu.py (qx_qgate64, qx_ref64) against torch and against the definitions of its
options one at a time, its case tables, and the condition its inputs must meet -- a wrong helper would either fail every GPU case or, worse,
agree with a kernel that is wrong in the same way."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_qproj_xattn_gpu as X


def _g(seed):
    return torch.Generator().manual_seed(seed)


B, H, NQ, NK, K = 2, 3, 37, 11, 96
INNER = H * 64


def _ops(seed=1):
    g = _g(seed)
    a = torch.randn(B * NQ, K, generator=g).double()
    w = torch.randn(INNER + 16, K, generator=g).double() / math.sqrt(K)       # 13 rows behind the gates that nothing may read
    k = torch.randn(B, NK, INNER, generator=g).double()
    v = torch.randn(B, NK, INNER, generator=g).double()
    return a, w, k, v


def _heads(t, n):
    return t.reshape(B, n, H, 64).permute(0, 2, 1, 3)


def test_plain_reference_is_torch_sdpa_times_sigmoid_gate():
    a, w, k, v = _ops()
    got = X.qx_ref64(a, w, k, v, B=B, H=H, Nq=NQ)
    z = a @ w.t()
    o = F.scaled_dot_product_attention(_heads(z[:, :INNER], NQ), _heads(k, NK), _heads(v, NK))      # default scale 1 / sqrt(64) = SCALE
    gate = z[:, INNER:INNER + H].reshape(B, NQ, H).permute(0, 2, 1)                                 # (B, H, Nq): row INNER + h of w is head h's gate
    want = (o * torch.sigmoid(gate)[..., None]).permute(0, 2, 1, 3).reshape(B, NQ, INNER)
    assert X.SCALE == 64 ** -0.5
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # the rows of w behind the H gate rows do not enter
    w2 = w.clone()
    w2[INNER + H:] = 1e9
    assert torch.equal(X.qx_ref64(a, w2, k, v, B=B, H=H, Nq=NQ), got)


def test_row_scale_is_rms_norm_of_the_row():
    a, w, _, _ = _ops(2)
    a = a * (torch.rand(B * NQ, 1, generator=_g(3)).double() * 3 + 0.2)         # rows of different rms
    parts = K // 32
    ssq = torch.full((B * NQ, 40), 1e30, dtype=torch.float64)                   # behind `parts`: never summed
    ssq[:, :parts] = a.reshape(-1, parts, 32).square().sum(-1)
    got = X.qx_qgate64(a, w, H=H, Nq=NQ, row_ssq=ssq, row_norm_dim=K)
    want = F.rms_norm(a, (K,), eps=0.0) @ w[:INNER + H].t()                      # the gate columns are scaled too
    assert got.shape == (B * NQ, INNER + H)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # scale before bias: the bias is not normalised
    bias = torch.randn(INNER + 16, generator=_g(4)).double()
    torch.testing.assert_close(X.qx_qgate64(a, w, H=H, Nq=NQ, row_ssq=ssq, row_norm_dim=K, bias=bias), want + bias[:INNER + H], rtol=1e-12, atol=1e-12)
    # a row of zero sums: the 1e-12 floor, not a division by zero
    z0 = X.qx_qgate64(a[:1], w, H=H, Nq=1, row_ssq=torch.zeros(1, 40), row_norm_dim=K)
    torch.testing.assert_close(z0, (a[:1] @ w[:INNER + H].t()) * math.sqrt(K) / 1e-12, rtol=1e-12, atol=0)


@pytest.mark.parametrize("rope_cols,off", [(INNER, 0), (INNER, 5), (64, 7)])
def test_rope_is_a_complex_rotation_at_offset_plus_row_in_clip(rope_cols, off):
    a, w, _, _ = _ops(5)
    bias = torch.randn(INNER + 16, generator=_g(6)).double()
    tab = X._rope_table(off + NQ)
    z = X.qx_qgate64(a, w, H=H, Nq=NQ, bias=bias)
    got = X.qx_qgate64(a, w, H=H, Nq=NQ, bias=bias, rope_table=tab, rope_cols=rope_cols, rope_pos_offset=off)
    assert torch.equal(got[:, rope_cols:], z[:, rope_cols:])                     # heads behind rope_cols and the gates pass through
    ang = torch.arange(off + NQ).double()[:, None] / 10000 ** (torch.arange(0, 64, 2).double() / 64)
    torch.testing.assert_close(tab.double(), torch.stack((ang.cos(), ang.sin()), -1), rtol=0, atol=2e-6)
    rot = torch.view_as_complex(tab.double())
    pos = torch.tensor([off + m % NQ for m in range(B * NQ)])                    # rotated after the bias, at the position inside the clip
    zc = torch.view_as_complex(z[:, :rope_cols].reshape(B * NQ, rope_cols // 64, 32, 2).contiguous())
    want = torch.view_as_real(zc * rot[pos][:, None, :]).reshape(B * NQ, rope_cols)
    torch.testing.assert_close(got[:, :rope_cols], want, rtol=0, atol=1e-13)
    assert int(pos[NQ]) == off and int(pos.max()) == off + NQ - 1
    if off:
        assert not torch.allclose(got[:, :64], X.qx_qgate64(a, w, H=H, Nq=NQ, bias=bias, rope_table=tab, rope_cols=rope_cols)[:, :64])


def test_bf16_storage_point_rounds_q_and_gate_to_nearest():
    a, w, _, _ = _ops(7)
    z = X.qx_qgate64(a * 3, w, H=H, Nq=NQ)
    zr = X.qx_qgate64(a * 3, w, H=H, Nq=NQ, round_bf16=True)
    assert torch.equal(zr.bfloat16().double(), zr)                               # representable, gate columns included
    assert bool(((zr - z).abs() <= X._ulp_bf16(z) / 2 * (1 + 2.0 ** -15)).all())  # (2^-15: the rounding goes through fp32, as the kernel's does)
    assert float((zr - z).abs().max()) > 0
    # the helper's ulp: 2^-7 at 1, 2^-8 just below, 2^-6 at 2 and at 3.99
    x = torch.tensor([1.0, 0.999, 2.0, 3.99, -1.5], dtype=torch.float64)
    assert X._ulp_bf16(x).tolist() == [2.0 ** -7, 2.0 ** -8, 2.0 ** -6, 2.0 ** -6, 2.0 ** -7]


def test_clamp_masks_and_dead_rows():
    a, w, k, v = _ops(8)
    a = a * 4                                                                    # logits that a clamp of 3 bends
    kv_len, q_len = [7, 0], [20, NQ]
    got = X.qx_ref64(a, w, k, v, B=B, H=H, Nq=NQ, kv_len=kv_len, q_len=q_len, clamp=3.0)
    assert float(got[0, 20:].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0     # past q_len; a clip without keys
    assert float(got[0, :20].abs().min()) > 0.0
    # clip 0 by hand: 7 live keys, tanh clamp, softmax, gate
    z = a @ w.t()
    for h in range(H):
        q = z[:20, h * 64:(h + 1) * 64]
        s = 3.0 * torch.tanh(X.SCALE * q @ k[0, :7, h * 64:(h + 1) * 64].t() / 3.0)
        want = torch.softmax(s, -1) @ v[0, :7, h * 64:(h + 1) * 64] * torch.sigmoid(z[:20, INNER + h])[:, None]
        torch.testing.assert_close(got[0, :20, h * 64:(h + 1) * 64], want, rtol=1e-12, atol=1e-12)
    # masked keys do not enter: garbage behind kv_len changes nothing
    k2, v2 = k.clone(), v.clone()
    k2[0, 7:], v2[0, 7:] = 1e3, -1e3
    assert torch.equal(X.qx_ref64(a, w, k2, v2, B=B, H=H, Nq=NQ, kv_len=kv_len, q_len=q_len, clamp=3.0), got)
    # absent lengths are full lengths
    assert torch.equal(X.qx_ref64(a, w, k, v, B=B, H=H, Nq=NQ, clamp=3.0), X.qx_ref64(a, w, k, v, B=B, H=H, Nq=NQ, kv_len=[NK, NK], q_len=[NQ, NQ], clamp=3.0))


def test_stored_operands_are_what_the_reference_reads():
    case = X.EDGE_CASES["nk5"]
    for dt in X.DTS:
        o = X.operands(case, dt)
        M = case["B"] * case["Nq"]
        assert o["a"].dtype == torch.bfloat16 and o["a"].shape == (M, case["K"] * (2 if dt == "split" else 1))
        assert o["k"].dtype == (torch.float32 if dt == "split" else torch.bfloat16)
        assert o["ssq"].shape == (M, 40) and bool((o["ssq"][:, case["K"] // 32:] == X.SSQ_SENTINEL).all())
        assert o["tab"].shape[0] == case["rope_off"] + case["Nq"]
    s = X.operands(case, "split")
    a32 = X._raw(case["B"], case["H"], case["Nq"], case["Nk"], case["K"], True)[0]
    assert torch.equal(s["a"][:, :case["K"]], a32.bfloat16())
    assert float((s["a64"] - a32.double()).abs().max()) <= 2.0 ** -16 * float(a32.abs().max())


@pytest.mark.parametrize("lst,name", [(lst, n) for lst, cases in X.CASE_LISTS.items() for n, c in cases.items() if "bf16" in c["dts"]])
def test_inputs_leave_room_under_the_bf16_bar(lst, name):
    """The bf16 storage point alone (q and gate rounded, everything else float64) moves the result by less than half the bf16 bar: the kernel
    keeps the other half for its bf16 weights and output."""
    case = X.CASE_LISTS[lst][name]
    ref, free = X.reference(case, "bf16"), X.reference(case, "bf16", round_bf16=False)
    half = X.TOL["bf16"] / 2
    print(f"{lst} {name}: storage point moves the reference by {float((ref - free).abs().max() / free.abs().max()):.2e} of max |ref|")
    torch.testing.assert_close(ref, free, atol=half, rtol=half)
    assert 1.0 < float(free.abs().max()) < 6.0


def test_case_tables():
    assert sorted({K // 64 % 3 for K in X.K_RING}) == [0, 1, 2] and 4096 in X.K_RING and max(X.K_RING) == 4096
    assert all(K % 512 == 0 for K in X.K_RING)
    assert [K // 64 % 3 for K in X.K_RING] == [2, 1, 0, 2, 0, 1]
    for order in X.K_ORDERS.values():
        assert sorted(order) == X.K_RING
    assert X.K_ORDERS["k4096_first"][0] == 4096 and X.K_ORDERS["k4096_last"][-1] == 4096
    assert set(X.K_TWO_LAUNCH) == {1536, 4096} and set("K%d" % K for K in X.K_RING) == set(X.RING_CASES)
    for cases in X.CASE_LISTS.values():
        for c in cases.values():
            assert c["Nq"] <= 260 and c["Nk"] <= 64 and c["K"] <= 4096 and c["K"] % 512 == 0 and (c["H"] <= 3 or (c["H"] == 16 and c["dts"] == ("split",)))
            assert not c["folded"] or c["K"] <= 1280
            assert c["kv_len"] is None or len(c["kv_len"]) == c["B"]
            assert c["q_len"] is None or len(c["q_len"]) == c["B"]
    assert {c["clamp"] for c in X.ENGINE_CASES.values()} == {50.0, 80.0, 0.0} and {c["layout"] for c in X.ENGINE_CASES.values()} == {"engine", "engine2"}
    assert [X._clamp_mode(c, 64) for c in (50.0, 80.0, 0.0)] == [2, 1, 0]
    assert {c["K"] for c in X.EPILOGUE_CASES.values() if c["folded"]} == {512, 1024}
    assert {(c["rope_cols"], c["rope_off"]) for n, c in X.EPILOGUE_CASES.items() if n.startswith("rope_cols64")} == {(64, 0), (64, 7)}
    # the clamp rule's last integers with CLAMP = 2
    assert [max(i for i in range(1, 200) if X._clamp_mode(float(i), n) == 2) for n in (1, 64)] == [62, 58]
