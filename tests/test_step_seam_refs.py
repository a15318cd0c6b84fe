"""CPU: the float64 reference helpers, the case lists and the bars of tests/test_step_seam_abi_gpu.py against independent forms -- Python loops over
the formulas of include/v2a_cfm.h, torch, and the oracle's own CFG + Euler loop -- so that a wrong helper cannot agree with a kernel that is wrong
in the same way, and against a plain fp32 evaluation on the CPU, so that tol_euler is known to admit a correct fp32 kernel before any GPU run."""
import itertools

import pytest
import torch

import test_step_seam_abi_gpu as S
from oracle import e2_cfm_oracle as O
from test_rowops_gpu import _apg_sums_ref, _euler_ref, tol_euler

SHAPES = S.ROW_SHAPES + [S.BIG]


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_row_map_and_live_rows_against_loops(shape):
    B, row_off, T, rps = shape
    mh = B * rps
    half, b, r = S.row_map(B, rps)
    live = S.updates_y(rps, row_off, T)
    n_live = 0
    for m in range(2 * mh):
        hh, mm = (1, m - mh) if m >= mh else (0, m)
        bb = mm // rps
        t = mm - bb * rps - row_off                       # the header's b and t of row m of a half
        assert (int(half[m]), int(b[m]), int(r[m])) == (hh, bb, t + row_off)
        assert bool(live[r[m]]) == (0 <= t < T)
        n_live += 0 <= t < T
    assert n_live == 2 * B * T and int(live.sum()) == T


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_row_is_in_exactly_one_tile(shape):
    """The header's tile map: tile row j of band i is row 32 i + (j mod 32) of the conditional (j < 32) or the null half.  Over ceil(mh / 32) bands
    the rows below mh of each half appear once each; what lies at or past mh is the part of the last band that the kernel clamps and skips."""
    B, _, _, rps = shape
    mh = B * rps
    seen = torch.zeros(2 * mh, dtype=torch.int32)
    skipped = 0
    for i in range((mh + 31) // 32):
        for j in range(64):
            r = 32 * i + j % 32
            if r < mh:
                seen[(mh if j >= 32 else 0) + r] += 1
            else:
                skipped += 1
    assert bool((seen == 1).all()) and skipped == 2 * (-mh % 32)


def test_pred_halves_against_loops():
    B, row_off, T, rps, C = 3, 4, 15, 23, 8
    out = torch.randn(2 * B * rps, C, generator=_g(1))
    pc, pn = S.pred_halves(out, B, rps, row_off, T)
    assert pc.shape == pn.shape == (B, T, C)
    for b in range(B):
        for t in range(T):
            assert torch.equal(pc[b, t], out[b * rps + row_off + t]) and torch.equal(pn[b, t], out[B * rps + b * rps + row_off + t])


# ------------------------------------------------------------------------------------------------------------- planes
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("B,T,rps,row_off", [(3, 15, 23, 4), (1, 1, 10, 6), (2, 32, 32, 0), (3, 37, 46, 6)])
def test_plane_rows_and_expected_planes_against_loops(B, T, rps, row_off, copies):
    rows = S.plane_rows(B, T, rps, row_off, copies)
    assert rows.shape == (copies, B, T)
    C, lo = 8, 16
    ld = lo + C + 4
    y = torch.randn(B, T, C, generator=_g(2)) * 3
    total = 2 * B * rps
    got = S.expected_planes(y, total, ld, lo, rps, row_off, copies)
    want = torch.full((total, ld), S.SENT, dtype=torch.bfloat16)
    for k in range(copies):
        for b in range(B):
            for i in range(T):
                row = (k * B + b) * rps + row_off + i         # include/v2a_cfm.h, v2a_y_planes
                assert int(rows[k, b, i]) == row
                for c in range(C):
                    hi = y[b, i, c].bfloat16()
                    want[row, c] = hi
                    want[row, lo + c] = (y[b, i, c] - hi.float()).bfloat16()
    assert torch.equal(got, want)
    assert rows.unique().numel() == rows.numel() and int(rows.max()) < copies * B * rps
    if copies == 1:
        assert bool((got[B * rps:] == S.SENT).all())
    written = (got != S.SENT).any(1)
    assert int(written.sum()) == copies * B * T


def test_split_planes_is_the_library_rule():
    from v2a_amd import _lib
    x = torch.randn(37, 68, generator=_g(3)) * 3
    p = S.split_planes(x)
    assert p.dtype == torch.bfloat16 and torch.equal(p, _lib.split_planes(x)) and torch.equal(p[:, :68], x.bfloat16())
    back = p[:, :68].double() + p[:, 68:].double()
    assert float(((back - x.double()).abs() / x.double().abs()).max()) <= 2.0 ** -16
    assert float(torch.tensor(S.SENT).bfloat16()) == S.SENT           # the sentinel is exact in both formats


def test_row_scale_is_the_consumers_formula():
    import test_gemm_split_ring_gpu as G
    assert S.NORM_DIM == G.NORM_DIM
    c = S.seam_case(S.RAGGED)
    ssq, rstd = c["ssq"], c["rstd"]
    assert bool((ssq[:, S.NORM_DIM // 32:] == 0).all()) and rstd.unique().numel() == c["M"]      # a distinct scale per row
    for m in (0, 5, c["mh"], c["M"] - 1):
        assert abs(float(rstd[m]) - (S.NORM_DIM ** 0.5) / sum(float(v) for v in ssq[m]) ** 0.5) < 1e-12 * float(rstd[m])


# ------------------------------------------------------------------------------------------------------------- the sequence
def _preds(B, T, C, n, seed):
    g = _g(seed)
    return [(torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)) for _ in range(n)]


def test_sequence_ref_against_a_loop():
    B, T, C, s = 2, 3, 4, 2.0
    y0 = torch.randn(B, T, C, generator=_g(4))
    preds, hs = _preds(B, T, C, 3, 5), [0.1, 0.25, 0.05]
    got, tol = S.sequence_ref(y0, preds, hs, s)
    for b in range(B):
        for t in range(T):
            for c in range(C):
                y, bound = float(y0[b, t, c]), 0.0
                for (pc, pn), h in zip(preds, hs):
                    p, q = float(pc[b, t, c]), float(pn[b, t, c])
                    bound += 8 * 2.0 ** -24 * (abs(y) + h * (abs(p) + s * (abs(p) + abs(q))))
                    y = y + h * (p + s * (p - q))
                assert abs(float(got[b, t, c]) - y) <= 1e-14 * max(abs(y), 1.0)
                assert abs(float(tol[b, t, c]) - bound) <= 1e-12 * bound
    one, tol1 = S.sequence_ref(y0, preds[:1], hs[:1], s)
    ref, par = _euler_ref(y0, *preds[0], hs[0], s, None, 0.0)
    assert torch.equal(one, ref) and torch.equal(tol1, tol_euler(y0, *preds[0], par, hs[0], s)) and float(par.abs().max()) == 0.0


@pytest.mark.parametrize("s", [2.0, 0.75, 0.0])
def test_sequence_ref_against_the_oracle_sampler(monkeypatch, s):
    """O.sample's own loop -- cfg_pred (pred + (pred - null) s) and y + dt f over the sway grid -- with the two forwards replaced by canned
    predictions: the sequence the seam's launches must follow.  (Below 1e-5 the oracle takes the conditional prediction alone, x3:2101, which at
    s = 0 is the same value; the kernels' formula is literal in s, and the negative strength of the GPU file is checked against it as written.)"""
    B, T, C, steps = 2, 5, 8, 4
    y0 = torch.randn(B, T, C, generator=_g(6)).double()
    preds = _preds(B, T, C, steps - 1, 7)
    calls = []

    def head(P, cfg, x, *a, drop_text_cond, **kw):
        k = sum(1 for d in calls if d == drop_text_cond)
        calls.append(drop_text_cond)
        return preds[k][1 if drop_text_cond else 0].double()

    monkeypatch.setattr(O, "transformer_with_pred_head", head)
    want = O.sample(None, None, y0, None, None, None, None, steps=steps, cfg_strength=s, remove_parallel_component=False)
    t = O.sway_grid(steps)
    hs = [float(t[i + 1] - t[i]) for i in range(steps - 1)]
    got, _ = S.sequence_ref(y0, preds, hs, s)
    assert calls.count(False) == steps - 1
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-14)
    assert not torch.equal(got, y0)


def test_euler_ref_with_apg_against_the_oracle_projection():
    c = S.planes_case(*S.PLANES_CASES[1])
    pc, pn, y = c["pc"], c["pn"], c["y"]
    par, orth = O.apg_project(pc.double() - pn.double(), pc.double())
    h = float(c["dt"][c["step"]])
    ref, rpar = _euler_ref(y, pc, pn, h, 2.0, _apg_sums_ref(pc, pn, None), S.KEEP)
    torch.testing.assert_close(rpar, par, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref, y.double() + h * (pc.double() + 2.0 * (orth + S.KEEP * par)), rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------- the bar admits fp32
def _fp32_step(y, pc, pn, h, s):
    h, s = torch.tensor(h, dtype=torch.float32), torch.tensor(s, dtype=torch.float32)
    return y + h * (pc + s * (pc - pn))


@pytest.mark.parametrize("strength", S.STRENGTHS)
@pytest.mark.parametrize("shape,N,K", [(sh, 64, 128) for sh in S.ROW_SHAPES] + [(S.RAGGED, 320, 128), (S.BIG, S.BIG_N, S.BIG_K)], ids=str)
def test_tol_euler_admits_an_fp32_evaluation_of_the_seam_cases(shape, N, K, strength):
    """On the generators of the GPU file (the float64 product rounded to fp32 stands for the stored out): the formula in torch fp32 on the CPU
    stays within tol_euler of its float64 value, for every dt, and within the summed bar over three steps."""
    c = S.seam_case(shape, N=N, ks=(K,), nbuf=3 if shape == S.BIG else 1)
    B, row_off, T, rps = shape
    out = (c["acc"][0] + c["bias"].double()).float()
    pc, pn = S.pred_halves(out, B, rps, row_off, T)
    worst = 0.0
    for k in range(S.NDT):
        h = float(c["dt"][k])
        ref, par = _euler_ref(c["y"], pc, pn, h, strength, None, 0.0)
        tol = tol_euler(c["y"], pc, pn, par, h, strength)
        assert bool((tol > 0).all())
        worst = max(worst, float(((_fp32_step(c["y"], pc, pn, h, strength).double() - ref).abs() / tol).max()))
    assert worst <= 1.0, worst
    if len(c["acc"]) == 3:
        preds = [S.pred_halves((a + c["bias"].double()).float(), B, rps, row_off, T) for a in c["acc"]]
        hs = [float(c["dt"][2 + k]) for k in range(3)]
        ref, tol = S.sequence_ref(c["y"], preds, hs, strength)
        y = c["y"]
        for (p, q), h in zip(preds, hs):
            y = _fp32_step(y, p, q, h, strength)
        assert float(((y.double() - ref).abs() / tol).max()) <= 1.0


@pytest.mark.parametrize("case", S.PLANES_CASES, ids=lambda t: "-".join(str(v) for v in t))
def test_tol_euler_admits_an_fp32_evaluation_of_the_planes_cases(case):
    """With APG the fp32 form takes the projection coefficient from the float64 sums, rounded once to fp32, as the header describes it."""
    c = S.planes_case(*case)
    y, pc, pn = c["y"], c["pc"], c["pn"]
    h, s = float(c["dt"][c["step"]]), c["strength"]
    sums = _apg_sums_ref(pc, pn, None) if c["apg_on"] else None
    ref, par = _euler_ref(y, pc, pn, h, s, sums, S.KEEP)
    tol = tol_euler(y, pc, pn, par, h, s)
    if sums is None:
        got = _fp32_step(y, pc, pn, h, s)
    else:
        coef = (sums[:, 0] / sums[:, 1]).float()[:, None, None]
        p32 = coef * pc
        upd = ((pc - pn) - p32) + p32 * torch.tensor(S.KEEP, dtype=torch.float32)
        got = y + torch.tensor(h, dtype=torch.float32) * (pc + torch.tensor(s, dtype=torch.float32) * upd)
    assert got.dtype == torch.float32
    assert float(((got.double() - ref).abs() / tol).max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------- the case lists
def test_planes_cases_cover_every_value_and_every_pair():
    cols = list(zip(*S.PLANES_CASES))
    copies, trail, prow, wide, C, T, B, pad, step, apg, strength = cols
    assert set(copies) == {1, 2} and set(trail) == {0, 3} and set(prow) == {S.PRED_ROW_OFF, 6} and set(wide) == {False, True}
    assert set(C) == {4, 68, 260} and set(T) == {1, 37} and set(B) == {1, 3} and set(pad) == {0, 16} and set(apg) == {False, True}
    assert any(v != 0 for v in step) and 0 in step and max(step) < S.NDT
    for i, j in itertools.combinations(range(4), 2):
        assert len(set(zip(cols[i], cols[j]))) == 4, (i, j)
    for case in S.PLANES_CASES:
        c = S.planes_case(*case)
        assert c["rps"] == c["prow"] + c["T"] + case[1] and c["ld"] % 4 == 0 and c["lo"] % 4 == 0 and c["ld"] >= c["lo"] + c["C"] and c["pbs"] % 4 == 0
        assert (c["lo"], c["ld"]) == ((c["C"] + 8, 2 * c["C"] + 12) if case[3] else (c["C"], 2 * c["C"]))
        assert c["pbs"] == (S.PRED_ROW_OFF + c["T"]) * c["C"] + case[7]


def test_seam_cases_are_the_listed_shapes():
    assert S.ROW_SHAPES == [(1, 4, 28, 32), (1, 4, 5, 9), (1, 4, 41, 45), (3, 4, 15, 23), (2, 0, 32, 32)]
    assert (S.BIG, S.BIG_N, S.BIG_K) == ((8, 4, 103, 107), 640, 64) and ((8 * 107 + 31) // 32) * (640 // 64) == 270
    assert S.SEAM_N == [128, 192, 320] and S.SEAM_K == [64, 192, 256, 448] and S.STRENGTHS == [0.0, 2.0, -0.5]
    assert all(len(ks) in (2, 3) for ks in S.SEG_KS) and {len(ks) for ks in S.SEG_KS} == {2, 3}
    c = S.seam_case(S.RAGGED)
    assert c["M"] == 2 * 69 and c["rps"] > c["row_off"] + c["T"]
    # every row of a has its own magnitude: RMS of row m grows as 1 + m / mh
    rms = c["a"][0][0].double().pow(2).mean(1).sqrt()
    assert float(rms[-8:].mean() / rms[:8].mean()) > 2.2
    assert len(set(c["dt"].tolist())) == S.NDT and 0.05 <= float(c["dt"].min()) <= float(c["dt"].max()) <= 0.25
    # operands are never modified: a second request returns the same tensors
    assert S.seam_case(S.RAGGED) is c
