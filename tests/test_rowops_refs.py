"""CPU: the float64 reference helpers, the tolerance formulas and the inputs of tests/test_rowops_gpu.py against independent forms -- the oracle,
torch, Python loops and vectors the reference's own code produced -- so that a wrong helper cannot agree with a kernel that is wrong in the
same way, and no tolerance is loose enough to hide a wrong lane: every fp32 formula stays below 1e-3 of the RMS of its reference on every case
of the GPU file's parameter lists (the bf16 formulas are the format's half ulp plus the fp32 formula, checked as such)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_rowops_gpu as R
from oracle import e2_cfm_oracle as O

CAP = 1e-3                       # largest tolerance / RMS of the reference


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rms(v):
    return float(v.double().pow(2).mean().sqrt())


def _bound_ok(what, tol, ref, cap=CAP):
    """The tolerance is finite, positive wherever the reference is not exactly 0, and below cap * RMS(ref) everywhere."""
    tol, ref = tol.double(), ref.double()
    assert bool(torch.isfinite(tol).all()) and bool((tol >= 0).all()), what
    assert bool((tol[ref != 0] > 0).all()), what
    ratio = float(tol.max()) / _rms(ref)
    assert 0 < ratio < cap, (what, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------- bf16 half ulp
def test_half_ulp_bf16_is_the_rounding_bound_and_2_pow_minus_9_is_not():
    x = torch.randn(20000, generator=_g(1)) * 3
    err = (x.bfloat16().double() - x.double()).abs()
    h = R._half_ulp_bf16(x)
    assert bool((err <= h).all())                                            # round to nearest never misses by more than half an ulp
    assert bool((h <= 2.0 ** -8 * x.double().abs()).all()) and bool((h > 2.0 ** -9 * x.double().abs() * (1 - 1e-12)).all())
    frac = float((err > 2.0 ** -9 * x.double().abs()).double().mean())
    assert 0.15 < frac < 0.35, frac                                          # ... and 2^-9 |x| is passed by a quarter of all roundings
    v = torch.tensor([1.0, 1.9921875, 2.0, -3.0, 0.0, 2.0 ** -100])
    assert R._half_ulp_bf16(v).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -108]
    sp, is_tie = R.bf16_specials()
    t = sp[is_tie]
    assert torch.equal((t.bfloat16().double() - t.double()).abs(), R._half_ulp_bf16(t))          # the ties sit on the bound


# ------------------------------------------------------------------------------------------------------------- rmsnorm
def test_rmsnorm_ref_against_normalize_and_oracle():
    for d in R.RMS_WIDTHS:
        c = R.rms_case(d)
        x, g = c["x"][:, :d], c["g"]
        want = F.normalize(x.double(), dim=-1) * math.sqrt(d) * g.double()
        torch.testing.assert_close(c["ref"], want, rtol=1e-14, atol=0)
        torch.testing.assert_close(c["ref"].float(), O.rmsnorm(x, g), rtol=2e-6, atol=1e-30)
        assert float(c["ref"][R.RMS_ZERO_ROW].abs().max()) == 0.0 and float(c["x"][R.RMS_ZERO_ROW, d:].abs().min()) > 0
        # scaling a row does not change its result: the scaled rows test the range of the sum of squares, not another value
        torch.testing.assert_close(R._rmsnorm_ref(x[R.RMS_BIG_ROW] / 1e3, g), c["ref"][R.RMS_BIG_ROW], rtol=1e-6, atol=0)
        assert c["ldx"] == d + 12 and c["rows"] == 37


def test_gamma_rows_against_a_loop_and_the_kernel_addressing():
    c = R.rms_table_case()
    S, B, d, step, rpb, rows = (c[k] for k in ("S", "B", "d", "step", "rpb", "rows"))
    assert (S, B, step, rpb, rows) == (3, 3, 2, 5, 13) and rows % rpb != 0 and (rows - 1) // rpb == B - 1
    gr = R._gamma_rows(c["tab"], step, rows, rpb)
    flat = c["tab"].reshape(-1)
    for r in range(rows):
        at = step * (B * d) + (r // rpb) * d                                 # base + step * step stride + batch * batch stride
        assert torch.equal(gr[r], flat[at:at + d])
        torch.testing.assert_close(c["ref"][r].float(), O.rmsnorm(c["x"][r, :d], c["tab"][step, r // rpb]), rtol=2e-6, atol=0)


def test_rmsnorm_bounds():
    for c in [R.rms_case(d) for d in R.RMS_WIDTHS] + [R.rms_table_case()]:
        ref = c["ref"]
        _bound_ok("rmsnorm f32", R.tol_rms_f32(ref), ref)
        _bound_ok("rmsnorm hi + lo", R.tol_rms_split(ref), ref)
        # bf16: the half ulp of the format and, beyond it, nothing but the fp32 bound
        assert torch.equal(R.tol_rms_bf16(ref) - R._half_ulp_bf16(ref), R.tol_rms_f32(ref)) or bool(
            ((R.tol_rms_bf16(ref) - R._half_ulp_bf16(ref) - R.tol_rms_f32(ref)).abs() <= 1e-12 * ref.abs()).all())
        assert bool((R.tol_rms_bf16(ref) <= (2.0 ** -8 + 64 * R.U) * ref.abs()).all())


# ------------------------------------------------------------------------------------------------------------- rope
@pytest.mark.parametrize("layout", [0, 1])
def test_rope_ref_against_the_oracle(layout):
    name = ["interleaved", "half"][layout]
    rows, nheads = 21, 3
    c = R.rope_case(rows, nheads, layout, False)
    rpb, off = c["rpb"], c["off"]
    assert (rows, rpb, off) == (21, 7, 5) and c["tab"].shape == (12, 32, 2) and c["stride"] == nheads * 64 + 16
    pos = torch.arange(rows) % rpb + off
    assert int(pos.max()) == 11 and pos[rpb] == off and pos[2 * rpb] == off  # the table's last row; two wraps
    z = c["z"][:rows, :nheads * 64].double()
    t = z.reshape(rows // rpb, rpb, nheads, 64).permute(0, 2, 1, 3)          # (b, h, n, 64)
    want = O.apply_rope(t, O.rotary_freqs(off + rpb, 64, name).double(), name).permute(0, 2, 1, 3).reshape(rows, nheads * 64)
    torch.testing.assert_close(c["ref"][:, :nheads * 64], want, rtol=0, atol=2e-6)             # fp32 table against cos / sin in double
    assert torch.equal(c["ref"][:, nheads * 64:], c["z"][:rows, nheads * 64:].double())       # behind the heads: untouched
    # the rotation is a complex product by the table row, whatever the layout
    a, b = R._rope_pairs(z, nheads, layout)
    ra, rb = R._rope_pairs(c["ref"], nheads, layout)
    rot = torch.view_as_complex(c["tab"].double())[pos][:, None, :]
    torch.testing.assert_close(torch.complex(ra, rb), torch.complex(a, b) * rot, rtol=0, atol=1e-14)
    assert torch.equal(R._rope_unpairs(a, b, layout), z)
    m = R._rope_unpairs(a.abs() + b.abs(), a.abs() + b.abs(), layout)
    assert torch.equal(c["mag"][:, :nheads * 64], m) and float(c["mag"][:, nheads * 64:].abs().max()) == 0.0


def test_rope_bounds_and_cases():
    assert (100, 16) in R.ROPE_CASES and (100 * 16 * 8) % 256 == 0 and (101 * 16 * 8) % 256 != 0 and (21 * 3 * 8) % 256 != 0
    for rows, nheads in R.ROPE_CASES:
        for layout in (0, 1):
            for bf in (False, True):
                c = R.rope_case(rows, nheads, layout, bf)
                hc = nheads * 64
                ref, mag = c["ref"][:, :hc], c["mag"][:, :hc]
                _bound_ok("rope", R.tol_rope(mag), ref)
                if bf:
                    assert torch.equal(c["z"], c["z"].bfloat16().float())
                    assert torch.equal(R.tol_rope(mag, ref) - R.tol_rope(mag), R._half_ulp_bf16(ref)) or bool(
                        ((R.tol_rope(mag, ref) - R.tol_rope(mag) - R._half_ulp_bf16(ref)).abs() <= 1e-12 * ref.abs() + 1e-300).all())


# ------------------------------------------------------------------------------------------------------------- linear_small
def test_linear_ref_against_a_scatter_loop():
    B, T, K, d, Roff, dup, stride = 2, 3, 5, 4, 2, 2, (2 + 3) * 4 + 8
    g = _g(3)
    a, wt = torch.randn(B * T, K, generator=g), torch.randn(K, d, generator=g)
    bias, add, regs = torch.randn(d, generator=g), torch.randn(T, d, generator=g), torch.randn(Roff, d, generator=g)
    for use_bias, use_add, use_regs, use_dup in [(True, True, True, True), (False, False, False, False), (True, False, True, False),
                                                 (False, True, False, True)]:
        val, wr, mag = R._linear_ref(a, wt, bias if use_bias else None, add if use_add else None, regs if use_regs else None, B=B, T=T, d=d,
                                     row_off=Roff, dup=dup if use_dup else 0, stride=stride)
        nb = B + dup if use_dup else B
        want = np.full((nb, stride), np.nan)
        wmag = np.zeros((nb, stride))
        for m in range(B * T):
            for n in range(d):
                v = sum(float(a[m, k]) * float(wt[k, n]) for k in range(K))
                s = sum(abs(float(a[m, k])) * abs(float(wt[k, n])) for k in range(K))
                if use_bias:
                    v, s = v + float(bias[n]), s + abs(float(bias[n]))
                if use_add:
                    v, s = v + float(add[m % T, n]), s + abs(float(add[m % T, n]))
                for b in [m // T] + ([m // T + dup] if use_dup else []):
                    want[b, (Roff + m % T) * d + n], wmag[b, (Roff + m % T) * d + n] = v, s
        if use_regs:
            for b in range(nb):
                for r in range(Roff):
                    want[b, r * d:(r + 1) * d] = regs[r].double().numpy()
        assert np.array_equal(wr.numpy(), ~np.isnan(want))
        np.testing.assert_allclose(val.numpy()[wr.numpy()], want[wr.numpy()], rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(mag.numpy(), wmag, rtol=1e-14, atol=0)
        assert float(val[~wr].abs().max()) == 0.0


def test_linear_forms_follow_the_dispatch_rule():
    """blocks = ceil((R_fused + T) / 8) * B: below 512 for the 2-row form, at least 512 for the 8-row forms with and without fused registers."""
    for name, f in R.LIN_FORMS.items():
        for fused in (0, f["R"]):
            blocks = (fused + f["T"] + 7) // 8 * f["B"]
            assert (blocks >= 512) == name.startswith("8row"), (name, fused, blocks)
    f = R.LIN_FORMS["8row_full"]
    assert (f["R"] + f["T"]) % 8 == 0 and 0 < f["R"] < 8                      # a block of register rows and data rows, no empty row
    f = R.LIN_FORMS["8row_ragged"]
    assert (f["R"] + f["T"]) % 8 == 7                                        # one empty row in the last block
    ks, ds = {c[0] for c in R.LIN_CASES}, {c[1] for c in R.LIN_CASES}
    assert ks == {1, 51, 1024, 1032, 2048} and ds == {4, 64, 1280}
    for i, n in enumerate(("bias", "add", "regs", "shadow", "dup")):
        assert {c[2 + i] for c in R.LIN_CASES} == {True, False}, n
    assert 2 * 8 * 1024 * 4 == 65536 < 2 * 8 * 1032 * 4


@pytest.mark.parametrize("form", list(R.LIN_FORMS))
def test_linear_bounds(form):
    for K, d, bias, add, regs, shadow, dup in R.LIN_CASES:
        c = R.lin_case(form, K, d, bias, add, regs, dup)
        lo, hi = c["R"] * d, (c["R"] + c["T"]) * d
        ref, tol = c["ref"][:c["B"], lo:hi], R.tol_linear(K, c["mag"])[:c["B"], lo:hi]
        assert bool(c["written"][:, lo:hi].all()) and c["stride"] == hi + R.LIN_PAD
        _bound_ok("linear_small %s K=%d d=%d" % (form, K, d), tol, ref)
        assert float(c["mag"][:, :lo].abs().max()) == 0.0                    # register rows: exact
        if dup:
            assert torch.equal(c["ref"][:c["B"]], c["ref"][c["B"]:])
        R._CASES.pop(("lin", form, K, d, bias, add, regs, dup))              # the large ones are not kept around on the CPU


# ------------------------------------------------------------------------------------------------------------- time_cond
def test_time_cond_ref_against_the_oracle(small):
    P = small["P"]
    fw, w, b = (P["transformer.time_cond_mlp." + k] for k in ("0.weights", "1.weight", "1.bias"))
    d = w.shape[0]
    assert d == 128 and fw.shape == (64,)
    t = torch.tensor([0.0, 0.37, 1.0])
    r = R._time_cond_ref(t, fw, w.t().contiguous(), b)
    torch.testing.assert_close(r["ref"].float(), O.time_cond(P, t), rtol=0, atol=5e-6)
    torch.testing.assert_close(r["ref"], F.silu(r["z"]), rtol=1e-14, atol=0)
    # the partial sums, by a loop, in the kernel's order
    wt = w.t().double()
    e = torch.cat((t[:, None], O.fourier_embed(t, fw)[:, 1:]), -1).double()
    for s, n in ((1, 5), (2, 127)):
        acc, run = float(b[n]), 0.0
        for k in range(d + 1):
            acc += float(e[s, k]) * float(wt[k, n])
            run += abs(acc) + abs(float(e[s, k]) * float(wt[k, n]))
        assert abs(acc - float(r["z"][s, n])) < 1e-5 and abs(run - float(r["run"][s, n])) < 1e-3 * run
    # the derived bound is no looser than the 2e-5 the existing golden test allows at this very shape, and than the order-free one
    tol = R.tol_time_cond(r)
    assert 0 < float(tol.max()) <= 2e-5, float(tol.max())
    assert bool((tol <= R.tol_time_cond_classical(d, r)).all()) and float(R.tol_time_cond_classical(d, r).max()) > 2e-5


def test_time_cond_bounds():
    for d in R.TC_WIDTHS:
        for S in R.TC_S:
            c = R.tc_case(d, S)
            assert c["fw"].shape == (d // 2,) and c["wt"].shape == (d + 1, d) and c["ref"].shape == (S, d)
            tol = R.tol_time_cond(c)
            _bound_ok("time_cond d=%d S=%d" % (d, S), tol, c["ref"])
            assert bool((tol <= R.tol_time_cond_classical(d, c)).all())
            assert d == 2 or float(c["ref"].std()) > 0.3                     # neighbouring columns differ by far more than the bound
    t = R.tc_times(33)
    assert float(t[0]) == 0.0 and float(t[-1]) == 1.0 and float(R.tc_times(1)[0]) == 1.0


# ------------------------------------------------------------------------------------------------------------- apg_reduce, cfg_euler
def test_apg_and_euler_refs_against_the_oracle():
    c = R.apg_case()
    pc, pn, y = c["pc"], c["pn"], c["y"]
    B, T, C = pc.shape
    assert (B, T, C) == (3, 1100, 128) and T * C > 64 * 2048 and c["pbs"] == (c["row_off"] + T) * C + 8
    # the views into the flat buffer are the kernel's addressing: pred + b * pbs + row_off * C
    for b in range(2 * B):
        at = b * c["pbs"] + c["row_off"] * C
        assert torch.equal(c["flat"][at:at + T * C].reshape(T, C), (pc if b < B else pn)[b % B])
    sums = R._apg_sums_ref(pc, pn, None)
    par, orth = O.apg_project(pc.double() - pn.double(), pc.double())
    for keep in (0.0, 0.3):
        ref, rpar = R._euler_ref(y, pc, pn, 0.25, 2.0, sums, keep)
        torch.testing.assert_close(rpar, par, rtol=1e-11, atol=1e-15)
        torch.testing.assert_close(ref, y.double() + 0.25 * (pc.double() + 2.0 * (orth + keep * par)), rtol=0, atol=1e-12)
    plain, zero = R._euler_ref(y, pc, pn, 0.25, 2.0, None, 0.3)
    assert torch.equal(plain, y.double() + 0.25 * (pc.double() + 2.0 * (pc.double() - pn.double()))) and float(zero.abs().max()) == 0.0
    # valid rows: a loop over the clamp
    for v in R.APG_VALID:
        n = T if v is None else min(T, max(0, v))
        want = torch.tensor([[float(((pc[b, :n].double() - pn[b, :n].double()) * pc[b, :n].double()).sum()), float((pc[b, :n].double() ** 2).sum())]
                             for b in range(B)], dtype=torch.float64)
        torch.testing.assert_close(R._apg_sums_ref(pc, pn, v), want, rtol=1e-13, atol=0)
    assert [T if v is None else min(T, max(0, v)) for v in R.APG_VALID] == [1100, 0, 1, 1099, 1100, 1100, 0]


def test_euler_ref_against_the_reference_project_vectors():
    from conftest import GOLDEN
    r = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "intree_blocks.npz"), allow_pickle=False).items() if k.startswith("project_")}
    pc, upd, par, orth = r["project_y"], r["project_x"], r["project_parallel"], r["project_orthogonal"]
    pn = pc - upd
    y = torch.randn(pc.shape, generator=_g(4))
    ref, rpar = R._euler_ref(y, pc, pn, 0.125, 2.0, R._apg_sums_ref(pc, pn, None), 0.25)
    torch.testing.assert_close(rpar.float(), par, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ref.float(), y + 0.125 * (pc + 2.0 * (orth + 0.25 * par)), rtol=1e-5, atol=2e-6)


def test_euler_bounds_and_the_degenerate_clip():
    for zero in (False, True):
        c = R.apg_case(zero)
        pc, pn, y = c["pc"], c["pn"], c["y"]
        for sums in (None, R._apg_sums_ref(pc, pn, None), R._apg_sums_ref(pc, pn, 0)):
            for h in R.EULER_DT:
                ref, par = R._euler_ref(y, pc, pn, h, R.EULER_S, sums, 0.3)
                assert bool(torch.isfinite(ref).all())
                _bound_ok("cfg_euler", R.tol_euler(y, pc, pn, par, h, R.EULER_S), ref)
    c = R.apg_case(True)
    assert float(c["pc"][1].abs().max()) == 0.0 and float(c["pc"][0].abs().max()) > 0
    assert R._apg_sums_ref(c["pc"], c["pn"], None)[1].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------- split_bf16, cast_bf16
def test_tie_inputs_are_ties():
    sp, is_tie = R.bf16_specials()
    assert bool(torch.isfinite(sp).all())
    nz = sp[sp != 0]
    assert float(nz.abs().min()) >= 2.0 ** -101 and float(nz.abs().min()) > torch.finfo(torch.float32).tiny               # no subnormal
    assert float(sp.abs().max()) > 1e29 and int((sp == 0).sum()) == 2 and bool(torch.signbit(sp[sp == 0]).tolist() == [False, True])
    t = sp[is_tie]
    n = t.numel()
    bits = t.view(torch.int32)
    down = (bits & ~0xFFFF).view(torch.float32)                              # the bf16 neighbour towards zero
    up = ((bits & ~0xFFFF) + 0x10000).view(torch.float32)                    # the one away from zero (a carry moves into the next binade)
    assert torch.equal(down.bfloat16().float(), down) and torch.equal(up.bfloat16().float(), up)
    assert torch.equal(t.double(), (down.double() + up.double()) / 2)        # exactly half way
    odd = ((bits >> 16) & 1).bool()
    assert int(odd.sum()) == n // 2                                          # both parities of the lower neighbour
    assert torch.equal(t.bfloat16().float(), torch.where(odd, up, down))     # torch rounds ties to even
    assert int(((bits >> 16) & 0x7F == 0x7F).sum()) >= 1                     # a tie that rounds up into the next binade
    # one fp32 ulp either side of a tie is decided by the value, not by parity
    below, above = sp[n:2 * n], sp[2 * n:3 * n]
    assert torch.equal(below.view(torch.int32), bits - 1) and torch.equal(above.view(torch.int32), bits + 1)
    assert torch.equal(below.bfloat16().float(), down) and torch.equal(above.bfloat16().float(), up)
    # values whose hi plane rounds up leave a negative lo plane (of the value's own sign reversed), and no lo plane is subnormal in bf16
    hi = sp.bfloat16().float()
    lo = (sp - hi).bfloat16().float()
    assert int((torch.sign(lo) * torch.sign(sp) < 0).sum()) >= n
    assert float(lo[lo != 0].abs().min()) >= 2.0 ** -126
    assert torch.equal((hi.double() + (sp - hi).double()), sp.double())      # x - hi is exact in fp32
    # the specials lead every input the GPU tests build, the ties first
    for d in R.SPLIT_WIDTHS:
        v = R.bf16_values(R.SPLIT_ROWS * d, 901 + d)
        k = min(v.numel(), sp.numel())
        assert torch.equal(v[:k].view(torch.int32), sp[:k].view(torch.int32)) and k >= n
    assert sp.numel() <= R.SPLIT_ROWS * 260 and sp.numel() <= 1028
    assert int(torch.equal(R.bf16_values(4, 954).view(torch.int32), sp[:4].view(torch.int32)))
