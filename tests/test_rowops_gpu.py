"""GPU: the row kernels of csrc/rowops.hip that run around the GEMMs in every Euler step -- v2a_rmsnorm, v2a_rope_inplace, v2a_linear_small,
v2a_fill_registers, v2a_time_cond, v2a_apg_reduce, v2a_cfg_euler, v2a_split_bf16, v2a_cast_bf16 -- against plain float64 restatements of the
formulas in include/v2a_cfm.h, at the widths, strides and launch forms tests/test_kernels_gpu.py does not reach.

Every reference below takes the fp32 inputs converted to double; none calls the oracle module or a kernel (tests/test_rowops_refs.py checks
them on the CPU against the oracle, torch and Python loops, and checks that no tolerance is loose enough to hide a wrong lane).  Inputs come from
seeded CPU generators, are made once per case (the _CASES cache) and never modified.  Every output buffer is prefilled with SENT, and whatever the
header says a call does not write -- padding columns, rows past `rows`, columns behind the heads, the tail of a flat buffer -- must still hold
it bit for bit.  u = 2^-24 is the fp32 unit roundoff; "half a bf16 ulp" of v is 2^(floor(log2 |v|) - 8) (_half_ulp_bf16).

Tolerances (per element, from the float64 reference; where the reference is exactly 0 the result must be exactly 0):

  rmsnorm fp32     64 u |ref|.  Worst case by derivation ~25 u: the sum of squares is at most 32 terms per lane and 6 shuffle adds, ~39 u, halved
                   by the square root; then sqrtf, the division, sqrtf(d) and two multiplies; the rest is room for a square root or a division
                   that is not correctly rounded.
  rmsnorm bf16     half a bf16 ulp of ref + 64 u |ref| (the fp32 noise that can move a rounding); and bit equality with the fp32 launch's
                   result rounded by .bfloat16().  The same for the hi plane of the split output.
                   (The bound was first written as 2^-9 |ref| for the half ulp.  bf16 keeps 8 significand bits: ulp(v) = 2^(e - 7) for
                   2^e <= |v| < 2^(e + 1), half of it 2^(e - 8), which is 2^-8 |v| at the bottom of a binade and 2^-9 |v| only at its top.
                   Round-to-nearest itself exceeds 2^-9 |v| on a quarter of all values -- test_rowops_refs.py shows that on torch's own
                   conversion -- so the half ulp is taken exactly, which is never looser than 2^-8 |ref| and is what the words say.)
  split hi + lo    2^-16 |ref| + 64 u |ref|: |v - hi| <= 2^(e - 8), and lo rounds that to 8 bits again.
  rope fp32        4 u (|a| + |b|) per pair (a, b): two products and one sum, contracted or not.  bf16: + half a bf16 ulp of ref, the input
                   being the bf16-rounded tensor.
  linear_small     (K + 3) u (sum_k |a_k| |w_kn| + |bias_n| + |add_tn|): the classical bound of a sum of K products and two more terms in any
                   order; FMA contraction only lowers the error.  Register rows and fill_registers are exact copies; the bf16 shadow equals
                   .bfloat16() of the fp32 output bit for bit; the dup half equals the first half bit for bit.
  time_cond        see test_time_cond.
  apg_reduce       rtol 1e-12 (fp64 atomics: any order); exactly 0 where no row enters.
  cfg_euler        8 u (|y| + |dt| (|pc| + |s| (|pc| + |pn| + 2 |par|))), par from the float64 reference.
  split / cast     bit equality with torch's CPU conversion (round to nearest even).

Read out of the code before these tests ran, and what the run showed:
  v2a_linear_small  the 8-row launch form asks for 2 * 8 * K * 4 bytes of dynamic LDS -- 128 KB at the admitted K = 2048 -- and did so without
                    raising the kernel's limit, which csrc/v2a_common.h says is needed past 64 KB.  On the MI355X the library as it was
                    launched K = 1032 and 2048 on the "8row" forms all the same and passed test_linear_small (22 of 22): the runtime grants
                    the device's LDS without the opt-in, so this was no failure there.  The launch now opts in (v2a_enable_lds, as the dwconv
                    streaming kernel does) instead of depending on that; the kernel and its results are unchanged.
No other kernel missed a bound.

Every case prints "rowops <kernel> <group> <case> max |got - ref| / tol = <ratio>" before it asserts ratio <= 1, and the module prints the
largest ratio per (kernel, group) when it is done (pytest -s); profiles/rowops_parity.txt records them as first measured on the MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = -7.25                     # exact in fp32 and in bf16
ERR_ARG = -1                     # V2A_ERR_ARG
F32, BF16, SPLIT = "f32", "bf16", "split"

# ---- rmsnorm
RMS_WIDTHS = [4, 100, 256, 768, 1536, 1792, 2048]     # one lane, a partial wave, float4 per lane 1, 3, 6, the 7 -> 8 instantiation, 8
RMS_ROWS = 37                                          # the last block of four waves has one live wave
RMS_ZERO_ROW, RMS_SMALL_ROW, RMS_BIG_ROW = 3, 5, 36
RMS_TABLE = dict(S=3, B=3, d=100, step=2, rpb=5, rows=13)      # a ragged last batch element
# ---- rope
ROPE_SMALL = dict(rows=21, rpb=7, off=5)               # 12 table rows: the last one is reached, the position wraps twice
ROPE_CASES = [(21, 1), (21, 3), (100, 16), (101, 16)]  # (rows, nheads); 101 x 16 x 8 work items end inside the last block of 256
# ---- linear_small: launch forms by the dispatch rule blocks = ceil((R_fused + T) / 8) * B >= 512
LIN_FORMS = {"2row": dict(B=3, T=9, R=3),
             "8row_full": dict(B=256, T=13, R=3),      # 16 rows with the register rows: block 0 holds register rows and data rows
             "8row_ragged": dict(B=256, T=12, R=3)}    # 15 rows: the last block has an empty row
# (K, d, bias, add, regs fused, bf16 shadow, dup); d stays small where K is large
LIN_CASES = [(1, 4, True, True, True, True, True),
             (51, 64, False, False, False, False, False),
             (51, 1280, True, True, True, True, False),          # d > 1024: a thread takes a second group of four columns
             (1024, 64, True, False, True, True, True),          # 64 KB of LDS on the 8-row form: the most it may ask for
             (1032, 4, True, True, True, False, False),          # the first K past 64 KB on the 8-row form
             (2048, 4, False, False, True, False, True),
             (2048, 64, False, True, False, True, True)]
LIN_PAD = 8                                            # out_batch_stride = (R + T) * d + LIN_PAD
# ---- time_cond
TC_WIDTHS = [2, 130, 256, 384, 1024]
TC_S = [1, 33]
# ---- apg_reduce / cfg_euler
APG = dict(B=3, C=128, T=1100, row_off=4, pad=8)       # T * C > 64 chunks x 2048: the grid-stride loop iterates; 413 blocks of cfg_euler
APG_VALID = [None, 0, 1, 1099, 1100, 1150, -3]
EULER_DT = [0.1, 0.25, 0.05]
EULER_S = 2.0
# ---- split_bf16 / cast_bf16
SPLIT_WIDTHS = [4, 260]
SPLIT_ROWS = 37
CAST_N = [4, 1028, 300000]


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- float64 reference helpers
def _half_ulp_bf16(v):
    """Half the spacing of bf16 (8 significand bits) at |v|, 0 at 0: the largest error of rounding v to nearest."""
    a = v.double().abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.pow(torch.full_like(a, 2.0), e - 8), torch.zeros_like(a))


def _rmsnorm_ref(x, g):
    """y = x / max(|x|_2, 1e-12) * sqrt(d) * gamma; x (rows, d) fp32, g (d,) or (rows, d) fp32."""
    x, g = x.double(), g.double()
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    return x / torch.clamp(n, min=1e-12) * math.sqrt(x.shape[-1]) * g


def _gamma_rows(tab, step, rows, rpb):
    """tab (S, B, d) -> the (rows, d) gamma of every row: base + step * step stride + (row / rpb) * batch stride."""
    return tab[step][torch.arange(rows) // rpb]


def _rope_table(n):
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(n).float()[:, None] * inv[None, :]
    return torch.stack((ang.cos(), ang.sin()), -1).contiguous()


def _rope_pairs(z, nheads, layout):
    """(rows, >= nheads * 64) -> the (rows, nheads, 32) first and second elements of every pair: layout 0 (2i, 2i + 1), 1 (i, i + 32)."""
    h = z[:, :nheads * 64].reshape(z.shape[0], nheads, 64)
    if layout == 0:
        return h[..., 0::2], h[..., 1::2]
    return h[..., :32], h[..., 32:]


def _rope_unpairs(a, b, layout):
    rows, nheads, _ = a.shape
    if layout == 0:
        return torch.stack((a, b), -1).reshape(rows, nheads * 64)
    return torch.cat((a, b), -1).reshape(rows, nheads * 64)


def _rope_ref(z, tab, nheads, rpb, off, layout):
    """fp64: every pair (a, b) of the nheads 64-wide heads times (cos + i sin) of table row off + row % rpb; the other columns pass through.
    Returns (rotated, |a| + |b| of the pair of every element, 0 outside the heads)."""
    z = z.double()
    pos = torch.arange(z.shape[0]) % rpb + off
    cos, sin = tab[pos, :, 0].double()[:, None], tab[pos, :, 1].double()[:, None]
    a, b = _rope_pairs(z, nheads, layout)
    out, mag = z.clone(), torch.zeros_like(z)
    out[:, :nheads * 64] = _rope_unpairs(a * cos - b * sin, b * cos + a * sin, layout)
    m = a.abs() + b.abs()
    mag[:, :nheads * 64] = _rope_unpairs(m, m, layout)
    return out, mag


def _linear_ref(a, wt, bias, add, regs, *, B, T, d, row_off, dup, stride):
    """v2a_linear_small in fp64 on a (batches, stride) buffer: out[m / T][(row_off + m % T) * d + n] = bias[n] + add[m % T][n] + sum_k a[m][k] wt[k][n],
    the same again at batch m / T + dup when dup > 0, rows [0, row_off) = regs when regs is given.  a (B * T, K), wt (K, d).
    Returns (values, written mask, the sum of magnitudes the tolerance is built on: 0 on register rows)."""
    nb = B + dup if dup > 0 else B
    val = torch.zeros(nb, stride, dtype=torch.float64)
    mag, wr = torch.zeros_like(val), torch.zeros(nb, stride, dtype=torch.bool)
    z = a.double() @ wt.double()
    m = a.double().abs() @ wt.double().abs()
    if bias is not None:
        z, m = z + bias.double(), m + bias.double().abs()
    z, m = z.reshape(B, T, d), m.reshape(B, T, d)
    if add is not None:
        z, m = z + add.double(), m + add.double().abs()
    lo, hi = row_off * d, (row_off + T) * d
    for h in ((0, dup) if dup > 0 else (0,)):
        val[h:h + B, lo:hi], mag[h:h + B, lo:hi], wr[h:h + B, lo:hi] = z.reshape(B, T * d), m.reshape(B, T * d), True
        if regs is not None:
            val[h:h + B, :lo], wr[h:h + B, :lo] = regs.double().reshape(1, -1), True
    return val, wr, mag


def _time_cond_ref(t, fw, wt, bias):
    """out[s] = silu(z), z = bias + wt^T [t_s, sin(f), cos(f)], f = ((t_s * w) * 2) * pi formed in fp32 in the kernel's own order (elementwise IEEE
    products: exact restatements), everything after it in fp64.  wt (d + 1, d).  Returns ref = out, z, pmag = sum_k |e_k| |w_kn|,
    mag = |bias_n| + pmag, and run = sum_k |s_k| + pmag over the partial sums s_k = bias_n + sum_(j <= k) e_j w_jn (the kernel's order)."""
    f = (t[:, None] * fw[None, :] * 2 * torch.pi)
    assert f.dtype == torch.float32
    e = torch.cat((t[:, None].double(), f.double().sin(), f.double().cos()), -1)
    w, b = wt.double(), bias.double()
    z = b + e @ w
    pmag = e.abs() @ w.abs()
    run = torch.stack([(b + torch.cumsum(e[s][:, None] * w, 0)).abs().sum(0) for s in range(t.numel())]) + pmag
    return dict(ref=z * torch.sigmoid(z), z=z, pmag=pmag, mag=b.abs() + pmag, run=run)


def _apg_sums_ref(pc, pn, valid):
    """(B, 2) fp64 {sum (pc - pn) pc, sum pc pc} over rows [0, min(T, max(0, valid))) of every clip; pc, pn (B, T, C)."""
    T = pc.shape[1]
    n = T if valid is None else min(T, max(0, valid))
    c, nn = pc[:, :n].double().reshape(pc.shape[0], -1), pn[:, :n].double().reshape(pc.shape[0], -1)
    return torch.stack((((c - nn) * c).sum(-1), (c * c).sum(-1)), -1)


def _euler_ref(y, pc, pn, h, s, sums, keep):
    """y + h (pc + s upd); upd = pc - pn, or with the projection sums (B, 2): par = <upd, pc> / max(|pc|, 1e-12)^2 pc, upd = (upd - par) + keep par.
    Returns (y', par)."""
    y, pc, pn = y.double(), pc.double(), pn.double()
    upd, par = pc - pn, torch.zeros_like(pc)
    if sums is not None:
        nrm = torch.clamp(torch.sqrt(sums[:, 1]), min=1e-12)
        par = (sums[:, 0] / (nrm * nrm))[:, None, None] * pc
        upd = (upd - par) + keep * par
    return y + h * (pc + s * upd), par


# ------------------------------------------------------------------------------------------------------------- tolerances
def tol_rms_f32(ref):
    return 64 * U * ref.abs()


def tol_rms_bf16(ref):
    return _half_ulp_bf16(ref) + 64 * U * ref.abs()


def tol_rms_split(ref):
    return 2.0 ** -16 * ref.abs() + 64 * U * ref.abs()


def tol_rope(mag, ref=None):
    """fp32: 4 u (|a| + |b|); bf16 (ref given): + half a bf16 ulp of ref."""
    return 4 * U * mag + (_half_ulp_bf16(ref) if ref is not None else 0.0)


def tol_linear(K, mag):
    return (K + 3) * U * mag


def tol_time_cond(r):
    """See test_time_cond; r: what _time_cond_ref returns."""
    return 1.1 * (U * r["run"] + 8 * U * r["pmag"]) + (2 * r["z"].abs() + 8) * U * r["ref"].abs()


def tol_time_cond_classical(d, r):
    """The same with the order-free bound of the sum, (d + 4) u (|b_n| + sum_k |e_k| |w_kn|): what tol_time_cond never exceeds."""
    return 1.1 * ((d + 4) * U * r["mag"] + 8 * U * r["pmag"]) + (2 * r["z"].abs() + 8) * U * r["ref"].abs()


def tol_euler(y, pc, pn, par, h, s):
    return 8 * U * (y.double().abs() + abs(h) * (pc.double().abs() + abs(s) * (pc.double().abs() + pn.double().abs() + 2 * par.abs())))


# ------------------------------------------------------------------------------------------------------------- cases, made once on the CPU
_CASES = {}


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def rms_case(d):
    """x (rows, d + 12) with every column random (the padding must not enter the norm), one zero row, one row scaled by 1e-3, one by 1e3."""
    def make():
        x = torch.randn(RMS_ROWS, d + 12, generator=_g(100 + d))
        x[RMS_ZERO_ROW, :d] = 0
        x[RMS_SMALL_ROW] *= 1e-3
        x[RMS_BIG_ROW] *= 1e3
        g = 1 + 0.1 * torch.randn(d, generator=_g(200 + d))
        return dict(d=d, rows=RMS_ROWS, ldx=d + 12, x=x, g=g, ref=_rmsnorm_ref(x[:, :d], g))
    return _cached(("rms", d), make)


def rms_table_case():
    def make():
        c = RMS_TABLE
        x = torch.randn(c["rows"], c["d"] + 12, generator=_g(300))
        tab = 1 + 0.5 * torch.randn(c["S"], c["B"], c["d"], generator=_g(301))
        return dict(c, ldx=c["d"] + 12, x=x, tab=tab, ref=_rmsnorm_ref(x[:, :c["d"]], _gamma_rows(tab, c["step"], c["rows"], c["rpb"])))
    return _cached(("rms_table",), make)


def rope_case(rows, nheads, layout, bf16):
    """(rows + 2, nheads * 64 + 16) random everywhere: the 16 columns behind the heads and the two rows past `rows` must come back unchanged."""
    def make():
        stride = nheads * 64 + 16
        z = torch.randn(rows + 2, stride, generator=_g(400 + rows + nheads))
        if bf16:
            z = z.bfloat16().float()
        tab = _rope_table(ROPE_SMALL["off"] + ROPE_SMALL["rpb"])
        ref, mag = _rope_ref(z[:rows], tab, nheads, ROPE_SMALL["rpb"], ROPE_SMALL["off"], layout)
        return dict(rows=rows, nheads=nheads, stride=stride, z=z, tab=tab, ref=ref, mag=mag, **{k: ROPE_SMALL[k] for k in ("rpb", "off")})
    return _cached(("rope", rows, nheads, layout, bf16), make)


def lin_case(form, K, d, bias, add, regs, dup):
    """Operands of one v2a_linear_small call.  From K = 1024 on a and w are positive (|randn|): with signed operands the sum of magnitudes the
    bound is built on grows as K against sqrt(K) for the result, and the bound would pass 1e-3 of the result's RMS (test_rowops_refs.py)."""
    def make():
        f = LIN_FORMS[form]
        B, T, R = f["B"], f["T"], f["R"]
        g = _g(500 + 7 * K + d + B)
        a, w = torch.randn(B * T, K, generator=g), torch.randn(K, d, generator=g) / math.sqrt(K)
        if K >= 1024:
            a, w = a.abs(), w.abs()
        bv = torch.randn(d, generator=g) if bias else None
        ad = torch.randn(T, d, generator=g) if add else None
        rg = torch.randn(R, d, generator=g)
        stride = (R + T) * d + LIN_PAD
        val, wr, mag = _linear_ref(a, w, bv, ad, rg if regs else None, B=B, T=T, d=d, row_off=R, dup=B if dup else 0, stride=stride)
        return dict(B=B, T=T, R=R, K=K, d=d, a=a, w=w, bias=bv, add=ad, regs=rg, fused=regs, dup=B if dup else 0, stride=stride, ref=val,
                    written=wr, mag=mag)
    return _cached(("lin", form, K, d, bias, add, regs, dup), make)


def tc_times(S):
    return torch.tensor([1.0]) if S == 1 else torch.linspace(0.0, 1.0, S)


def tc_case(d, S):
    """fourier_w ~ N(0, 1), wt ~ N(0, 1) / sqrt(d + 1), bias ~ N(0, 1)."""
    def make():
        g = _g(600 + d)
        fw = torch.randn(d // 2, generator=g)
        wt = torch.randn(d + 1, d, generator=g) / math.sqrt(d + 1)
        bias = torch.randn(d, generator=g)
        t = tc_times(S)
        return dict(_time_cond_ref(t, fw, wt, bias), d=d, S=S, t=t, fw=fw, wt=wt, bias=bias)
    return _cached(("tc", d, S), make)


def apg_case(zero_clip=False):
    """pred (2 B, row_off + T, C) inside a flat buffer whose batch stride carries 8 floats of padding; zero_clip: the conditional prediction of
    clip 1 is all zero."""
    def make():
        c = APG
        B, T, C, R = c["B"], c["T"], c["C"], c["row_off"]
        pbs = (R + T) * C + c["pad"]
        g = _g(700)
        flat = torch.randn(2 * B * pbs, generator=g)
        pred = flat.view(2 * B, pbs)[:, :(R + T) * C].unflatten(1, (R + T, C))       # a view of flat
        if zero_clip:
            pred[1, R:] = 0
            assert float(flat[pbs + R * C:pbs + (R + T) * C].abs().max()) == 0.0
        y = torch.randn(B, T, C, generator=g)
        return dict(c, pbs=pbs, flat=flat, pc=pred[:B, R:].clone(), pn=pred[B:, R:].clone(), y=y)
    return _cached(("apg", zero_clip), make)


def bf16_specials():
    """fp32 values where round-to-nearest-even is decided: exact ties between two bf16 neighbours with the lower neighbour even and odd, the
    fp32 values one ulp either side of such ties, +-0, values that round up (negative lo), magnitudes near 2^-100 and 1e30.  No inf, NaN or
    subnormal, and no lo plane that is subnormal in bf16.  Returns (values, mask of the exact ties)."""
    def make():
        g = _g(800)
        n = 64
        expo = torch.randint(100, 150, (n,), generator=g, dtype=torch.int32)           # 2^-27 .. 2^22
        mant = torch.randint(0, 128, (n,), generator=g, dtype=torch.int32)
        sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
        mant[0::2] &= ~1                                                                # lower neighbour even: the tie rounds down
        mant[1::2] |= 1                                                                 # odd: the tie rounds up, lo = -half ulp
        mant[2], mant[3] = 126, 127                                                     # 127: the tie rounds up into the next binade
        hi = (sign << 31) | (expo << 23) | (mant << 16)
        tie = hi | 0x8000
        up = hi | 0xC123                                                                # past the tie: hi rounds up, lo negative
        scale = lambda e: ((sign << 31) | (torch.full_like(expo, e) << 23) | (mant << 16) | 0x5A5A)   # noqa: E731
        bits = torch.cat([tie, tie - 1, tie + 1, up, scale(27), scale(226), torch.tensor([0, -2 ** 31], dtype=torch.int32)])   # 2^-100, ~1e30
        is_tie = torch.zeros(bits.numel(), dtype=torch.bool)
        is_tie[:n] = True
        return bits.view(torch.float32).clone(), is_tie
    return _cached(("specials",), make)


def bf16_values(n, seed):
    """n fp32 values: the specials, then randn."""
    sp, _ = bf16_specials()
    v = torch.randn(n, generator=_g(seed))
    k = min(n, sp.numel())
    v[:k] = sp[:k]
    return v


# ------------------------------------------------------------------------------------------------------------- reporting
_WORST = {}


def _report(kernel, group, case, got, ref, tol):
    """Prints max |got - ref| / tol, keeps the largest per (kernel, group), asserts it is at most 1; where tol is 0 got must equal ref."""
    got, ref = got.double(), ref.double()
    tol = tol if torch.is_tensor(tol) else torch.full_like(ref, tol)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(got).all()), "%s %s %s: not finite" % (kernel, group, case)
    exact = tol == 0
    assert torch.equal(got[exact], ref[exact]), "%s %s %s: an element that must be exact is not" % (kernel, group, case)
    ratio = float(((got - ref).abs()[~exact] / tol[~exact]).max()) if bool((~exact).any()) else 0.0
    _WORST[(kernel, group)] = max(_WORST.get((kernel, group), 0.0), ratio)
    print("rowops %-13s %-20s %-44s max |got - ref| / tol = %.3f" % (kernel, group, case, ratio))
    assert ratio <= 1.0, (kernel, group, case, ratio)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nrowops parity: largest |got - ref| / tol per kernel and case group")
    for (kernel, group), r in sorted(_WORST.items()):
        print("  %-13s %-20s %.3f" % (kernel, group, r))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def _all_sent(t):
    return bool((t == SENT).all())


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------- rmsnorm
_RMS_F32 = {}


def _rms_launch(L, c, kind, gamma, **kw):
    """One launch into a sentinel buffer of rows + 3 rows with ldy = d + 8 (split: 2 d + 8).  Returns the CPU copy."""
    d, rows = c["d"], c["rows"]
    ldy = (2 * d if kind == SPLIT else d) + 8
    y = _sent((rows + 3, ldy), torch.float32 if kind == F32 else torch.bfloat16)
    L.rmsnorm(c["x"].to(DEV), y, rows=rows, d=d, gamma=gamma.to(DEV), ldx=c["ldx"], ldy=ldy, split=kind == SPLIT, **kw)
    y = y.cpu()
    assert _all_sent(y[rows:]) and _all_sent(y[:rows, (2 * d if kind == SPLIT else d):])      # rows past `rows`, padding columns
    return y


def _rms_check(group, case, kind, y, f32, ref, d):
    """y: what the launch of `kind` left; f32: the (rows, d) result of the fp32 launch on the same inputs."""
    if kind == F32:
        _report("rmsnorm", group + " f32", case, y[:, :d], ref, tol_rms_f32(ref))
        return
    hi = y[:, :d]
    _report("rmsnorm", group + " bf16", case, hi, ref, tol_rms_bf16(ref))
    assert _same_bits(hi, f32.bfloat16())                                    # the rounding of the very fp32 result, not of a neighbour
    if kind == SPLIT:
        _report("rmsnorm", group + " hi+lo", case, hi.double() + y[:, d:2 * d].double(), ref, tol_rms_split(ref))


@pytest.mark.parametrize("kind", [F32, BF16, SPLIT])
@pytest.mark.parametrize("d", RMS_WIDTHS)
def test_rmsnorm_widths_and_strides(L, d, kind):
    """Every float4-per-lane instantiation the existing tests do not launch (3, 6, 8, and 8 serving 7), a single lane, a last float4 group that
    ends inside a wave, with ldx = d + 12 and ldy = d + 8 (2 d + 8 with the lo plane at column d), 37 rows; an all-zero row comes out exactly 0
    (the reference is 0 there and _report demands equality), rows scaled by 1e-3 and 1e3 come out as the unscaled row would."""
    c = rms_case(d)
    rows = c["rows"]
    if d not in _RMS_F32:
        _RMS_F32[d] = _rms_launch(L, c, F32, c["g"])[:rows, :d].clone()
    y = _RMS_F32[d] if kind == F32 else _rms_launch(L, c, kind, c["g"])[:rows]
    assert float(c["ref"][RMS_ZERO_ROW].abs().max()) == 0.0
    _rms_check("widths", "d=%d" % d, kind, y, _RMS_F32[d], c["ref"], d)


@pytest.mark.parametrize("kind", [F32, BF16, SPLIT])
def test_rmsnorm_gamma_table(L, kind):
    """A (steps, batch, d) gamma table addressed by step[0] = 2 and row / rows_per_batch, 13 rows of 5 per batch element, on every output type."""
    c = rms_table_case()
    kw = dict(step=_i32(c["step"]), gamma_step_stride=c["B"] * c["d"], gamma_batch_stride=c["d"], rows_per_batch=c["rpb"])
    f32 = _rms_launch(L, c, F32, c["tab"], **kw)[:c["rows"], :c["d"]]
    y = f32 if kind == F32 else _rms_launch(L, c, kind, c["tab"], **kw)[:c["rows"]]
    _rms_check("table", "S=3 B=3 d=%d step=2" % c["d"], kind, y, f32, c["ref"], c["d"])


def test_rmsnorm_refusals(L):
    """d = 2052 (> 2048), d = 6 (no float4), a split row shorter than two planes, an unknown y dtype: V2A_ERR_ARG, nothing written."""
    x = torch.randn(4, 4096, generator=_g(1)).to(DEV)
    g = torch.ones(4096, device=DEV)
    for d, ldy, ydt, dtype in [(2052, 2052, L.F32, torch.float32), (6, 8, L.F32, torch.float32), (64, 2 * 64 - 4, L.BF16_SPLIT, torch.bfloat16),
                               (64, 64, 7, torch.float32)]:
        y = _sent((4, 4096), dtype)
        rc = L.lib().v2a_rmsnorm(x.data_ptr(), 4096, y.data_ptr(), ldy, ydt, 4, d, g.data_ptr(), 0, 0, 0, 0, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (d, ldy, ydt, rc)
        assert _all_sent(y)


# ------------------------------------------------------------------------------------------------------------- rope
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["interleaved", "half"])
@pytest.mark.parametrize("rows,nheads", ROPE_CASES)
def test_rope_wrap_offset_stride(L, rows, nheads, layout, dt):
    """The stand-alone kernel on several batch elements: position = 5 + row % 7 on a 12-row table (the last table row is reached, the position
    wraps at least twice), row_stride = nheads * 64 + 16, both layouts and dtypes; (100, 16) and (101, 16) run 50 full blocks and 50 and a half.
    The 16 columns behind the heads and the rows past `rows` come back bit for bit."""
    bf = dt == torch.bfloat16
    c = rope_case(rows, nheads, layout, bf)
    buf = c["z"].to(DEV, dt)
    L.rope(buf, rows=rows, row_stride=c["stride"], nheads=nheads, rows_per_batch=c["rpb"], pos_offset=c["off"], table=c["tab"].to(DEV), layout=layout)
    got, before = buf.cpu(), c["z"].to(dt)
    assert _same_bits(got[rows:], before[rows:]) and _same_bits(got[:rows, nheads * 64:], before[:rows, nheads * 64:])
    hc = nheads * 64
    ref, mag = c["ref"][:, :hc], c["mag"][:, :hc]
    _report("rope", "bf16" if bf else "f32", "rows=%d heads=%d layout=%d" % (rows, nheads, layout), got[:rows, :hc], ref,
            tol_rope(mag, ref if bf else None))


def test_rope_refusals(L):
    buf = torch.randn(4, 64, generator=_g(2)).to(DEV)
    tab = _rope_table(4).to(DEV)
    before = buf.clone()
    for dtype, layout in [(L.F32, 2), (L.BF16_SPLIT, 0)]:
        rc = L.lib().v2a_rope_inplace(buf.data_ptr(), dtype, 4, 64, 1, 4, 0, tab.data_ptr(), layout, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (dtype, layout, rc)
        assert torch.equal(buf, before)


# ------------------------------------------------------------------------------------------------------------- linear_small, fill_registers
@pytest.mark.parametrize("K,d,bias,add,regs,shadow,dup", LIN_CASES)
@pytest.mark.parametrize("form", list(LIN_FORMS))
def test_linear_small(L, form, K, d, bias, add, regs, shadow, dup):
    """Both launch forms through the dispatch rule (2 rows per block at 3 clips, 8 rows at 256 clips with a block of register and data rows or a
    last block with an empty row), K from 1 to the admitted 2048, d of one lane, 16 lanes and a second column group per thread, every option on
    and off, out_batch_stride 8 floats longer than the rows.
    K = 1032 and 2048 on the 8-row forms ask for more than 64 KB of LDS (66 and 128 KB): the launch raises the kernel's limit first."""
    c = lin_case(form, K, d, bias, add, regs, dup)
    B, T, R, stride = c["B"], c["T"], c["R"], c["stride"]
    nb = B + c["dup"]
    dv = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    out = _sent((nb + 1, stride))
    sh = _sent((nb + 1, stride), torch.bfloat16) if shadow else None
    L.linear_small(c["a"].to(DEV), c["w"].to(DEV), dv(c["bias"]), dv(c["add"]), out, M=B * T, K=K, T=T, out_batch_stride=stride, row_off=R, d=d,
                   dup=c["dup"], regs=c["regs"].to(DEV) if regs else None, out_bf16=sh)
    got = out.cpu()
    wr = c["written"]
    assert _all_sent(got[nb:]) and _all_sent(got[:nb][~wr])                  # the batch past the last, the stride padding, unfused register rows
    _report("linear_small", form, "K=%d d=%d %s" % (K, d, "".join(n for n, f in zip("barsd", (bias, add, regs, shadow, dup)) if f)),
            got[:nb][wr], c["ref"][wr], tol_linear(K, c["mag"])[wr])
    if c["dup"]:
        assert _same_bits(got[:B], got[B:nb])
    if shadow:
        s = sh.cpu()
        assert _all_sent(s[nb:]) and _all_sent(s[:nb][~wr])
        assert _same_bits(s[:nb][wr], got[:nb][wr].bfloat16())
    if not regs:
        # the register rows by their own kernel into the same strided buffer: exact copies, nothing else touched
        L.fill_registers(out, c["regs"].to(DEV), B=nb, R=R, d=d, out_batch_stride=stride)
        after = out.cpu()
        assert _same_bits(after[:nb, :R * d], c["regs"].reshape(1, -1).expand(nb, -1).contiguous())
        assert _same_bits(after[:, R * d:], got[:, R * d:]) and _all_sent(after[nb:])


def test_linear_small_refusals(L):
    """K = 2049 is past what the argument check admits; d = 6 has no float4."""
    a, w, out = torch.zeros(8, 2049, device=DEV), torch.zeros(2049, 8, device=DEV), _sent((8, 8))
    for K, d in [(2049, 4), (4, 6)]:
        rc = L.lib().v2a_linear_small(a.data_ptr(), 8, K, w.data_ptr(), 0, 0, 8, out.data_ptr(), 64, 0, d, 0, 0, 0, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and _all_sent(out), (K, d, rc)


# ------------------------------------------------------------------------------------------------------------- time_cond
@pytest.mark.parametrize("S", TC_S)
@pytest.mark.parametrize("d", TC_WIDTHS)
def test_time_cond(L, d, S):
    """One and four column blocks, a column block with a tail (130, 384), d = 2, one grid point and 33 (t = 0 and 1 among them).

    Tolerance, for out = silu(z), z = b_n + sum_k e_k w_kn over the d + 1 entries e = [t, sin f, cos f]:
      1. the sum.  In any order it is within (d + 4) u (|b_n| + sum_k |e_k| |w_kn|): d + 1 products, the bias.  On the small configuration
         (d = 128) that alone is 5.5e-5, looser than the 2e-5 test_time_cond_golden allows there, so the sum is bounded in the order the
         kernel keeps -- acc = b_n, then acc += e_k w_kn for k = 0 .. d, which the compiler may contract but not reorder: every step rounds the
         new partial sum s_k once (|s_k| u) and, where the product is not contracted into an FMA, the product once (|e_k w_kn| u):
         u (sum_k |s_k| + sum_k |e_k| |w_kn|), partial sums from the float64 reference.  It is never above the order-free bound
         (|s_k| <= |b_n| + sum |e| |w|), and the whole tolerance stays under 2e-5 on the small configuration (both asserted in
         test_rowops_refs.py);
      2. sinf / cosf of the device library: within 4 ulp (the bound OpenCL sets for sin and cos, which the device library is built to; its
         range reduction keeps that near the zeros for |f| <= 2 pi * 5 here), so |delta e_k| <= 4 * 2^-23 |e_k| = 8 u |e_k| and
         |delta z| <= 8 u sum_k |e_k| |w_kn| more;  the argument f itself is formed in fp32 by the reference exactly as by the kernel;
      3. silu: |silu'| <= 1.1 carries delta z into the output;  z / (1 + __expf(-z)): the fast exponential is exp2(-z log2 e) with a rounded
         product (|z| u relative in the result), a rounded constant (|z| u) and a 1-ulp v_exp_f32 (2 u), the sum 1 + E rounds once (u) and the
         division is within 2.5 ulp (5 u): at most (2 |z| + 8) u |out|.
    Together 1.1 u (sum_k |s_k| + 9 sum_k |e_k| |w_kn|) + (2 |z| + 8) u |out|."""
    c = tc_case(d, S)
    out = _sent((S + 1, d))
    L.time_cond(c["t"].to(DEV), c["fw"].to(DEV), c["wt"].to(DEV), c["bias"].to(DEV), out, S=S, d=d)
    got = out.cpu()
    assert _all_sent(got[S:])
    _report("time_cond", "S=%d" % S, "d=%d" % d, got[:S], c["ref"], tol_time_cond(c))


# ------------------------------------------------------------------------------------------------------------- apg_reduce, cfg_euler
def _apg_kw(c):
    return dict(B=c["B"], T=c["T"], C_=c["C"], pred_batch_stride=c["pbs"], row_off=c["row_off"])


def _apg_launch(L, c, pred, valid):
    apg = torch.tensor([1e300, -7.0] * c["B"], dtype=torch.float64, device=DEV)      # garbage: the call itself zeroes it
    L.apg_reduce(pred, apg, valid_rows=None if valid is None else _i32(valid), **_apg_kw(c))
    return apg


@pytest.mark.parametrize("valid", APG_VALID)
def test_apg_reduce_valid_rows(L, valid):
    """valid_rows absent, 0, 1, T - 1, T, past T and negative: the sums cover rows [0, min(T, max(0, valid))) of every clip, over more elements
    than 64 blocks take in one pass, on a pred with row_off = 4 and a padded batch stride, into a buffer that held garbage."""
    c = apg_case()
    got = _apg_launch(L, c, c["flat"].to(DEV), valid).cpu().reshape(c["B"], 2)
    ref = _apg_sums_ref(c["pc"], c["pn"], valid)
    _report("apg_reduce", "valid_rows", "valid=%s" % valid, got, ref, 1e-12 * ref.abs())


@pytest.mark.parametrize("apg_on", [False, True], ids=["plain", "apg"])
@pytest.mark.parametrize("keep", [0.0, 0.3])
@pytest.mark.parametrize("step", [None, 2])
def test_cfg_euler(L, step, keep, apg_on):
    """413 blocks of float4, dt taken at step[0] = 2 of three entries or at 0 without a step, with and without the projection."""
    c = apg_case()
    h = EULER_DT[0 if step is None else step]
    pred = c["flat"].to(DEV)
    n = c["y"].numel()
    y = _sent((n + 64,))
    y[:n] = c["y"].reshape(-1).to(DEV)
    apg = _apg_launch(L, c, pred, None) if apg_on else None
    L.cfg_euler(y, pred, cfg_strength=EULER_S, dt=torch.tensor(EULER_DT, device=DEV), step=None if step is None else _i32(step), apg=apg, keep=keep,
                **_apg_kw(c))
    got = y.cpu()
    assert _all_sent(got[n:])
    ref, par = _euler_ref(c["y"], c["pc"], c["pn"], h, EULER_S, _apg_sums_ref(c["pc"], c["pn"], None) if apg_on else None, keep)
    _report("cfg_euler", "apg" if apg_on else "plain", "step=%s keep=%g" % (step, keep), got[:n].reshape(c["y"].shape), ref,
            tol_euler(c["y"], c["pc"], c["pn"], par, h, EULER_S))


def test_cfg_euler_zero_prediction_and_no_valid_rows(L):
    """A clip whose conditional prediction is all zero takes the 1e-12 branch of the projection: its update is finite and y + dt s (-pn).
    valid_rows = [0] leaves both sums 0 for every clip: the update is finite, with no projection applied."""
    c = apg_case(zero_clip=True)
    assert float(c["pc"][1].abs().max()) == 0.0
    pred, h = c["flat"].to(DEV), EULER_DT[0]
    for name, valid in (("zero clip", None), ("valid_rows=0", 0)):
        y = c["y"].to(DEV).clone()
        apg = _apg_launch(L, c, pred, valid)
        L.cfg_euler(y, pred, cfg_strength=EULER_S, dt=torch.tensor(EULER_DT, device=DEV), step=None, apg=apg, keep=0.3, **_apg_kw(c))
        sums = _apg_sums_ref(c["pc"], c["pn"], valid)
        assert float(sums[1].abs().max()) == 0.0 and (valid is None or float(sums.abs().max()) == 0.0)
        ref, par = _euler_ref(c["y"], c["pc"], c["pn"], h, EULER_S, sums, 0.3)
        if valid == 0:                                                       # no projection: the plain CFG update
            assert torch.equal(ref, _euler_ref(c["y"], c["pc"], c["pn"], h, EULER_S, None, 0.0)[0])
        assert torch.equal(ref[1], c["y"][1].double() + h * (EULER_S * -c["pn"][1].double()))
        _report("cfg_euler", "degenerate", name, y.cpu(), ref, tol_euler(c["y"], c["pc"], c["pn"], par, h, EULER_S))


# ------------------------------------------------------------------------------------------------------------- split_bf16, cast_bf16
@pytest.mark.parametrize("d", SPLIT_WIDTHS)
def test_split_bf16_ties_and_strides(L, d):
    """Rounding ties of both parities, their fp32 neighbours, +-0, negative lo, 2^-100 and 1e30 among randn, on d = 4 and 260 with ldx = d + 4
    and ldy = 2 d + 8: hi == bf16(x) and lo == bf16(x - hi) as torch rounds on the CPU, bit for bit, sentinels in the padding."""
    rows, ldx, ldy = SPLIT_ROWS, d + 4, 2 * d + 8
    x = torch.randn(rows, ldx, generator=_g(900 + d))
    x[:, :d] = bf16_values(rows * d, 901 + d).reshape(rows, d)
    y = _sent((rows + 1, ldy), torch.bfloat16)
    L.split_bf16(x.to(DEV), y, rows=rows, d=d, ldx=ldx, ldy=ldy)
    got = y.cpu()
    assert _all_sent(got[rows:]) and _all_sent(got[:rows, 2 * d:])
    hi = x[:, :d].bfloat16()
    assert _same_bits(got[:rows, :d], hi)
    assert _same_bits(got[:rows, d:2 * d], (x[:, :d] - hi.float()).bfloat16())
    print("rowops %-13s %-20s %-44s bit for bit" % ("split_bf16", "ties", "d=%d" % d))


@pytest.mark.parametrize("n", CAST_N)
def test_cast_bf16_ties(L, n):
    """The same values through v2a_cast_bf16 at one thread, a partial block and 293 blocks: bit equality with torch's conversion."""
    x = bf16_values(n, 950 + n)
    y = _sent((n + 8,), torch.bfloat16)
    L.cast_bf16(x.to(DEV), y[:n])
    got = y.cpu()
    assert _all_sent(got[n:])
    assert _same_bits(got[:n], x.bfloat16())
    print("rowops %-13s %-20s %-44s bit for bit" % ("cast_bf16", "ties", "n=%d" % n))


def test_split_and_cast_refusals(L):
    x = torch.zeros(4, 64, device=DEV)
    y = _sent((4, 64), torch.bfloat16)
    lib, s = L.lib(), L.stream_ptr()
    assert lib.v2a_split_bf16(x.data_ptr(), 64, y.data_ptr(), 64, 4, 6, s) == ERR_ARG               # d = 6
    assert lib.v2a_split_bf16(x.data_ptr(), 64, y.data_ptr(), 2 * 16 - 4, 4, 16, s) == ERR_ARG      # ldy = 2 d - 4
    assert lib.v2a_cast_bf16(x.data_ptr(), y.data_ptr(), 6, s) == ERR_ARG                           # n = 6
    torch.cuda.synchronize()
    assert _all_sent(y)
