"""GPU: the encoder-side kernels -- v2a_clip_embed_init, v2a_clip_layernorm, v2a_clip_attention (csrc/clip.hip), v2a_t5_rmsnorm, v2a_t5_attention,
v2a_gemm_skinny_f32 (csrc/t5.hip) -- against plain float64 restatements of the formulas in include/v2a_cfm.h, at the sizes, strides and masks the
encoder tests (test_clip_gpu.py, test_t5_gpu.py, test_dinov2_gpu.py) do not reach, and the DINOv2 encoder run through v2a_clip_attention.

Every reference below takes the fp32 inputs converted to double; none calls the oracle module or a kernel (tests/test_encoder_kernels_refs.py
checks them on the CPU against torch, Python loops and test_t5_gpu._attn_ref, and checks that no tolerance is loose enough to hide a wrong lane).
Inputs come from seeded CPU generators, are made once per case (the _CASES cache) and never modified.  Every output buffer is prefilled with SENT,
and whatever the header says a call does not write -- padding columns, rows past `rows`, the columns past H * d_head or past d in each half of a
split row, the padding between batch elements -- must still hold it bit for bit.  u = 2^-24 is the fp32 unit roundoff; "half a bf16 ulp" is
test_rowops_gpu._half_ulp_bf16.  The calls go through the C ABI wherever the Python wrapper cannot express a stride.

Tolerances (per element, from the float64 reference; where the reference is exactly 0 the result must be exactly 0):

  layernorm fp32   y = (x - m) r g + b, r = 1 / sqrt(var + eps).
                   mean: a lane adds up to 4 float4 as ((x + y) + (z + w)) onto its sum (6 roundings on the longest path), 6 shuffle adds, 2 adds
                   of the four wave sums, the division: |dm| <= 16 u mean|x|.
                   centred squares: the same tree over e^2 (7 + 6 + 2), / d, + eps, and 2 u for the rounded e = x - m in each square: 19 u on
                   var + eps, halved by the square root, then sqrtf and the division at 1 ulp (2 u) each instead of the half ulp of a correctly
                   rounded one: 14 u on r.  The common shift dm of every e moves var by dm^2 only (sum e = 0): + dm^2 / (2 (var + eps)) on r.
                   x - m and (x - m) r round once each (2 u), the final FMA rounds the result (u |y|).  Together
                     |g| r (dm + (16 u + dm^2 / (2 (var + eps))) |x - m|) + u |ref|,       dm = 16 u mean|x|.
                   The first term dominates the mean-100 row (|x - m| ~ 1 against mean|x| = 100).  A one-pass variance E[x^2] - m^2 in fp32 rounds
                   two numbers near 1e4 and subtracts them, an error of up to 1e4 u on a variance of 1, hundreds of times this bound on r
                   (test_encoder_kernels_refs.py applies that mutation).
                   A constant 0.5 row and a zero row have exact sums and an exact mean: e = 0, y = beta bit for bit.
  layernorm split  the planes equal the planes of the fp32 launch's result bit for bit (hi = bf16(y), lo = bf16(y - hi)); hi against the
                   reference: + half a bf16 ulp of ref; hi + lo: + 2^-16 |ref| (the format terms of test_rowops_gpu.py).
  embed_init       bit equality with the fp32 sum pos[r % T] (+ cls): one addition.
  t5 rmsnorm       24 u |ref|, derived as the rowops rmsnorm bound is: the sum of squares is at most 4 FMA-contracted squares and an add per
                   float4, 4 float4 per lane, 6 shuffle adds, 2 adds of the wave sums, / d and + eps: 18 u, halved by the square root; sqrtf
                   and the division at 1 ulp (2 u) each; two products: 15 u.  The rest is room for a 2.5-ulp division.  A zero row gives exact
                   zeros; resid is the gathered row bit for bit.
  attention        z_j = scale (q . k_j) (+ bias for T5), A_j = scale sum |q| |k_j| (+ |bias|), p = softmax(z), o = sum_j p_j v_j,
                   R = max_j z_j - min_j z_j over the keys that enter, nb the key blocks (32 keys CLIP, 64 T5), D the head dim.
                   score: a lane's FMA chain over at most min(D, 28) (16) non-zero products, 2 quad adds, the product by scale * log2(e) (its
                   own two roundings and the product's) or the bias add: (D + 6) u A_j in any order.
                   weight: the subtraction of the running max rounds once (u R relative on the weight), exp2f / expf at 3 ulp (6 u: the bound
                   OpenCL sets for exp and exp2, which the device library is built to); every later block rescales by one more such
                   exponential and one product: (nb + 1) (R + 7) u.  eta = (D + 6) u max_j A_j + (nb + 1) (R + 7) u bounds the relative error of
                   every unnormalised weight.  The running max itself cancels between numerator and denominator.
                   With weights w_j (1 + eta_j), |eta_j| <= eta, the normalised weights move by at most 2 eta / (1 - eta) relative, and since
                   they still sum to 1 the output moves by at most that times S1 = sum_j p_j |v_j - o|.
                   sums: N FMAs on the numerator (N u S2, S2 = sum_j p_j |v_j|), N adds on the denominator, the division at 1 ulp and the
                   final product ((N + 3) u |o|).  Together
                     2 eta / (1 - eta) S1 + N u S2 + (N + 3) u |o|.
                   A T5 batch row without a valid key is exactly 0 (the reference is 0 there, the bound is 0).
  attention split  as layernorm split, against the fp32 launch of the same case.
  skinny GEMM      (K + 3) u (sum_k |a| |w| + |bias| + |resid|): a sum of K products and two more terms in any order (the 8 waves' K shares
                   and the fixed-order LDS sum are one such order).  GEGLU_TANH, out = v G(g), G = gelu_new: with tv, tg the bounds of the value
                   and the gate, |G'| <= 1.13, and G evaluated in fp32 within 4 u |g| + 2 u |G| (the argument of tanh within 5 u relative, where
                   |t| sech^2 t <= 0.45; tanhf at 2 ulp, 4 u absolute since |tanh| <= 1; the sum 1 + tanh, the products by 0.5 and g):
                     |G| tv + (|v| + tv) (1.13 tg + 4 u |g| + 2 u |G|) + u |ref|.
                   Row 0 has the same bits for every M at a given K, N and epilogue, as the header promises.

The existing bars on the shapes the existing tests run (test_encoder_kernels_refs.py, test_bounds_against_the_existing_bars).  The layernorm bound
stays under 2e-6 max|y| on test_clip_gpu.py's own d = 1664 input (1.0e-6).  The other three bars are measured figures of errors that grow as the
square root of the operation count, and no worst-case bound of the forms above can be under them, whatever the inputs:
  v2a_clip_attention   the N FMAs of the p.v sum alone allow N u sum p |v| >= N u |o|: 1.5e-5 at N = 257 and 3.4e-5 at N = 577, against 2e-6;
  v2a_gemm_skinny_f32  (K + 3) u sum |a| |w| >= (K + 3) u |ref|: 7.8e-6 at K = 128 against 4e-6, 1.7e-4 at K = 2816 against 1.9e-5;
  v2a_t5_attention     on this file's inputs at N = 7 .. 512 the bound is 2.4e-4 .. 4.4e-4 against 5e-5 .. 7e-5 (at N = 1 9e-7: inside).
The refs file asserts these inequalities as they stand, so that nobody reads the derived bounds as tighter than they are; what holds the kernels
to a sharper line than the old bars is that the bounds are per element (a wrong small output no longer hides under max|y|), the bit equalities
and the sentinels.

Read out of the code before these tests ran, and what the run showed:
  v2a_clip_attention   the staging loop zero-fills the dims past d_head and the keys past N, the q load and the store skip whole float4 past
                       d_head, a query past N is computed on row N - 1 and not stored: nothing to fix, and no case missed its bound (fp32 at
                       0.11 of it at most).
  v2a_clip_layernorm   the variance is the centred second pass over the registers, as the header says; the constant and zero rows came out as
                       beta bit for bit at every width.  Nothing missed.
  v2a_t5_attention     the `continue` on a masked key block depends on the batch row's mask and the block alone, so the whole workgroup takes it
                       and meets at the next barrier; the first live block after masked ones rescales l = 0 and o = 0 by expf(-inf) = 0.  The
                       row without a key came out as exact zeros.  Nothing missed.
  v2a_gemm_skinny_f32  "RESID (resid may alias out)" holds for ldr = ldo only: with two strides on one buffer a row's residual is another
                       row's output, written by another workgroup.  The entry point does not refuse that and the engine never asks for it;
                       the in-place case here uses one stride, the two-stride case a residual of its own.  Nothing missed.
  v2a_t5_rmsnorm, v2a_clip_embed_init: nothing missed.
No kernel missed a bound, and csrc/clip.hip and csrc/t5.hip are unchanged.

Every case prints "encoder <kernel> <group> <case> max |got - ref| / tol = <ratio>" before it asserts ratio <= 1, and the module prints the
largest ratio per (kernel, group) when it is done (pytest -s); profiles/encoder_kernels_parity.txt records them as first measured on the MI355X."""
import ctypes
import math

import pytest
import torch

from test_rowops_gpu import _half_ulp_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = -7.25                     # exact in fp32 and in bf16
ERR_ARG = -1                     # V2A_ERR_ARG
EXP_ULP_U = 6                    # exp2f / expf: 3 ulp = 6 u
GELU_SLOPE = 1.13                # max |gelu_new'|

# ---- v2a_clip_attention
CA_B, CA_H = 2, 3
CA_DHEADS = [4, 28, 32, 64, 104, 108, 112]            # one lane, exactly one lane, a float4 into the second, ..., all four lanes full
CA_DHEAD_N = [33, 65]                                 # one key past a key block; one query past a query block
CA_NS = [1, 31, 32, 33, 64, 65, 129]
CA_N_DHEADS = [64, 104]
CA_SHAPES = sorted({(D, N) for D in CA_DHEADS for N in CA_DHEAD_N} | {(D, N) for D in CA_N_DHEADS for N in CA_NS})
CA_LARGE = dict(D=64, N=129, first=5, last=128)       # the dominant key in key block 0, or alone in key block 4 (the last of 5)
# ---- v2a_clip_layernorm
LN_WIDTHS = [4, 384, 1020, 1024, 1028, 1664, 4096]    # one lane, two idle waves, the last lane of float4 0 idle, full, one lane into float4 1, ...
LN_ROWS = 5
LN_PLAIN, LN_OUTLIER, LN_CONST, LN_MEAN100, LN_ZERO = range(5)
LN_EPS = 1e-5
# ---- v2a_clip_embed_init
EI_CASES = [(T, d) for T in (1, 5) for d in (4, 260)]
# ---- v2a_t5_rmsnorm
TR_WIDTHS = [4, 512, 1020, 1024, 1028, 2048, 4096]
TR_ROWS, TR_VOCAB, TR_EPS = 8, 11, 1e-6
TR_IDS = [0, 10, 3, 7, 3, 10, 1, 0]                   # 0 and vocab - 1, repeats, table row 3 is zero
TR_ZERO = 3                                           # the zero row of x / of the table
# ---- v2a_t5_attention
TA_B, TA_H = 4, 2
TA_NS = [1, 63, 64, 65, 128, 129]
TA_ALL, TA_LAST, TA_FIRST, TA_NONE = range(4)         # the mask of each batch row
# ---- v2a_gemm_skinny_f32
SK_MS = [1, 16, 17, 32, 33, 64, 65]
SK_KS = [32, 64, 96, 224, 288]                        # S = K / 32 = 1, 2, 3, 7, 9 steps over 8 waves
SK_NS = [16, 48]                                      # output columns (GEGLU_TANH: 32 and 96 packed rows)
SK_MMAX = 65
SK_SHAPES = [(M, 96, 48) for M in SK_MS] + [(17, K, 16) for K in SK_KS if K != 96] + [(33, 288, 48)]
SK_EPIS = ["store", "resid", "resid_inplace", "geglu_tanh"]


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- float64 reference helpers
def _layernorm_ref(x, g, b, eps):
    """y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance; x (rows, d) fp32."""
    x = x.double()
    m = x.mean(-1, keepdim=True)
    e = x - m
    var = (e * e).mean(-1, keepdim=True)
    return e / torch.sqrt(var + eps) * g.double() + b.double()


def _embed_ref(rows, T, cls, pos):
    """fp32: h[r] = pos[r % T] + (cls if r % T == 0), one fp32 addition."""
    t = torch.arange(rows) % T
    return torch.where((t == 0)[:, None], pos[t] + cls[None, :], pos[t])


def _t5_rmsnorm_ref(x, w, eps):
    """y = w * x * rsqrt(mean(x^2) + eps); x (rows, d) fp32."""
    x = x.double()
    return w.double() * (x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps))


def _attn_ref(q, k, v, scale, bias=None, mask=None):
    """softmax_j(scale q_i . k_j + bias[h][j - i + N - 1] | mask[b][j]) v_j in float64; q, k, v (B, N, H, D) fp32, bias (H, 2N - 1), mask (B, N).
    A batch row without a valid key gives 0.  Returns dict(o, S1 = sum_j p_j |v_j - o|, S2 = sum_j p_j |v_j|, A = max_j scale sum |q| |k_j|
    (+ |bias|), R = the range of the scores that enter), o / S1 / S2 as (B, N, H * D), A / R as (B, N, H)."""
    B, N, H, D = q.shape
    q, k, v = q.double(), k.double(), v.double()
    z = scale * torch.einsum("bihd,bjhd->bhij", q, k)
    a = scale * torch.einsum("bihd,bjhd->bhij", q.abs(), k.abs())
    if bias is not None:
        idx = torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1
        z, a = z + bias.double()[:, idx][None], a + bias.double().abs()[:, idx][None]
    live = torch.ones(B, 1, 1, N, dtype=torch.bool) if mask is None else mask.bool()[:, None, None, :]
    live = live.expand(B, H, N, N)
    zm = torch.where(live, z, torch.full_like(z, -math.inf))
    top = zm.max(-1, keepdim=True).values
    w = torch.where(live, torch.exp(z - torch.where(torch.isfinite(top), top, torch.zeros_like(top))), torch.zeros_like(z))
    den = w.sum(-1, keepdim=True)
    p = torch.where(den > 0, w / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(w))
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    S2 = torch.einsum("bhij,bjhd->bihd", p, v.abs())
    S1 = torch.empty_like(o)
    for b in range(B):
        for h in range(H):
            S1[b, :, h] = torch.einsum("ij,ijd->id", p[b, h], (v[b, None, :, h] - o[b, :, None, h]).abs())
    A = torch.where(live, a, torch.zeros_like(a)).max(-1).values
    R = top[..., 0] - torch.where(live, z, torch.full_like(z, math.inf)).min(-1).values
    R = torch.where(torch.isfinite(R), R, torch.zeros_like(R))
    flat = lambda t: t.reshape(B, N, H * D)   # noqa: E731
    return dict(o=flat(o), S1=flat(S1), S2=flat(S2), A=A.permute(0, 2, 1), R=R.permute(0, 2, 1))


def _gelu_new(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def _skinny_ref(a, w, bias, resid, epi):
    """acc = a w^T (+ bias) (+ resid); GEGLU_TANH: W rows and bias packed [16 value | 16 gate] per 16 outputs, out = v gelu_new(g).
    Returns (ref, tol) in float64; a (M, K), w (N, K) fp32."""
    K = a.shape[1]
    acc = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    if bias is not None:
        acc, mag = acc + bias.double(), mag + bias.double().abs()
    if epi in ("resid", "resid_inplace"):
        acc, mag = acc + resid.double(), mag + resid.double().abs()
    t = (K + 3) * U * mag
    if epi != "geglu_tanh":
        return acc, t
    M, N = acc.shape
    acc, t = acc.view(M, N // 32, 2, 16), t.view(M, N // 32, 2, 16)
    v, g, tv, tg = (x.reshape(M, N // 2) for x in (acc[:, :, 0], acc[:, :, 1], t[:, :, 0], t[:, :, 1]))
    G = _gelu_new(g)
    ref = v * G
    return ref, G.abs() * tv + (v.abs() + tv) * (GELU_SLOPE * tg + 4 * U * g.abs() + 2 * U * G.abs()) + U * ref.abs()


# ------------------------------------------------------------------------------------------------------------- tolerances
def tol_layernorm(x, g, ref, eps):
    x = x.double()
    d = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    e = x - m
    ve = (e * e).mean(-1, keepdim=True) + eps
    dm = 16 * U * x.abs().sum(-1, keepdim=True) / d
    return g.double().abs() / torch.sqrt(ve) * (dm + (16 * U + dm * dm / (2 * ve)) * e.abs()) + U * ref.abs()


def tol_split_hi(tol, ref):
    return tol + _half_ulp_bf16(ref)


def tol_split_sum(tol, ref):
    return tol + 2.0 ** -16 * ref.abs()


def tol_t5_rmsnorm(ref):
    return 24 * U * ref.abs()


def tol_attention(r, D, N, key_block):
    """r: what _attn_ref returns."""
    nb = (N + key_block - 1) // key_block
    eta = ((D + 6) * U * r["A"] + (nb + 1) * (r["R"] + 1 + EXP_ULP_U) * U).repeat_interleave(D, -1)
    return 2 * eta / (1 - eta) * r["S1"] + N * U * r["S2"] + (N + 3) * U * r["o"].abs()


# ------------------------------------------------------------------------------------------------------------- cases, made once on the CPU
_CASES = {}


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _carve(flat, B, N, rs, bs, off, H, D):
    """The (B, N, H, D) view of a flat buffer at base off, row stride rs, batch stride bs."""
    return flat[off:].as_strided((B, N, H, D), (bs, rs, D, 1))


def ca_case(D, N, kind="plain"):
    """q, k, v carved from one buffer with row_stride = 3 H D + 8 and batch_stride = N row_stride + 4, every float of it random (the padding must
    not enter).  plain: q, k ~ N(0, 1), v ~ 0.5 + N(0, 1) (a mean, so that the outputs of 129 nearly even weights do not shrink to the bound's own
    size), scale = D^-0.5.  first / last: scale = 1 and q . k_j = 200 + 1.1 n_j, + 12 on the dominant key of key block 0 or of the last key block --
    q and every k are a multiple of one unit vector plus small noise, so that sum |q| |k| is about |q . k|."""
    def make():
        B, H = CA_B, CA_H
        rs = 3 * H * D + 8
        bs = N * rs + 4
        g = _g(1000 + 13 * D + N + {"plain": 0, "first": 1, "last": 2}[kind])
        flat = torch.randn(B * bs + 8, generator=g)
        q, k, v = (_carve(flat, B, N, rs, bs, i * H * D, H, D) for i in range(3))
        scale = D ** -0.5
        if kind != "plain":
            scale = 1.0
            e = torch.full((D,), D ** -0.5)
            dom = torch.zeros(N)
            dom[CA_LARGE[kind]] = 1.0
            q.copy_(10 * e * (1 + 0.02 * torch.randn(B, N, H, 1, generator=g)) + 0.1 * torch.randn(B, N, H, D, generator=g))
            k.copy_((20 + 0.1 * torch.randn(B, N, H, 1, generator=g) + 1.2 * dom[None, :, None, None]) * e + 0.05 * torch.randn(B, N, H, D, generator=g))
        else:
            v.add_(0.5)
        r = _attn_ref(q, k, v, scale)
        return dict(B=B, H=H, N=N, D=D, rs=rs, bs=bs, scale=scale, flat=flat, q=q, k=k, v=v, r=r, ref=r["o"], tol=tol_attention(r, D, N, 32))
    return _cached(("ca", D, N, kind), make)


def ln_rows(d, g):
    """The five rows of a layernorm case, (5, d) fp32."""
    x = torch.randn(LN_ROWS, d, generator=g) * 3 + 0.5
    x[LN_OUTLIER, [0, d // 2, d - 1]] *= 60
    x[LN_CONST] = 0.5
    x[LN_MEAN100] = 100 + torch.randn(d, generator=g)
    x[LN_ZERO] = 0
    return x


def ln_case(d):
    """x (5, d + 4) with the pad columns random: a plain row, one with three x60 outlier channels, a constant 0.5 row, a row of mean 100 and
    standard deviation 1, a zero row."""
    def make():
        g = _g(2000 + d)
        x = torch.randn(LN_ROWS, d + 4, generator=g)
        x[:, :d] = ln_rows(d, g)
        gam, bet = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
        ref = _layernorm_ref(x[:, :d], gam, bet, LN_EPS)
        return dict(d=d, ldx=d + 4, x=x, g=gam, b=bet, ref=ref, tol=tol_layernorm(x[:, :d], gam, ref, LN_EPS))
    return _cached(("ln", d), make)


def tr_case(d, gather, eps=TR_EPS):
    """x (8, d + 4) or a table (11, d + 4), pad columns random, row 3 zero (not with eps = 0), one row scaled by 1e-3, one by 1e3."""
    def make():
        g = _g(3000 + d + (1 if gather else 0))
        n = TR_VOCAB if gather else TR_ROWS
        x = 3 * torch.randn(n, d + 4, generator=g)
        if eps > 0:
            x[TR_ZERO, :d] = 0
        x[1] *= 1e-3
        x[7] *= 1e3
        w = 1 + 0.1 * torch.randn(d, generator=g)
        ids = torch.tensor(TR_IDS, dtype=torch.int32)
        rows = x[ids.long()] if gather else x
        ref = _t5_rmsnorm_ref(rows[:, :d], w, eps)
        return dict(d=d, ldx=d + 4, ldr=d + 8, ldy=d + 12, x=x, w=w, ids=ids if gather else None, rows=rows[:, :d], eps=eps, ref=ref,
                    tol=tol_t5_rmsnorm(ref))
    return _cached(("tr", d, gather, eps), make)


def ta_masks(N):
    m = torch.zeros(TA_B, N, dtype=torch.int32)
    m[TA_ALL] = 1
    m[TA_LAST, N - 1] = 1
    m[TA_FIRST, 0] = 1
    return m


def ta_case(N, large=False):
    """q, k, v in three buffers of their own with row strides H 64 + 8 / 16 / 24 and batch strides N row_stride + 4 / 8 / 12, every float random.
    plain: q, k ~ 0.5 N(0, 1), v, bias ~ N(0, 1).  large: q . k_j = 100 + 2.2 n_j (q and k multiples of one unit vector plus small noise), bias
    entries +50, -50 or N(0, 1) by thirds, v ~ 2 + 0.3 N(0, 1) (the bound on a score of magnitude 150 is 6e-4: the values' spread is kept small
    against their size so that it stays under 1e-3 of the outputs)."""
    def make():
        B, H, D = TA_B, TA_H, 64
        g = _g(4000 + N + (500 if large else 0))
        st = [(H * D + 8 * (i + 1), 4 * (i + 1)) for i in range(3)]
        st = [(rs, N * rs + pad) for rs, pad in st]
        flats = [torch.randn(B * bs + 8, generator=g) for rs, bs in st]
        q, k, v = (_carve(f, B, N, rs, bs, 0, H, D) for f, (rs, bs) in zip(flats, st))
        bias = torch.randn(H, 2 * N - 1, generator=g)
        if large:
            e = torch.full((D,), D ** -0.5)
            q.copy_(10 * e * (1 + 0.02 * torch.randn(B, N, H, 1, generator=g)) + 0.1 * torch.randn(B, N, H, D, generator=g))
            k.copy_((10 + 0.2 * torch.randn(B, N, H, 1, generator=g)) * e + 0.1 * torch.randn(B, N, H, D, generator=g))
            v.mul_(0.3).add_(2.0)
            pick = torch.rand(H, 2 * N - 1, generator=g)
            bias = torch.where(pick < 1 / 3, torch.full_like(bias, 50.0), torch.where(pick < 2 / 3, torch.full_like(bias, -50.0), bias))
        else:
            q.mul_(0.5)
            k.mul_(0.5)
        mask = ta_masks(N)
        r = _attn_ref(q, k, v, 1.0, bias, mask)
        return dict(B=B, H=H, N=N, st=st, flats=flats, q=q, k=k, v=v, bias=bias, mask=mask, r=r, ref=r["o"], tol=tol_attention(r, D, N, 64))
    return _cached(("ta", N, large), make)


def sk_case(K, N, M=SK_MMAX):
    """a (M, K + 4), w (N, K + 8) (and a packed (2 N, K + 8) for GEGLU_TANH), resid (M, N + 8), bias (N,) and (2 N,), pad columns random;
    a ~ 0.35 + N(0, 1), w ~ (0.35 + N(0, 1)) / sqrt(K): the means keep the sums from cancelling down to the size of the bound, which grows as K
    against sqrt(K) for a sum of signed terms (the value and the gate stay within a few units: gelu_new is not saturated).  The cases of one
    (K, N) use the first M rows of the same a."""
    def make():
        g = _g(5000 + 7 * K + N + M)
        a = 0.35 + torch.randn(M, K + 4, generator=g)
        w = 0.35 + torch.randn(2 * N, K + 8, generator=g)
        w[:, :K] /= math.sqrt(K)
        return dict(K=K, N=N, a=a, w=w, bias=torch.randn(2 * N, generator=g), resid=torch.randn(M, N + 8, generator=g))
    return _cached(("sk", K, N, M), make)


def sk_ref(K, N, M, epi, bias, Mfull=SK_MMAX):
    """(ref, tol) of the first M rows of sk_case(K, N): STORE / RESID use w[:N] and bias[:N], GEGLU_TANH the 2 N packed rows."""
    def make():
        c = sk_case(K, N, Mfull)
        nw = 2 * N if epi == "geglu_tanh" else N
        return _skinny_ref(c["a"][:, :K], c["w"][:nw, :K], c["bias"][:nw] if bias else None, c["resid"][:, :N], epi)
    ref, tol = _cached(("sk_ref", K, N, Mfull, epi, bias), make)
    return ref[:M], tol[:M]


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
    print("encoder %-15s %-18s %-40s max |got - ref| / tol = %.3f" % (kernel, group, case, ratio))
    assert ratio <= 1.0, (kernel, group, case, ratio)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nencoder kernels parity: largest |got - ref| / tol per kernel and case group")
    for (kernel, group), r in sorted(_WORST.items()):
        print("  %-15s %-18s %.3f" % (kernel, group, r))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sent(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def _all_sent(t):
    return bool((t == SENT).all())


def _split_checks(kernel, group, case, hi, lo, f32, ref, tol):
    """The planes are those of the fp32 launch's result, bit for bit; hi and hi + lo against the reference with the format terms."""
    assert _same_bits(hi, f32.bfloat16()), (kernel, case, "hi plane")
    assert _same_bits(lo, (f32 - f32.bfloat16().float()).bfloat16()), (kernel, case, "lo plane")
    _report(kernel, group + " hi", case, hi, ref, tol_split_hi(tol, ref))
    _report(kernel, group + " hi+lo", case, hi.double() + lo.double(), ref, tol_split_sum(tol, ref))


# ------------------------------------------------------------------------------------------------------------- v2a_clip_attention
def _ca_args(L, c, buf, out, split, ors, obs):
    a = L.ClipAttnArgs()
    hd = c["H"] * c["D"]
    a.q, a.k, a.v, a.out = buf.data_ptr(), buf.data_ptr() + 4 * hd, buf.data_ptr() + 8 * hd, out.data_ptr()
    a.row_stride, a.batch_stride, a.out_row_stride, a.out_batch_stride = c["rs"], c["bs"], ors, obs
    a.B, a.H, a.N, a.d_head, a.scale, a.out_split = c["B"], c["H"], c["N"], c["D"], c["scale"], split
    return a


def _ca_launch(L, c, split):
    """One launch into a sentinel buffer: fp32 rows of H D + 8 floats, split rows of 2 (H D + 8) bf16 (lo at H D + 8), 4 elements between the
    batch elements and 8 behind the last.  Returns the (B, N, H D) result, or the (hi, lo) planes."""
    B, N, hd = c["B"], c["N"], c["H"] * c["D"]
    half = hd + 8
    ors = 2 * half if split else half
    obs = N * ors + 4
    out = _sent((B * obs + 8,), torch.bfloat16 if split else torch.float32)
    buf = c["flat"].to(DEV)
    a = _ca_args(L, c, buf, out, split, ors, obs)
    L.check(L.lib().v2a_clip_attention(ctypes.byref(a), L.stream_ptr()))
    o = out.cpu()
    per = o[:B * obs].view(B, obs)
    rows = per[:, :N * ors].view(B, N, ors)
    assert _all_sent(o[B * obs:]) and _all_sent(per[:, N * ors:])                      # behind the last batch element, between batch elements
    if not split:
        assert _all_sent(rows[..., hd:])
        return rows[..., :hd].contiguous()
    assert _all_sent(rows[..., hd:half]) and _all_sent(rows[..., half + hd:])           # past H * d_head in each half
    return rows[..., :hd].contiguous(), rows[..., half:half + hd].contiguous()


def _ca_check(L, c, group, case):
    f32 = _ca_launch(L, c, 0)
    _report("clip_attention", group + " f32", case, f32, c["ref"], c["tol"])
    hi, lo = _ca_launch(L, c, 1)
    _split_checks("clip_attention", group, case, hi, lo, f32, c["ref"], c["tol"])


@pytest.mark.parametrize("D,N", CA_SHAPES)
def test_clip_attention_head_dims_and_lengths(L, D, N):
    """d_head from one float4 of one lane to all four lanes full (which lanes load q, which read zeros, which skip the store), at one key past
    a key block and one query past a query block; N on and around the 32-key and 64-query boundaries and over five key blocks at d_head 64 (the
    DINOv2 configuration) and 104; q, k, v carved from one padded buffer, out rows and batch elements padded, fp32 and split output."""
    _ca_check(L, ca_case(D, N), "shapes", "d_head=%d N=%d" % (D, N))


@pytest.mark.parametrize("kind", ["first", "last"])
def test_clip_attention_large_logits(L, kind):
    """scale = 1 and q . k around 200: the dominant key (+12) sits in the first key block, whose sums every later block must carry unscaled, or
    in the last, which must scale the four blocks before it down by e^-12."""
    c = ca_case(CA_LARGE["D"], CA_LARGE["N"], kind)
    _ca_check(L, c, "large logits", "dominant key %d of %d" % (CA_LARGE[kind], c["N"]))


def test_clip_attention_refusals(L):
    """d_head 116 (> 112) and 6 (no float4), N 0 and 4097, q four bytes off, an fp32 out row shorter than H * d_head: V2A_ERR_ARG, nothing written."""
    c = dict(ca_case(64, 33))
    buf = c["flat"].to(DEV)
    hd = c["H"] * 64
    out = _sent((c["B"] * 40 * 2 * hd,))
    for name, ch in [("d_head=116", dict(D=116)), ("d_head=6", dict(D=6)), ("N=0", dict(N=0)), ("N=4097", dict(N=4097)), ("q + 4 bytes", dict(qoff=4)),
                     ("out_row_stride", dict(ors=hd - 4))]:
        cc = dict(c, **{k: v for k, v in ch.items() if k in ("D", "N")})
        a = _ca_args(L, cc, buf, out, 0, ch.get("ors", hd + 8), 40 * (hd + 8))
        a.q += ch.get("qoff", 0)
        rc = L.lib().v2a_clip_attention(ctypes.byref(a), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (name, rc)
        assert _all_sent(out), name


# ------------------------------------------------------------------------------------------------------------- v2a_clip_layernorm
def _ln_launch(L, c, split, **over):
    d = c["d"]
    ldy = 2 * (d + 64) if split else d + 8
    y = _sent((LN_ROWS + 2, ldy), torch.bfloat16 if split else torch.float32)
    x, g, b = c["x"].to(DEV), c["g"].to(DEV), c["b"].to(DEV)
    L.check(L.lib().v2a_clip_layernorm(x.data_ptr(), c["ldx"], y.data_ptr(), ldy, L.BF16_SPLIT if split else L.F32, LN_ROWS, d, g.data_ptr(),
                                       b.data_ptr(), LN_EPS, L.stream_ptr()))
    y = y.cpu()
    assert _all_sent(y[LN_ROWS:])
    if not split:
        assert _all_sent(y[:LN_ROWS, d:])
        return y[:LN_ROWS, :d].contiguous()
    assert _all_sent(y[:LN_ROWS, d:d + 64]) and _all_sent(y[:LN_ROWS, d + 64 + d:])     # columns d .. ldy / 2 - 1 of each half
    return y[:LN_ROWS, :d].contiguous(), y[:LN_ROWS, d + 64:d + 64 + d].contiguous()


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_clip_layernorm_widths_and_rows(L, d):
    """d of one lane, of two idle waves, around the 1024 where the second float4 of a thread starts, the model's 1664 and the admitted 4096, with
    ldx = d + 4, ldy = d + 8 and split rows of 2 (d + 64); a constant row and a zero row come out as beta bit for bit, and the row of mean 100
    and deviation 1 is held to a bound that a one-pass variance misses."""
    c = ln_case(d)
    f32 = _ln_launch(L, c, False)
    _report("clip_layernorm", "widths f32", "d=%d" % d, f32, c["ref"], c["tol"])
    _report("clip_layernorm", "mean-100 row f32", "d=%d" % d, f32[LN_MEAN100], c["ref"][LN_MEAN100], c["tol"][LN_MEAN100])
    assert _same_bits(f32[LN_CONST], c["b"]) and _same_bits(f32[LN_ZERO], c["b"])
    hi, lo = _ln_launch(L, c, True)
    _split_checks("clip_layernorm", "widths", "d=%d" % d, hi, lo, f32, c["ref"], c["tol"])


def test_clip_layernorm_refusals(L):
    """d = 4100 (> 4096), d = 6 (no float4), a split row shorter than two planes: V2A_ERR_ARG, nothing written."""
    x = torch.randn(4, 4200, generator=_g(1)).to(DEV)
    g = torch.ones(4200, device=DEV)
    for d, ldy, ydt, dtype in [(4100, 4104, L.F32, torch.float32), (6, 8, L.F32, torch.float32), (64, 2 * 64 - 4, L.BF16_SPLIT, torch.bfloat16)]:
        y = _sent((4, 4200), dtype)
        rc = L.lib().v2a_clip_layernorm(x.data_ptr(), 4200, y.data_ptr(), ldy, ydt, 4, d, g.data_ptr(), g.data_ptr(), LN_EPS, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (d, ldy, ydt, rc)
        assert _all_sent(y)


# ------------------------------------------------------------------------------------------------------------- v2a_clip_embed_init
@pytest.mark.parametrize("T,d", EI_CASES)
def test_clip_embed_init(L, T, d):
    """rows = 2 T + 1 (the position wraps twice and ends on a class row), ldh = d + 4: h[r] = pos[r % T] (+ cls on class rows) in fp32, bit for bit."""
    g = _g(6000 + 10 * T + d)
    rows, ldh = 2 * T + 1, d + 4
    cls, pos = torch.randn(d, generator=g), torch.randn(T, d, generator=g)
    h, cd, pd = _sent((rows + 1, ldh)), cls.to(DEV), pos.to(DEV)
    L.check(L.lib().v2a_clip_embed_init(h.data_ptr(), ldh, rows, T, d, cd.data_ptr(), pd.data_ptr(), L.stream_ptr()))
    got = h.cpu()
    assert _all_sent(got[rows:]) and _all_sent(got[:rows, d:])
    assert _same_bits(got[:rows, :d].contiguous(), _embed_ref(rows, T, cls, pos))
    print("encoder %-15s %-18s %-40s bit for bit" % ("clip_embed_init", "rows", "T=%d d=%d" % (T, d)))


def test_clip_embed_init_refusal(L):
    h, v = _sent((4, 16)), torch.zeros(16, device=DEV)
    rc = L.lib().v2a_clip_embed_init(h.data_ptr(), 16, 4, 2, 6, v.data_ptr(), v.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and _all_sent(h)


# ------------------------------------------------------------------------------------------------------------- v2a_t5_rmsnorm
def _tr_launch(L, c):
    """ldx = d + 4, ldr = d + 8, ldy = d + 12 through the C ABI (the wrapper passes ldr = d).  Returns (y, resid or None) as (rows, d)."""
    d = c["d"]
    gather = c["ids"] is not None
    y, res = _sent((TR_ROWS + 1, c["ldy"])), _sent((TR_ROWS + 1, c["ldr"]))
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    ids = c["ids"].to(DEV) if gather else None
    L.check(L.lib().v2a_t5_rmsnorm(x.data_ptr(), c["ldx"], ids.data_ptr() if gather else 0, TR_VOCAB if gather else 0, res.data_ptr() if gather else 0,
                                   c["ldr"] if gather else 0, y.data_ptr(), c["ldy"], TR_ROWS, d, w.data_ptr(), c["eps"], L.stream_ptr()))
    y, res = y.cpu(), res.cpu()
    assert _all_sent(y[TR_ROWS:]) and _all_sent(y[:TR_ROWS, d:])
    assert _all_sent(res[TR_ROWS:]) and _all_sent(res[:TR_ROWS, d:]) and (gather or _all_sent(res))
    return y[:TR_ROWS, :d].contiguous(), res[:TR_ROWS, :d].contiguous() if gather else None


@pytest.mark.parametrize("gather", [False, True], ids=["rows", "gather"])
@pytest.mark.parametrize("d", TR_WIDTHS)
def test_t5_rmsnorm_widths_and_strides(L, d, gather):
    """d of one lane, of two waves, around the 1024 where a thread's second float4 starts, 2 and 4 float4 per thread; ldx, ldr and ldy all
    different; ids with 0, vocab - 1 and repeats; the zero row comes out exactly 0 (the reference is 0 there and _report demands equality); resid is
    the gathered row bit for bit."""
    c = tr_case(d, gather)
    y, res = _tr_launch(L, c)
    assert float(c["ref"][TR_IDS.index(TR_ZERO) if gather else TR_ZERO].abs().max()) == 0.0
    _report("t5_rmsnorm", "gather" if gather else "rows", "d=%d" % d, y, c["ref"], c["tol"])
    if gather:
        assert _same_bits(res, c["rows"].contiguous())


def test_t5_rmsnorm_eps_zero(L):
    c = tr_case(1028, False, eps=0.0)
    assert float(c["rows"].abs().sum(-1).min()) > 0
    y, _ = _tr_launch(L, c)
    _report("t5_rmsnorm", "eps=0", "d=1028", y, c["ref"], c["tol"])


def test_t5_rmsnorm_refusals(L):
    """ldx < d, a gather without resid, a negative eps: V2A_ERR_ARG, nothing written."""
    x, w, y, res = torch.zeros(16, 64, device=DEV), torch.ones(64, device=DEV), _sent((8, 64)), _sent((8, 64))
    ids = torch.zeros(8, dtype=torch.int32, device=DEV)
    for name, ldx, idp, resp, eps in [("ldx < d", 60, 0, 0, 1e-6), ("no resid", 64, ids.data_ptr(), 0, 1e-6), ("eps < 0", 64, 0, 0, -1e-6)]:
        rc = L.lib().v2a_t5_rmsnorm(x.data_ptr(), ldx, idp, 16 if idp else 0, resp, 64, y.data_ptr(), 64, 8, 64, w.data_ptr(), eps, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (name, rc)
        assert _all_sent(y) and _all_sent(res), name


# ------------------------------------------------------------------------------------------------------------- v2a_t5_attention
def _ta_args(L, c, bufs, out, bias, mask, ors, obs):
    a = L.T5AttnArgs()
    a.q, a.k, a.v, a.out = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), out.data_ptr()
    (a.q_row_stride, a.q_batch_stride), (a.k_row_stride, a.k_batch_stride), (a.v_row_stride, a.v_batch_stride) = c["st"]
    a.out_row_stride, a.out_batch_stride = ors, obs
    a.B, a.H, a.N, a.d_kv = c["B"], c["H"], c["N"], 64
    a.bias, a.key_mask = bias.data_ptr(), mask.data_ptr()
    return a


def _ta_check(L, c, group, case):
    B, N, hd = c["B"], c["N"], c["H"] * 64
    ors = hd + 4
    obs = N * ors + 4
    bufs = [f.to(DEV) for f in c["flats"]]
    bias, mask = c["bias"].to(DEV), c["mask"].to(DEV)
    outs = []
    for _ in range(2):
        out = _sent((B * obs + 8,))
        a = _ta_args(L, c, bufs, out, bias, mask, ors, obs)
        L.check(L.lib().v2a_t5_attention(ctypes.byref(a), L.stream_ptr()))
        outs.append(out.cpu())
    assert _same_bits(outs[0], outs[1]), "not bit-equal on a second run"
    o = outs[0]
    per = o[:B * obs].view(B, obs)
    rows = per[:, :N * ors].view(B, N, ors)
    assert _all_sent(o[B * obs:]) and _all_sent(per[:, N * ors:]) and _all_sent(rows[..., hd:])
    got = rows[..., :hd]
    assert float(c["ref"][TA_NONE].abs().max()) == 0.0 and float(c["tol"][TA_NONE].abs().max()) == 0.0     # no valid key: exact zeros
    for b, name in ((TA_ALL, "all valid"), (TA_LAST, "last key only"), (TA_FIRST, "key 0 only"), (TA_NONE, "no key")):
        _report("t5_attention", group + ", " + name, case, got[b], c["ref"][b], c["tol"][b])


@pytest.mark.parametrize("N", TA_NS)
def test_t5_attention_masks_and_strides(L, N):
    """N around the 64-key / 64-query block and over three blocks; q, k and v in three buffers with three row and three batch strides, out
    padded; batch rows with every key, only the last key (masked leading blocks: the running max starts from -inf at the last block), only key 0
    (masked trailing blocks) and no key at all (exact zeros); two runs give the same bits."""
    _ta_check(L, ta_case(N), "masks", "N=%d" % N)


def test_t5_attention_large_logits(L):
    """Unscaled q . k around 100 and bias entries of +-50 over three key blocks: the running max moves by tens between blocks."""
    _ta_check(L, ta_case(129, large=True), "large logits", "N=129")


def test_t5_attention_refusals(L):
    """d_kv = 32, N = 513, a row stride that is no multiple of 4: V2A_ERR_ARG, nothing written."""
    c = ta_case(65)
    bufs = [f.to(DEV) for f in c["flats"]]
    bias, mask = torch.zeros(c["H"], 2 * 513 - 1, device=DEV), torch.ones(c["B"], 513, dtype=torch.int32, device=DEV)
    hd = c["H"] * 64
    out = _sent((c["B"] * 65 * (hd + 4) + 64,))
    for name, ch in [("d_kv=32", dict(d_kv=32)), ("N=513", dict(N=513)), ("q_row_stride", dict(q_row_stride=hd + 2))]:
        a = _ta_args(L, c, bufs, out, bias, mask, hd + 4, 65 * (hd + 4) + 4)
        for k, v in ch.items():
            setattr(a, k, v)
        rc = L.lib().v2a_t5_attention(ctypes.byref(a), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (name, rc)
        assert _all_sent(out), name


# ------------------------------------------------------------------------------------------------------------- v2a_gemm_skinny_f32
def _sk_args(L, a, lda, K, w, ldw, bias, out, ldo, resid, ldr, M, N, epi):
    g = L.GemmArgs()
    g.a[0], g.lda[0], g.ka[0], g.nseg = a.data_ptr(), lda, K, 1
    g.a_dtype = g.compute_dtype = g.out_dtype = L.F32
    g.w, g.ldw, g.bias = w.data_ptr(), ldw, 0 if bias is None else bias.data_ptr()
    g.M, g.N, g.epilogue = M, N, {"store": L.EPI_STORE, "resid": L.EPI_RESID, "resid_inplace": L.EPI_RESID, "geglu_tanh": L.EPI_GEGLU_TANH}[epi]
    g.out, g.ldo = out.data_ptr(), ldo
    g.resid, g.ldr = 0 if resid is None else resid.data_ptr(), ldr
    return g


def _sk_launch(L, c, M, epi, bias):
    """lda = K + 4, ldw = K + 8, ldo = columns + 4, ldr = N + 8 (in place: resid is out, ldr = ldo -- with two strides on one buffer a row's
    residual would be another row's output).  Returns the (M, columns) result."""
    K, N = c["K"], c["N"]
    nw = 2 * N if epi == "geglu_tanh" else N             # W rows: the N output columns, or 2 N packed value / gate rows
    ldo = N + 4
    out = _sent((M + 1, ldo))
    a, w = c["a"][:M].to(DEV), c["w"][:nw].to(DEV)
    bv = c["bias"][:nw].to(DEV) if bias else None
    resid, ldr = None, 0
    if epi == "resid":
        resid, ldr = c["resid"][:M].to(DEV), N + 8
    elif epi == "resid_inplace":
        out[:M, :N] = c["resid"][:M, :N].to(DEV)
        resid, ldr = out, ldo
    g = _sk_args(L, a, K + 4, K, w, K + 8, bv, out, ldo, resid, ldr, M, nw, epi)
    L.check(L.lib().v2a_gemm_skinny_f32(ctypes.byref(g), L.stream_ptr()))
    o = out.cpu()
    assert _all_sent(o[M:]) and _all_sent(o[:M, N:])
    return o[:M, :N].contiguous()


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("epi", SK_EPIS)
@pytest.mark.parametrize("M,K,N", SK_SHAPES)
def test_gemm_skinny_rows_steps_and_strides(L, M, K, N, epi, bias):
    """M on both sides of the 16 / 32 switches between the 1-, 2- and 4-tile kernels and on both sides of a 64-row workgroup, at K = 96 (3 steps:
    five waves idle); K of 1, 2, 7 and 9 steps (idle waves, uneven shares) at M = 17; one and three column workgroups; every epilogue with and
    without bias (GEGLU_TANH: bias[n] on the value and bias[n + 16] on the gate of packed rows), every stride larger than the logical width,
    RESID with a residual of its own stride and in place."""
    c = sk_case(K, N)
    got = _sk_launch(L, c, M, epi, bias)
    ref, tol = sk_ref(K, N, M, epi, bias)
    _report("gemm_skinny", epi, "M=%d K=%d N=%d %s" % (M, K, N, "bias" if bias else ""), got, ref, tol)


def test_gemm_skinny_8192_rows(L):
    """The admitted M: 128 row workgroups of the 4-tile kernel at one K step."""
    M, K, N = 8192, 32, 16
    c = sk_case(K, N, M)
    got = _sk_launch(L, c, M, "store", True)
    ref, tol = sk_ref(K, N, M, "store", True, Mfull=M)
    _report("gemm_skinny", "store", "M=8192 K=32 N=16 bias", got, ref, tol)


@pytest.mark.parametrize("epi", ["store", "geglu_tanh"])
@pytest.mark.parametrize("K", SK_KS)
def test_gemm_skinny_row_0_has_the_same_bits_for_every_m(L, K, epi):
    c = sk_case(K, 48)
    rows = [_sk_launch(L, c, M, epi, True)[0] for M in SK_MS]
    assert all(_same_bits(rows[0], r) for r in rows[1:]), (K, epi)
    print("encoder %-15s %-18s %-40s bit for bit" % ("gemm_skinny", "row 0, every M", "K=%d %s" % (K, epi)))


def test_gemm_skinny_refusals(L):
    """K = 48, M = 8193, STORE with N = 24, GEGLU_TANH with N = 48, RESID without resid, a tile hint: V2A_ERR_ARG, nothing written."""
    a, w, out = torch.zeros(16, 64, device=DEV), torch.zeros(64, 64, device=DEV), _sent((16, 64))
    for name, K, M, N, epi, resid, hint in [("K=48", 48, 16, 16, "store", None, 0), ("M=8193", 32, 8193, 16, "store", None, 0),
                                            ("STORE N=24", 32, 16, 24, "store", None, 0), ("GEGLU_TANH N=48", 32, 16, 48, "geglu_tanh", None, 0),
                                            ("RESID without resid", 32, 16, 16, "resid", None, 0), ("tile hint", 32, 16, 16, "store", None, 1)]:
        g = _sk_args(L, a, 64, K, w, 64, None, out, 64, resid, 64, M, N, epi)
        g.tile_hint = hint
        rc = L.lib().v2a_gemm_skinny_f32(ctypes.byref(g), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (name, rc)
        assert _all_sent(out), name


# ------------------------------------------------------------------------------------------------------------- DINOv2 through v2a_clip_attention
def test_dinov2_small_through_clip_attention(monkeypatch):
    """The DINOv2 encoder in fp32 mode with f32_attention = "v2a_clip_attention" (d_head = 64 on the VALU kernel) against the transformers
    float64 fixture, at the bar test_dinov2_gpu.py holds the fp32 mode to."""
    import numpy as np
    import test_dinov2_gpu as D2
    from v2a_amd.vit import ViTImageEncoder
    calls = []
    base = ViTImageEncoder.attention
    monkeypatch.setattr(ViTImageEncoder, "attention", lambda self, qkv, out, F: (calls.append(F), base(self, qkv, out, F))[1])
    z, meta = D2._fx("small")
    worst = {}
    for cname, case in meta["cases"].items():
        enc = D2._encoder(case, "fp32", D2._weights(case), chunk=2)
        enc.f32_attention = "v2a_clip_attention"
        assert enc.dh == 64 and not enc.split
        for clip in case["clips"]:
            key = f"{cname}_{clip[0]}"
            fr = torch.from_numpy(D2._frames(clip, key, z)).to(D2.DEV)
            n0 = len(calls)
            got = enc.encode_chunk(fr).cpu().numpy().astype(np.float64)
            assert len(calls) - n0 == len(enc.layers), "the encoder did not go through v2a_clip_attention"
            worst[key] = D2._rel(got, z[key + "_embeds"])
            print("encoder %-15s %-18s %-40s pooler_output %.2e (bar %.0e)" % ("dinov2", "clip_attention", key, worst[key], D2.BARS["fp32"]))
        del enc
    assert worst and all(e <= D2.BARS["fp32"] for e in worst.values()), worst
