"""CPU: the float64 reference helpers, the tolerance formulas and the inputs of tests/test_encoder_kernels_gpu.py against independent forms --
torch.nn.functional.layer_norm, softmax with einsum and masked_fill, Python loops over keys and over K, the T5 reference of tests/test_t5_gpu.py --
so that a wrong helper cannot agree with a kernel that is wrong in the same way, and no tolerance is loose enough to hide a wrong lane: every
bound stays below 1e-3 of the RMS of its reference on every case of the GPU file's parameter lists, and every check misses its bound when the
reference is mutated the way a wrong lane, a dropped key or K step, a shifted bias index or a one-pass variance would."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_encoder_kernels_gpu as E
import test_t5_gpu as T5

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


def _misses(mut, ref, tol):
    """A mutated reference is outside the bound on at least one element."""
    return bool(((mut.double() - ref.double()).abs() > tol).any())


# ------------------------------------------------------------------------------------------------------------- layernorm, embed_init, rmsnorm
def test_layernorm_ref_against_torch_and_the_special_rows():
    for d in E.LN_WIDTHS:
        c = E.ln_case(d)
        x = c["x"][:, :d]
        want = F.layer_norm(x.double(), (d,), c["g"].double(), c["b"].double(), E.LN_EPS)
        torch.testing.assert_close(c["ref"], want, rtol=1e-12, atol=1e-12)
        assert c["ldx"] == d + 4 and float(c["x"][:, d:].abs().min()) > 0                      # the pad columns are not zero
        assert torch.equal(c["ref"][E.LN_CONST], c["b"].double()) and torch.equal(c["ref"][E.LN_ZERO], c["b"].double())
        assert bool((x[E.LN_CONST] == 0.5).all()) and bool((x[E.LN_ZERO] == 0).all())
        m = x[E.LN_MEAN100].double()
        assert abs(float(m.mean()) - 100) < 2 and (d == 4 or 0.8 < float(m.std()) < 1.2)
        # three x60 channels: the row's largest magnitudes
        assert float(x[E.LN_OUTLIER].abs().max()) > (5 if d > 4 else 0) * float(x[E.LN_PLAIN].abs().median())


def test_layernorm_bounds_and_the_one_pass_variance():
    """The bound holds the cap on every width, and a variance formed as E[x^2] - mean^2 in fp32 misses it on the mean-100 row of every width."""
    for d in E.LN_WIDTHS:
        c = E.ln_case(d)
        _bound_ok("layernorm d=%d" % d, c["tol"], c["ref"])
        _bound_ok("layernorm hi + lo d=%d" % d, E.tol_split_sum(c["tol"], c["ref"]), c["ref"])
        assert torch.equal(E.tol_split_hi(c["tol"], c["ref"]) - c["tol"], E._half_ulp_bf16(c["ref"])) or bool(
            ((E.tol_split_hi(c["tol"], c["ref"]) - c["tol"] - E._half_ulp_bf16(c["ref"])).abs() <= 1e-12 * c["ref"].abs() + 1e-300).all())
        x = c["x"][E.LN_MEAN100, :d]                                                           # fp32 throughout
        mean = x.cumsum(0)[-1] / d                                                              # sums taken in order, as one lane would
        var = (x * x).cumsum(0)[-1] / d - mean * mean
        assert var.dtype == torch.float32
        mut = ((x - mean) * (1.0 / torch.sqrt(var + E.LN_EPS))) * c["g"] + c["b"]
        two = ((x - mean) * (1.0 / torch.sqrt(((x - mean) ** 2).sum() / d + E.LN_EPS))) * c["g"] + c["b"]
        assert _misses(mut, c["ref"][E.LN_MEAN100], c["tol"][E.LN_MEAN100]), d
        assert not _misses(two, c["ref"][E.LN_MEAN100], c["tol"][E.LN_MEAN100]), d                # the centred form in fp32 is inside it


def test_embed_ref_against_a_loop():
    for T, d in E.EI_CASES:
        g = _g(T + d)
        cls, pos = torch.randn(d, generator=g), torch.randn(T, d, generator=g)
        rows = 2 * T + 1
        ref = E._embed_ref(rows, T, cls, pos)
        assert ref.dtype == torch.float32 and rows % T == (1 if T > 1 else 0)
        for r in range(rows):
            want = pos[r % T] + cls if r % T == 0 else pos[r % T]
            assert torch.equal(ref[r], want)


def test_t5_rmsnorm_ref_and_bounds():
    assert E.TR_IDS[0] == 0 and E.TR_VOCAB - 1 in E.TR_IDS and E.TR_ZERO in E.TR_IDS and 0 <= min(E.TR_IDS) and max(E.TR_IDS) < E.TR_VOCAB
    for d in E.TR_WIDTHS:
        for gather in (False, True):
            c = E.tr_case(d, gather)
            x = c["rows"].double()
            want = c["w"].double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c["eps"]))
            torch.testing.assert_close(c["ref"], want, rtol=1e-13, atol=0)
            if gather:
                for r, i in enumerate(E.TR_IDS):
                    assert torch.equal(c["rows"][r], c["x"][i, :d])
            zero = E.TR_IDS.index(E.TR_ZERO) if gather else E.TR_ZERO
            assert float(c["ref"][zero].abs().max()) == 0.0 and float(c["x"][E.TR_ZERO, d:].abs().min()) > 0
            assert len({c["ldx"], c["ldr"], c["ldy"]}) == 3 and min(c["ldx"], c["ldr"], c["ldy"]) > d
            _bound_ok("t5_rmsnorm d=%d" % d, c["tol"], c["ref"])
    c = E.tr_case(1028, False, eps=0.0)
    assert c["eps"] == 0.0 and float(c["rows"].abs().sum(-1).min()) > 0
    torch.testing.assert_close(c["ref"], c["w"].double() * F.normalize(c["rows"].double(), dim=-1) * math.sqrt(1028), rtol=1e-13, atol=0)
    _bound_ok("t5_rmsnorm eps=0", c["tol"], c["ref"])


# ------------------------------------------------------------------------------------------------------------- attention
def _loop_attention(q, k, v, scale, bias, mask, b, h, i):
    """One query by a Python loop over the keys: (o, S1, S2, A, R) as lists / floats."""
    N, D = q.shape[1], q.shape[3]
    z, a, js = [], [], []
    for j in range(N):
        if mask is not None and not int(mask[b, j]):
            continue
        s = scale * sum(float(q[b, i, h, t]) * float(k[b, j, h, t]) for t in range(D))
        m = scale * sum(abs(float(q[b, i, h, t])) * abs(float(k[b, j, h, t])) for t in range(D))
        if bias is not None:
            s, m = s + float(bias[h, j - i + N - 1]), m + abs(float(bias[h, j - i + N - 1]))
        z.append(s), a.append(m), js.append(j)
    if not js:
        return [0.0] * D, [0.0] * D, [0.0] * D, 0.0, 0.0
    w = [math.exp(s - max(z)) for s in z]
    p = [x / sum(w) for x in w]
    o = [sum(pj * float(v[b, j, h, t]) for pj, j in zip(p, js)) for t in range(D)]
    S1 = [sum(pj * abs(float(v[b, j, h, t]) - o[t]) for pj, j in zip(p, js)) for t in range(D)]
    S2 = [sum(pj * abs(float(v[b, j, h, t])) for pj, j in zip(p, js)) for t in range(D)]
    return o, S1, S2, max(a), max(z) - min(z)


def test_attn_ref_against_softmax_einsum_and_a_loop_over_keys():
    for D, N, kind in [(4, 33, "plain"), (28, 33, "plain"), (104, 65, "plain"), (64, 129, "plain"), (64, 129, "first"), (64, 129, "last")]:
        c = E.ca_case(D, N, kind)
        q, k, v = (c[n].double().transpose(1, 2) for n in "qkv")                                # (B, H, N, D)
        p = torch.softmax(q @ k.transpose(-1, -2) * c["scale"], -1)
        want = (p @ v).transpose(1, 2).reshape(c["B"], N, c["H"] * D)
        torch.testing.assert_close(c["ref"], want, rtol=1e-11, atol=1e-13)
        # the views are the kernel's addressing: base + b * batch_stride + token * row_stride + h * d_head
        hd = c["H"] * D
        assert c["rs"] == 3 * hd + 8 and c["bs"] == N * c["rs"] + 4
        for which, name in enumerate("qkv"):
            at = 1 * c["bs"] + (N - 1) * c["rs"] + which * hd + 2 * D
            assert torch.equal(c["flat"][at:at + D], c[name][1, N - 1, 2])
    c = E.ca_case(28, 33)
    for b, h, i in [(0, 0, 0), (1, 2, 32), (1, 1, 17)]:
        o, S1, S2, A, R = _loop_attention(c["q"], c["k"], c["v"], c["scale"], None, None, b, h, i)
        sl = slice(h * 28, h * 28 + 28)
        for name, want in (("o", o), ("S1", S1), ("S2", S2)):
            np.testing.assert_allclose(c["r"][name][b, i, sl].numpy(), want, rtol=1e-11, atol=1e-14)
        assert abs(float(c["r"]["A"][b, i, h]) - A) < 1e-12 * A and abs(float(c["r"]["R"][b, i, h]) - R) < 1e-11


def test_large_logit_cases_are_large_and_dominated():
    for kind in ("first", "last"):
        c = E.ca_case(E.CA_LARGE["D"], E.CA_LARGE["N"], kind)
        z = torch.einsum("bihd,bjhd->bhij", c["q"].double(), c["k"].double())
        assert c["scale"] == 1.0 and float(z.abs().min()) > 150 and float(z.abs().max()) < 300
        j = E.CA_LARGE[kind]
        assert (j // 32 == 0) if kind == "first" else (j // 32 == (c["N"] - 1) // 32 and j // 32 >= 2)
        assert bool((z.argmax(-1) == j).all())                                                  # the dominant key of every query
        others = z.clone()
        others[..., j] = -math.inf
        assert float((z[..., j] - others.max(-1).values).min()) > 3
    c = E.ta_case(129, large=True)
    z = torch.einsum("bihd,bjhd->bhij", c["q"].double(), c["k"].double())
    assert float(z.abs().min()) > 80 and float(z.abs().max()) > 100 and int((c["bias"] == 50).sum()) > 50 and int((c["bias"] == -50).sum()) > 50


def test_t5_attn_ref_against_the_t5_reference_and_masked_fill():
    for N, large in [(1, False), (63, False), (65, False), (129, False), (129, True)]:
        c = E.ta_case(N, large)
        q, k, v, bias, mask = c["q"].double(), c["k"].double(), c["v"].double(), c["bias"].double(), c["mask"]
        hd = c["H"] * 64
        live = [E.TA_ALL, E.TA_LAST, E.TA_FIRST]
        want = T5._attn_ref(q[live], k[live], v[live], bias, mask[live], N).reshape(3, N, hd)
        torch.testing.assert_close(c["ref"][live], want, rtol=1e-10, atol=1e-13)
        # masked_fill on the scores, by hand
        s = torch.einsum("bihd,bjhd->bhij", q, k) + bias[:, torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1][None]
        s = s.masked_fill(~mask.bool()[:, None, None, :], -math.inf)
        p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)                                     # the row without a key: 0, as the header says
        torch.testing.assert_close(c["ref"], torch.einsum("bhij,bjhd->bihd", p, v).reshape(c["B"], N, hd), rtol=1e-10, atol=1e-13)
        assert float(c["ref"][E.TA_NONE].abs().max()) == 0.0 and float(c["tol"][E.TA_NONE].abs().max()) == 0.0
        # a single valid key: the output is that key's value row, whatever the scores
        assert torch.equal(c["ref"][E.TA_LAST], v[E.TA_LAST, N - 1].reshape(1, hd).expand(N, hd))
        assert torch.equal(c["ref"][E.TA_FIRST], v[E.TA_FIRST, 0].reshape(1, hd).expand(N, hd))
        assert c["mask"].sum(-1).tolist() == [N, 1, 1, 0]
        assert len({rs for rs, _ in c["st"]}) == 3 and len({bs - N * rs for rs, bs in c["st"]}) == 3
    c = E.ta_case(63)
    for b, h, i in [(E.TA_ALL, 0, 0), (E.TA_ALL, 1, 62), (E.TA_LAST, 1, 5), (E.TA_NONE, 0, 3)]:
        o, S1, S2, A, R = _loop_attention(c["q"], c["k"], c["v"], 1.0, c["bias"], c["mask"], b, h, i)
        sl = slice(h * 64, h * 64 + 64)
        for name, want in (("o", o), ("S1", S1), ("S2", S2)):
            np.testing.assert_allclose(c["r"][name][b, i, sl].numpy(), want, rtol=1e-11, atol=1e-14)
        assert abs(float(c["r"]["A"][b, i, h]) - A) <= 1e-12 * A and abs(float(c["r"]["R"][b, i, h]) - R) < 1e-11


def _zero_lane(q, lane, width):
    q = q.clone()
    q[..., lane * width:(lane + 1) * width] = 0
    return q


@pytest.mark.parametrize("D,N", E.CA_SHAPES)
def test_clip_attention_bounds_and_mutations(D, N):
    """The cap, and the bound against a dropped key (the last one: the key a wrong block tail loses) and against lane 0's 28 dims of q read as
    zero."""
    c = E.ca_case(D, N)
    _bound_ok("clip_attention d_head=%d N=%d" % (D, N), c["tol"], c["ref"])
    _bound_ok("clip_attention hi + lo", E.tol_split_sum(c["tol"], c["ref"]), c["ref"])
    if N > 1:
        keep = torch.ones(c["B"], N, dtype=torch.int32)
        keep[:, N - 1] = 0
        assert _misses(E._attn_ref(c["q"], c["k"], c["v"], c["scale"], None, keep)["o"], c["ref"], c["tol"])
        assert _misses(E._attn_ref(_zero_lane(c["q"], 0, 28), c["k"], c["v"], c["scale"])["o"], c["ref"], c["tol"])
        if D > 84:
            assert _misses(E._attn_ref(_zero_lane(c["q"], 3, 28), c["k"], c["v"], c["scale"])["o"], c["ref"], c["tol"])
    E._CASES.pop(("ca", D, N, "plain"))


@pytest.mark.parametrize("kind", ["first", "last"])
def test_clip_attention_large_logit_bounds_and_mutations(kind):
    c = E.ca_case(E.CA_LARGE["D"], E.CA_LARGE["N"], kind)
    _bound_ok("clip_attention large " + kind, c["tol"], c["ref"])
    keep = torch.ones(c["B"], c["N"], dtype=torch.int32)
    keep[:, E.CA_LARGE[kind]] = 0                                                              # the dominant key dropped
    assert _misses(E._attn_ref(c["q"], c["k"], c["v"], c["scale"], None, keep)["o"], c["ref"], c["tol"])
    assert _misses(E._attn_ref(_zero_lane(c["q"], 1, 28), c["k"], c["v"], c["scale"])["o"], c["ref"], c["tol"])


@pytest.mark.parametrize("N,large", [(N, False) for N in E.TA_NS] + [(129, True)])
def test_t5_attention_bounds_and_mutations(N, large):
    """The cap, and the bound against a dropped key, a 16-dim lane of q read as zero and the bias read one entry off."""
    c = E.ta_case(N, large)
    _bound_ok("t5_attention N=%d" % N, c["tol"], c["ref"])
    a = E.TA_ALL
    mut = E._attn_ref(c["q"], c["k"], c["v"], 1.0, torch.roll(c["bias"], 1, -1), c["mask"])["o"]
    assert N == 1 or _misses(mut[a], c["ref"][a], c["tol"][a])
    assert _misses(E._attn_ref(_zero_lane(c["q"], 2, 16), c["k"], c["v"], 1.0, c["bias"], c["mask"])["o"][a], c["ref"][a], c["tol"][a]) or N == 1
    if N > 1:
        keep = c["mask"].clone()
        keep[a, N - 1] = 0
        assert _misses(E._attn_ref(c["q"], c["k"], c["v"], 1.0, c["bias"], keep)["o"][a], c["ref"][a], c["tol"][a])


# ------------------------------------------------------------------------------------------------------------- skinny GEMM
def test_skinny_ref_against_a_loop_with_gelu_new():
    from v2a_amd.t5 import pack_geglu
    K, N, M = 32, 16, 3
    c = E.sk_case(K, N)
    a, w, bias, resid = c["a"][:M, :K], c["w"][:, :K], c["bias"], c["resid"][:M, :N]
    dot = lambda m, n: sum(float(a[m, k]) * float(w[n, k]) for k in range(K))                       # noqa: E731
    adot = lambda m, n: sum(abs(float(a[m, k])) * abs(float(w[n, k])) for k in range(K))            # noqa: E731
    gelu = lambda x: 0.5 * x * (1 + math.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))    # noqa: E731
    for use_bias in (False, True):
        for epi in ("store", "resid", "resid_inplace"):
            ref, tol = E.sk_ref(K, N, M, epi, use_bias)
            for m in range(M):
                for n in range(N):
                    v, s = dot(m, n), adot(m, n)
                    if use_bias:
                        v, s = v + float(bias[n]), s + abs(float(bias[n]))
                    if epi != "store":
                        v, s = v + float(resid[m, n]), s + abs(float(resid[m, n]))
                    assert abs(float(ref[m, n]) - v) < 1e-13 and abs(float(tol[m, n]) - (K + 3) * E.U * s) < 1e-18
        ref, tol = E.sk_ref(K, N, M, "geglu_tanh", use_bias)
        assert ref.shape == (M, N)
        for m in range(M):
            for j in range(N):                                                                  # output j: value row 32 (j / 16) + j % 16, gate 16 further
                n = 32 * (j // 16) + j % 16
                v, g = dot(m, n), dot(m, n + 16)
                if use_bias:
                    v, g = v + float(bias[n]), g + float(bias[n + 16])
                assert abs(float(ref[m, j]) - v * gelu(g)) < 1e-13
    # the packing is the engine's: value = wi_1, gate = wi_0 per 16 outputs
    wi0, wi1 = torch.randn(32, 8, generator=_g(1)), torch.randn(32, 8, generator=_g(2))
    packed = pack_geglu(wi0, wi1)
    x = torch.randn(2, 8, generator=_g(3))
    ref, _ = E._skinny_ref(x, packed, None, None, "geglu_tanh")
    torch.testing.assert_close(ref, (x.double() @ wi1.double().t()) * E._gelu_new(x.double() @ wi0.double().t()), rtol=1e-13, atol=1e-15)
    xs = torch.linspace(-6, 6, 4001, dtype=torch.float64, requires_grad=True)
    (slope,) = torch.autograd.grad(E._gelu_new(xs).sum(), xs)
    assert float(slope.abs().max()) <= E.GELU_SLOPE
    torch.testing.assert_close(E._gelu_new(xs.detach()), F.gelu(xs.detach(), approximate="tanh"), rtol=1e-13, atol=1e-15)


def test_skinny_shapes_reach_every_switch():
    ms, ks, ns = ({s[i] for s in E.SK_SHAPES} for i in range(3))
    assert ms == set(E.SK_MS) == {1, 16, 17, 32, 33, 64, 65} and ks == set(E.SK_KS) == {32, 64, 96, 224, 288} and ns == set(E.SK_NS) == {16, 48}
    assert sorted(k // 32 for k in E.SK_KS) == [1, 2, 3, 7, 9]
    shares = {k: [(w + 1) * (k // 32) // 8 - w * (k // 32) // 8 for w in range(8)] for k in E.SK_KS}
    assert all(sum(s) == k // 32 for k, s in shares.items()) and shares[32].count(0) == 7 and max(shares[288]) == 2 and min(shares[288]) == 1
    assert set(E.SK_EPIS) == {"store", "resid", "resid_inplace", "geglu_tanh"}


@pytest.mark.parametrize("M,K,N", E.SK_SHAPES + [(8192, 32, 16)])
def test_skinny_bounds_and_mutations(M, K, N):
    """The cap on every epilogue, and the bound against one 32-wide K step dropped and against bias[n] and bias[n + 16] swapped."""
    full = 8192 if M == 8192 else E.SK_MMAX
    c = E.sk_case(K, N, full)
    for epi in (["store"] if M == 8192 else E.SK_EPIS):
        for bias in (False, True):
            ref, tol = E.sk_ref(K, N, M, epi, bias, Mfull=full)
            _bound_ok("skinny %s M=%d K=%d N=%d" % (epi, M, K, N), tol, ref)
            nw = 2 * N if epi == "geglu_tanh" else N
            a = c["a"][:M, :K].clone()
            a[:, K - 32:] = 0                                                                   # the last K step dropped
            bv = c["bias"][:nw] if bias else None
            mut, _ = E._skinny_ref(a, c["w"][:nw, :K], bv, c["resid"][:M, :N], epi)
            assert _misses(mut, ref, tol), (epi, bias, "K step")
            if bias and epi == "geglu_tanh":
                sw = bv.view(-1, 2, 16).flip(1).reshape(-1)                                     # bias[n] <-> bias[n + 16]
                mut, _ = E._skinny_ref(c["a"][:M, :K], c["w"][:nw, :K], sw, c["resid"][:M, :N], epi)
                assert _misses(mut, ref, tol), "bias swap"
    if M == 8192:
        E._CASES.pop(("sk", K, N, full))


# ------------------------------------------------------------------------------------------------------------- the existing bars
def test_bounds_against_the_existing_bars():
    """The bars of test_clip_gpu.py and test_t5_gpu.py on the shapes those tests run.  The layernorm bound is inside its bar on that test's own
    input.  The other three bars are measured figures below what a worst-case bound can promise: a sum of n terms may err by n u of the sum of
    its magnitudes, which is at least the result -- asserted here as it stands, with the figures printed, so that the derived bounds are not
    taken for tighter than they are (see the GPU file's docstring).  For T5 attention the comparison is made on this file's inputs at the lengths
    test_t5_attention runs (B and H do not enter the bound)."""
    g = _g(1)
    rows, d = 300, 1664                                                                         # test_layernorm_fp32_and_split_against_float64
    x = torch.randn(rows, d, generator=g) * 3 + 0.5
    x[:, [5, 700, 1200]] *= 60
    gam, bet = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ref = F.layer_norm(x.double(), (d,), gam.double(), bet.double(), 1e-5)
    tol = E.tol_layernorm(x, gam, ref, 1e-5)
    print("layernorm d=1664: bound %.2e of max|y| (bar 2e-6)" % (float(tol.max()) / float(ref.abs().max())))
    assert float(tol.max()) <= 2e-6 * float(ref.abs().max())
    # v2a_clip_attention: N FMAs on sum p v; sum p |v| >= |o|
    for N in (257, 577):
        assert N * E.U > 2e-6
    # v2a_gemm_skinny_f32: (K + 3) u (sum |a| |w|) >= (K + 3) u |ref|
    for K in (128, 1024, 2816):
        assert (K + 3) * E.U > 4e-6 * max(1.0, math.sqrt(K / 128))
    # v2a_t5_attention on this file's inputs at the lengths of test_t5_attention
    for N in (1, 7, 64, 200, 512):
        c = E.ta_case(N)
        bar = 2e-5 * max(1.0, float(c["ref"].abs().max()))
        print("t5_attention N=%d: bound %.2e, bar %.2e" % (N, float(c["tol"].max()), bar))
        assert (float(c["tol"].max()) <= bar) == (N == 1)                                       # (64 + 6) u on scores of magnitude ~15 alone is 6e-5
        E._CASES.pop(("ta", N, False))
