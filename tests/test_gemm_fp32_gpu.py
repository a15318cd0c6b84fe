"""GPU: the register-staged GEMM (csrc/gemm.hip, gemm_kernel<T, A_F32, EPI, OutT, BM, BN> with the scalar gemm_epilogue of csrc/gemm_common.h)
against float64, on both of its tiles and on the three paths that reach it:

  path                                   tile                                            K tile
  exact fp32 (compute = V2A_F32)         64x64 if ceil(M/128) ceil(N/128) < 224 and      16 (v_mfma_f32_16x16x4_f32, an fma chain in k order)
                                         M > 64, else 128x128
  bf16 compute on fp32 A (A_F32)         128x128                                         64 (A rounded to bf16 on load)
  bf16 x bf16 with the SIGMOID epilogue  128x128                                         64

Shapes (M, N) of the exact-fp32 path, the smallest that reach each rule (tile_of() below restates v2a_gemm's rule; tests/test_gemm_fp32_refs.py
holds it against the source):
  (64, 144)     128x128 through M <= 64: 2 workgroups, a 16-column last tile
  (65, 144)     64x64: a second row band of one row, 6 workgroups
  (273, 272)    64x64: 25 workgroups (the XCD remap has a remainder of 1), full and partial wave tiles
  (1, 20)       128x128: N is no multiple of 16
  (130, 1/3)    64x64: output rows that are not 16-byte aligned
  (1800, 1920)  128x128 through 15 x 15 = 225 >= 224 tiles (K = 32): a last row band of 8 rows, remap remainder 1
K = 16 .. 80 gives 1 .. 5 K tiles on either tile (no prefetch, odd and even ring positions), K = 1024 the longest chain the project's bar covers,
segment lists (16, 48, 32) and (32, 16) put a segment switch on single K tiles, lda = C with K = 3C reads overlapping rows (Encodec's convolutions).
The bf16 paths run (65, 144), (273, 272) and (3, 144) at K = 64 .. 192 = 1 .. 3 K tiles and segments (64, 128).

Operands come from seeded CPU generators, a ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias ~ 0.1 N(0, 1), resid ~ N(0, 1); the values of an (M, N, K) are
made once and shared (never modified), and so is every device layout of them.  References are float64 products of the operands (of the
bf16-rounded operands on the bf16 paths) through plain torch ops.  Every output is prefilled with NaN and every shadow with a sentinel, so an element
nobody wrote fails; the padding of strided operands is NaN, so a read outside the k columns of a row fails; the columns behind N (N / 2) of a
wide output row must still hold their NaN afterwards.  Bars, all taken from the project's tests of the same operand scaling:
  fp32 compute STORE / RESID / GATE_RESID   atol 2e-5, rtol 1e-5 (test_gemm_store, test_gemm_gate_resid_and_sigmoid), and on K <= 128 the a-priori
                                            bound of an fma chain, |err| <= (K + 4) 2^-24 (|A| |W|^T + |bias| [+ |resid|]) (gated: the product
                                            scaled by |gate|): K roundings of the chain, one each for bias, gate and residual, one spare
  SIGMOID                                   atol 1e-5, rtol 1e-5 (test_gemm_gate_resid_and_sigmoid)
  fp32 compute GELU / GEGLU / SWIGLU        max |err| / max |ref| <= 2e-6 (test_clip_gpu, test_dinov2_gpu)
  bf16 paths, fp32 out                      atol 1e-4, rtol 1e-4 against float64 of the bf16-rounded operands (test_gemm_store)
  bf16 outputs                              |err| <= 2^-8 |ref| + 1e-3 (test_gemm_ring_hints_gpu)
  shadows                                   torch.equal to bfloat16() of the stored fp32 output
Bit equality (torch.equal, fp32 compute): the K order of an output element depends neither on the tile, nor on M, nor on the strides.

Every case prints its largest error ("gemm-fp32 <what> ... err=<e>") before it asserts."""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SHADOW_SENTINEL = -3.0
U = 2.0 ** -24                       # unit roundoff of fp32
F32_BAR = dict(atol=2e-5, rtol=1e-5)
SIGMOID_BAR = dict(atol=1e-5, rtol=1e-5)
BF16_COMPUTE_BAR = dict(atol=1e-4, rtol=1e-4)
ACT_REL_BAR = 2e-6
STEP, NSTEPS = 3, 5
BOUND_MAX_K = 128                    # the a-priori bound is asserted up to here (beyond, the project's bar is the tighter one)

# (M, N) -> (tile, workgroups) as v2a_gemm picks them for compute = V2A_F32
TILES = {(64, 144): (128, 2), (65, 144): (64, 6), (273, 272): (64, 25), (1, 20): (128, 1), (130, 1): (64, 3), (130, 3): (64, 3),
         (1800, 1920): (128, 225), (200, 1920): (64, 120), (3, 144): (128, 2), (3, 272): (128, 3),
         (64, 96): (128, 1), (65, 96): (64, 4), (64, 160): (128, 2), (65, 160): (64, 6)}
BIG = (1800, 1920)
BIG_K = 32
BIG_ROWS = 200                       # rows 0 .. 199 of the big launch, alone: 2 x 15 = 30 tiles of 128x128 -> the 64x64 tile
# the epilogue cases: one 128x128 shape and two 64x64 ones at 3 K tiles, and the shape that reaches 128x128 through the tile count
EPI_CASES = [(64, 144, 48), (65, 144, 48), (273, 272, 48), BIG + (BIG_K,)]
GLU_CASES = [(64, 96, 48), (65, 96, 48), (64, 160, 48), (65, 160, 48)]            # N / 32 odd: the last tile holds one value | gate pair


def tile_of(M, N):
    """The tile of the exact-fp32 kernel: v2a_gemm's `t128 < 224 && M > 64` rule (csrc/gemm.hip)."""
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    return 64 if t128 < 224 and M > 64 else 128


def workgroups(M, N, tile=None):
    t = tile or tile_of(M, N)
    return ((M + t - 1) // t) * ((N + t - 1) // t)


def glu_unpack(z):
    """(M, N) pre-activations of W rows packed [16 value | 16 gate] -> value, gate, (M, N / 2) each."""
    M, N = z.shape
    z = z.reshape(M, N // 32, 2, 16)
    return z[:, :, 0].reshape(M, N // 2), z[:, :, 1].reshape(M, N // 2)


def gate_rows(table, step, M, rpb):
    """table [steps][batches][N] -> the gate row of every output row: the step's row of batch element m // rpb."""
    return table[step][torch.arange(M) // rpb]


def tie_inputs(M, K, seed):
    """fp32 values that lie exactly between two neighbouring bf16 values (a bf16 value plus half a bf16 ulp of magnitude), both signs and both
    parities of the lower neighbour's last mantissa bit: nearest-even, half-up (half away from zero) and truncation give three different matrices."""
    b = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).bfloat16().float()
    return (b.view(torch.int32) | 0x8000).view(torch.float32)


def round_bf16_bits(x, rule):
    """fp32 -> bf16 (returned as fp32) by integer arithmetic on the bits; rule: "even" (round to nearest even), "half_up" (ties away from zero),
    "trunc"."""
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if rule == "even":
        bits = bits + 0x7FFF + ((bits >> 16) & 1)
    elif rule == "half_up":
        bits = bits + 0x8000
    bits = bits & 0xFFFF0000
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)


def dot_bound(K, absacc, *terms, gate=None):
    """(K + 4) 2^-24 (|A| |W|^T + |bias| ...): what an fp32 fma chain of K products in any order, then one rounding each for the bias, the gate
    and the residual, can be away from the exact result.  gate scales the product and the bias; terms behind it are added unscaled."""
    s = absacc
    if gate is not None:
        s = (s + terms[0]) * gate.abs()
        terms = terms[1:]
    for t in terms:
        s = s + t
    return (K + 4) * U * s


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------------------------- operands, made once
_VALS, _LAYOUTS, _GATES = {}, {}, {}


def _values(M, N, K, a=None):
    """CPU operands of one (M, N, K) and their float64 products; `a` replaces the activations (overlapping rows, ties)."""
    key = (M, N, K, None if a is None else a[0])
    if key not in _VALS:
        g = torch.Generator().manual_seed(1000 * M + N + 7 * K)
        v = types.SimpleNamespace(M=M, N=N, K=K)
        v.a = torch.randn(M, K, generator=g) if a is None else a[1]
        v.w = torch.randn(N, K, generator=g) / math.sqrt(K)
        v.bias = 0.1 * torch.randn(N, generator=g)
        v.res = torch.randn(M, N, generator=g)
        v.refs = {}
        _VALS[key] = v
    return _VALS[key]


def _ref(v, prec):
    """float64: acc = A W^T, |A| |W|^T, acc + bias; prec "f32" on the operands as they are, "bf16" on their bf16 roundings."""
    if prec not in v.refs:
        a, w = (v.a.double(), v.w.double()) if prec == "f32" else (v.a.bfloat16().double(), v.w.bfloat16().double())
        acc = a @ w.t()
        v.refs[prec] = types.SimpleNamespace(acc=acc, absacc=a.abs() @ w.abs().t(), z=acc + v.bias.double(), b=v.bias.double().abs(),
                                             res=v.res.double())
    return v.refs[prec]


def _padded(t, pad, dtype=None):
    """t as the leading columns of a buffer whose rows are `pad` elements wider, the padding NaN; returns the view and the row stride."""
    t = t if dtype is None else t.to(dtype)
    if not pad:
        return t.contiguous().to(DEV), t.shape[1]
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]], t.shape[1] + pad


def _layout(v, ks=None, pad_a=0, pad_w=0, pad_r=0, adt=torch.float32, wdt=torch.float32):
    """Device layout of v's operands: A in K segments `ks` of rows pad_a wider than k, W rows pad_w wider than K, residual rows pad_r wider
    than N.  Made once per (values, layout)."""
    ks = tuple(ks or (v.K,))
    key = (id(v), ks, pad_a, pad_w, pad_r, adt, wdt)
    if key not in _LAYOUTS:
        d = types.SimpleNamespace(segs=[], v=v)
        k0 = 0
        for k in ks:
            t, ld = _padded(v.a[:, k0:k0 + k], pad_a, adt)
            d.segs.append((t, ld, k))
            k0 += k
        assert k0 == v.K
        d.w, _ = _padded(v.w, pad_w, wdt)
        d.bias = v.bias.to(DEV)
        d.res, d.ldr = _padded(v.res, pad_r)
        _LAYOUTS[key] = d
    return _LAYOUTS[key]


def _gate(N, B):
    """Gate table [NSTEPS][B][N] inside rows 4 wider (NaN): returns the CPU table and the device view, whose strides the launch passes on."""
    if (N, B) not in _GATES:
        t = torch.rand(NSTEPS, B, N, generator=torch.Generator().manual_seed(17 * N + B))
        buf = torch.full((NSTEPS, B, N + 4), NAN)
        buf[:, :, :N] = t
        _GATES[(N, B)] = (t, buf.to(DEV)[:, :, :N], torch.tensor([STEP], dtype=torch.int32, device=DEV))
    return _GATES[(N, B)]


GLU = ("geglu", "swiglu")


def _launch(L, d, epi="store", *, bias=True, relu=False, wide=4, shadow=None, rpb=0, rows=None, compute="f32", odt=torch.float32):
    """One v2a_gemm on layout d.  wide: extra columns of the output rows (NaN before and after); shadow: extra columns of the bf16 shadow's
    rows over the OUTPUT's (None: no shadow); rows: launch the first `rows` rows only; RESID reads d.res, GATE_RESID runs in place (the
    residual is the output buffer) with the gate table's own strides and the device step counter at STEP.
    Returns the output's first N (N / 2) columns, the shadow's first N columns (or None)."""
    v = d.v
    M, N = rows or v.M, v.N
    ncols = N // 2 if epi in GLU else N
    ldo = ncols + wide
    out = torch.full((M, ldo), NAN, dtype=odt, device=DEV)
    kw = dict(M=M, N=N, compute=L.F32 if compute == "f32" else L.BF16, ldo=ldo, relu=relu,
              epilogue=dict(store=L.EPI_STORE, sigmoid=L.EPI_SIGMOID, gelu=L.EPI_GELU, geglu=L.EPI_GEGLU, swiglu=L.EPI_SWIGLU, resid=L.EPI_RESID,
                            gate_resid=L.EPI_GATE_RESID)[epi])
    if bias:
        kw["bias"] = d.bias
    if epi == "resid":
        kw.update(resid=d.res, ldr=d.ldr)
    if epi == "gate_resid":
        _, gd, step = _gate(N, (v.M + rpb - 1) // rpb)
        out[:, :N] = d.res[:M]
        kw.update(resid=out, ldr=ldo, gate=gd, step=step, gate_step_stride=gd.stride(0), gate_batch_stride=gd.stride(1), rows_per_batch=rpb)
    sh = None
    if shadow is not None:
        sh = torch.full((M, ldo + shadow), SHADOW_SENTINEL, dtype=torch.bfloat16, device=DEV)
        kw.update(out_bf16=sh, ld_out_bf16=ldo + shadow)
    L.gemm(d.segs, d.w, out, **kw)
    if wide:
        assert bool(torch.isnan(out[:, ncols:]).all()), "columns behind the output's were written"
    if sh is not None:
        assert bool((sh[:, N:] == SHADOW_SENTINEL).all()), "columns behind the shadow's were written"
        sh = sh[:, :N]
    return out[:, :ncols], sh


def _check(what, got, ref, bar, bound=None):
    got = got.float().cpu().double()
    err = (got - ref).abs()
    tail = "" if bound is None else " err/bound=%.3g" % float((err / bound).max())
    print("gemm-fp32 %s err=%.3g%s" % (what, float(err.max()), tail))
    assert not bool(torch.isnan(got).any()), "an element was not written, or a read left the operand's columns"
    torch.testing.assert_close(got, ref, **bar)
    if bound is not None:
        assert bool((err <= bound).all()), float((err - bound).max())


def _check_rel(what, got, ref):
    got = got.cpu().double()
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("gemm-fp32 %s err=%.3g rel=%.3g" % (what, float((got - ref).abs().max()), rel))
    assert not bool(torch.isnan(got).any())
    assert rel <= ACT_REL_BAR, rel


def _check_bf16(what, got, ref):
    got = got.float().cpu().double()
    over = (got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-3)
    print("gemm-fp32 %s bf16 err=%.3g over-bar=%.3g" % (what, float((got - ref).abs().max()), float(over.max())))
    assert not bool(torch.isnan(got).any())
    assert float(over.max()) <= 0, float(over.max())


def _check_equal(what, a, b):
    """torch.equal, with the largest difference printed first (NaN if an element of either side was not written)."""
    diff = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
    print("gemm-fp32 %s equal err=%.3g" % (what, diff))
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any())
    assert torch.equal(a, b)


def _name(v, tile=None):
    return "%dx%dx%d tile=%d" % (v.M, v.N, v.K, tile or tile_of(v.M, v.N))


def _bound(v, r, *terms, **kw):
    return dot_bound(v.K, r.absacc, *terms, **kw) if v.K <= BOUND_MAX_K else None


# ---------------------------------------------------------------------------------------------------------------- 1. the K loop
@pytest.mark.parametrize("K", [16, 32, 48, 64, 80, 1024])
@pytest.mark.parametrize("M,N", [(64, 144), (273, 272)])
def test_k_loop_and_strides(L, M, N, K):
    """1 .. 5 K tiles of 16 and a chain of 64 on either tile: STORE with bias on lda > K, ldw > K, ldo > N against float64 and the fma-chain bound,
    and bit for bit what the dense launch of the same values gives."""
    v = _values(M, N, K)
    r = _ref(v, "f32")
    got, _ = _launch(L, _layout(v, pad_a=4, pad_w=12))
    _check("k-loop %s strided" % _name(v), got, r.z, F32_BAR, _bound(v, r, r.b))
    dense, _ = _launch(L, _layout(v), wide=0)
    _check_equal("k-loop %s strided vs dense" % _name(v), got, dense)


@pytest.mark.parametrize("ks", [(16, 48, 32), (32, 16)])
@pytest.mark.parametrize("M,N", [(64, 144), (273, 272)])
def test_segments_on_single_k_tiles(L, M, N, ks):
    """A segment of one K tile in front, in the middle and at the end, each inside rows wider than its k: RESID with ldr != ldo, equal bit for
    bit to the one-segment launch of the concatenated operand."""
    v = _values(M, N, sum(ks))
    r = _ref(v, "f32")
    got, _ = _launch(L, _layout(v, ks, pad_a=8, pad_r=8), "resid")
    _check("segments %s ks=%s" % (_name(v), "+".join(map(str, ks))), got, r.res + r.z, F32_BAR, _bound(v, r, r.b, r.res.abs()))
    one, _ = _launch(L, _layout(v), "resid", wide=0)
    _check_equal("segments %s ks=%s vs one segment" % (_name(v), "+".join(map(str, ks))), got, one)


@pytest.mark.parametrize("M", [64, 65])
def test_overlapping_rows(L, M):
    """lda = C < K = 3C: row m is rows m .. m + 2 of an (M + 2, C) buffer, the form of Encodec's convolutions; the last row ends with the buffer."""
    N, C = 144, 16
    g = torch.Generator().manual_seed(M)
    buf = torch.randn(M + 2, C, generator=g)
    v = _values(M, N, 3 * C, a=("overlap", buf.as_strided((M, 3 * C), (C, 1)).contiguous()))
    r = _ref(v, "f32")
    d = types.SimpleNamespace(v=v, segs=[(buf.to(DEV), C, 3 * C)], w=v.w.to(DEV), bias=v.bias.to(DEV))
    got, _ = _launch(L, d, relu=True)
    _check("overlap %s lda=%d" % (_name(v), C), got, r.z.clamp_min(0), F32_BAR, _bound(v, r, r.b))
    dense, _ = _launch(L, _layout(v), relu=True)
    _check_equal("overlap %s vs dense rows" % _name(v), got, dense)


# ---------------------------------------------------------------------------------------------------------------- 2. epilogues, fp32 compute
def _epi_operands(M, N, K):
    v = _values(M, N, K)
    return v, _ref(v, "f32"), _layout(v, pad_a=4, pad_w=4, pad_r=8)


@pytest.mark.parametrize("bias,relu", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_store(L, M, N, K, bias, relu):
    v, r, d = _epi_operands(M, N, K)
    got, _ = _launch(L, d, bias=bias, relu=relu)
    ref = r.z if bias else r.acc
    _check("store %s bias=%d relu=%d" % (_name(v), bias, relu), got, ref.clamp_min(0) if relu else ref, F32_BAR,
           _bound(v, r, *([r.b] if bias else [])))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_resid(L, M, N, K, relu):
    """ldr = N + 8 against ldo = N + 4."""
    v, r, d = _epi_operands(M, N, K)
    got, _ = _launch(L, d, "resid", relu=relu)
    ref = r.res + r.z
    _check("resid %s relu=%d" % (_name(v), relu), got, ref.clamp_min(0) if relu else ref, F32_BAR, _bound(v, r, r.b, r.res.abs()))


def _gate_ref(v, r, rpb, M=None):
    table, _, _ = _gate(v.N, (v.M + rpb - 1) // rpb)
    g = gate_rows(table, STEP, v.M, rpb).double()
    return (r.res + g * r.z)[:M], g[:M]


@pytest.mark.parametrize("rpb", [23, 150])
@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_gate_resid_in_place(L, M, N, K, rpb):
    """out == resid; gate table [steps][batches][N] at device step 3 of 5, both strides the table's own; a batch element ends inside a 16-row
    MFMA slab (23) and the last one is partial (150, and 23 on every shape)."""
    v, r, d = _epi_operands(M, N, K)
    got, _ = _launch(L, d, "gate_resid", rpb=rpb)
    ref, g = _gate_ref(v, r, rpb)
    _check("gate-resid %s rpb=%d" % (_name(v), rpb), got, ref, F32_BAR, _bound(v, r, r.b, r.res.abs(), gate=g))


@pytest.mark.parametrize("epi", ["store_relu", "resid", "gate_resid"])
@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_bf16_shadow(L, M, N, K, epi):
    """out_bf16 with ld_out_bf16 = ldo + 8: bfloat16() of the stored fp32 value, after the relu."""
    v, r, d = _epi_operands(M, N, K)
    if epi == "store_relu":
        got, sh = _launch(L, d, relu=True, shadow=8)
        ref, bound = r.z.clamp_min(0), _bound(v, r, r.b)
    elif epi == "resid":
        got, sh = _launch(L, d, "resid", shadow=8)
        ref, bound = r.res + r.z, _bound(v, r, r.b, r.res.abs())
    else:
        got, sh = _launch(L, d, "gate_resid", rpb=23, shadow=8)
        ref, g = _gate_ref(v, r, 23)
        bound = _bound(v, r, r.b, r.res.abs(), gate=g)
    _check("shadow %s %s" % (epi, _name(v)), got, ref, F32_BAR, bound)
    assert torch.equal(sh, got.bfloat16())
    if epi == "store_relu":
        assert bool((got == 0).any()) and bool((sh >= 0).all())               # the relu cut something, and the shadow is the value behind it


@pytest.mark.parametrize("N", [144, 272])
def test_sigmoid_gate_table_form(L, N):
    """M = 3 rows (one per step of a gate table) on the 128x128 tile, as the AdaLN gate tables are made."""
    v = _values(3, N, 48)
    r = _ref(v, "f32")
    got, _ = _launch(L, _layout(v, pad_a=4, pad_w=4), "sigmoid")
    _check("sigmoid %s" % _name(v), got, torch.sigmoid(r.z), SIGMOID_BAR)


@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_gelu(L, M, N, K):
    v, r, d = _epi_operands(M, N, K)
    got, _ = _launch(L, d, "gelu")
    _check_rel("gelu %s" % _name(v), got, torch.nn.functional.gelu(r.z))


def _glu_ref(r, epi):
    val, gt = glu_unpack(r.z)
    return val * (torch.nn.functional.gelu(gt) if epi == "geglu" else torch.nn.functional.silu(gt))


@pytest.mark.parametrize("epi", GLU)
@pytest.mark.parametrize("M,N,K", GLU_CASES + [BIG + (BIG_K,)])
def test_glu(L, M, N, K, epi):
    """W rows packed [16 value | 16 gate]; N / 2 output columns in rows 4 wider."""
    v, r, d = _epi_operands(M, N, K)
    got, _ = _launch(L, d, epi)
    _check_rel("%s %s" % (epi, _name(v)), got, _glu_ref(r, epi))


@pytest.mark.parametrize("M,N", [(1, 20), (130, 1), (130, 3)])
def test_edges(L, M, N):
    """One row; N no multiple of 16; N = 1 and 3 with output, residual and shadow rows that are not 16-byte aligned (ldo = N + 2, ldr = N + 1)."""
    v = _values(M, N, 48)
    r = _ref(v, "f32")
    d = _layout(v, pad_a=4, pad_w=4, pad_r=1)
    got, _ = _launch(L, d, wide=2)
    _check("edge store %s" % _name(v), got, r.z, F32_BAR, _bound(v, r, r.b))
    got, sh = _launch(L, d, "resid", relu=True, wide=2, shadow=1)
    _check("edge resid+relu %s" % _name(v), got, (r.res + r.z).clamp_min(0), F32_BAR, _bound(v, r, r.b, r.res.abs()))
    assert torch.equal(sh, got.bfloat16())
    got, _ = _launch(L, d, "gate_resid", wide=2, rpb=23)
    ref, g = _gate_ref(v, r, 23)
    _check("edge gate-resid %s" % _name(v), got, ref, F32_BAR, _bound(v, r, r.b, r.res.abs(), gate=g))


# ---------------------------------------------------------------------------------------------------------------- 3. bit equality, fp32 compute
_EQ_EPIS = ["store", "resid_relu", "gate_resid", "geglu"]


def _eq_launch(L, d, epi, rows=None):
    if epi == "resid_relu":
        return _launch(L, d, "resid", relu=True, rows=rows)[0]
    if epi == "gate_resid":
        return _launch(L, d, "gate_resid", rpb=23, rows=rows)[0]
    return _launch(L, d, epi, rows=rows)[0]


@pytest.mark.parametrize("epi", _EQ_EPIS)
def test_tiles_agree_bit_for_bit_big(L, epi):
    """Rows 0 .. 199 of the (1800, 1920) launch (128x128 tiles, by the tile count) equal the launch of those rows alone (64x64 tiles)."""
    assert tile_of(*BIG) == 128 and tile_of(BIG_ROWS, BIG[1]) == 64
    v, r, d = _epi_operands(*BIG, BIG_K)
    full, part = _eq_launch(L, d, epi), _eq_launch(L, d, epi, rows=BIG_ROWS)
    _check_equal("tiles %s %s rows 0..%d tile=128 vs tile=64" % (epi, _name(v), BIG_ROWS - 1), full[:BIG_ROWS], part)


@pytest.mark.parametrize("epi", _EQ_EPIS)
def test_tiles_agree_bit_for_bit_small(L, epi):
    """Rows 0 .. 63 of a 65-row launch (64x64 tiles) equal the launch of 64 rows (one 128x128 band)."""
    N = 160 if epi == "geglu" else 144
    assert tile_of(65, N) == 64 and tile_of(64, N) == 128
    v, r, d = _epi_operands(65, N, 48)
    full, part = _eq_launch(L, d, epi), _eq_launch(L, d, epi, rows=64)
    _check_equal("tiles %s %s rows 0..63 tile=64 vs tile=128" % (epi, _name(v)), full[:64], part)


@pytest.mark.parametrize("rows", [1, 16, 64, 65, 129])
def test_a_row_does_not_depend_on_m(L, rows):
    """The batch independence gemm_prepare promises: the first rows of a (273, 272) launch, launched alone (on either tile, with other row
    bands and another XCD remap), come out the same bit for bit."""
    v, r, d = _epi_operands(273, 272, 80)
    full = _launch(L, d, "resid")[0]
    part = _launch(L, d, "resid", rows=rows)[0]
    _check_equal("rows %s first %d alone (tile=%d)" % (_name(v), rows, tile_of(rows, 272)), full[:rows], part)


@pytest.mark.parametrize("M,N,K", EPI_CASES)
def test_strides_do_not_change_the_result(L, M, N, K):
    """lda, ldw, ldo, ldr and the shadow's stride wider than dense: the same bits as the dense launch."""
    v, r, d = _epi_operands(M, N, K)
    dense = _layout(v)
    for epi, kw in (("store", dict(relu=True)), ("resid", {}), ("gate_resid", dict(rpb=150))):
        a, sa = _launch(L, d, epi, shadow=8, **kw)
        b, sb = _launch(L, dense, epi, wide=0, shadow=0, **kw)
        _check_equal("strides %s %s vs dense" % (epi, _name(v)), a, b)
        assert torch.equal(sa, sb), epi


# ---------------------------------------------------------------------------------------------------------------- 4. bf16 compute on fp32 A
AF32_SHAPES = [(65, 144), (273, 272)]
AF32_KS = [(64,), (128,), (192,), (64, 128)]


def _af32_operands(M, N, ks):
    v = _values(M, N, sum(ks))
    return v, _ref(v, "bf16"), _layout(v, ks, pad_a=4, pad_w=8, pad_r=8, wdt=torch.bfloat16)


def _ks_name(ks):
    return "ks=" + "+".join(map(str, ks))


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ks", AF32_KS)
@pytest.mark.parametrize("M,N", AF32_SHAPES)
def test_a_f32_store(L, M, N, ks, odt):
    v, r, d = _af32_operands(M, N, ks)
    got, _ = _launch(L, d, compute="bf16", odt=odt)
    what = "a_f32 store %s %s" % (_name(v, 128), _ks_name(ks))
    if odt == torch.float32:
        _check(what, got, r.z, BF16_COMPUTE_BAR)
    else:
        _check_bf16(what, got, r.z)


@pytest.mark.parametrize("ks", AF32_KS)
@pytest.mark.parametrize("M,N", AF32_SHAPES)
def test_a_f32_resid_relu_with_shadow(L, M, N, ks):
    v, r, d = _af32_operands(M, N, ks)
    got, sh = _launch(L, d, "resid", relu=True, shadow=8, compute="bf16")
    _check("a_f32 resid+relu %s %s" % (_name(v, 128), _ks_name(ks)), got, (r.res + r.z).clamp_min(0), BF16_COMPUTE_BAR)
    assert torch.equal(sh, got.bfloat16())


@pytest.mark.parametrize("rpb", [23, 150])
@pytest.mark.parametrize("ks", AF32_KS)
@pytest.mark.parametrize("M,N", AF32_SHAPES)
def test_a_f32_gate_resid(L, M, N, ks, rpb):
    v, r, d = _af32_operands(M, N, ks)
    got, _ = _launch(L, d, "gate_resid", rpb=rpb, compute="bf16")
    _check("a_f32 gate-resid %s %s rpb=%d" % (_name(v, 128), _ks_name(ks), rpb), got, _gate_ref(v, r, rpb)[0], BF16_COMPUTE_BAR)


@pytest.mark.parametrize("ks", AF32_KS)
@pytest.mark.parametrize("M,N", [(65, 96), (273, 160)])
def test_a_f32_geglu_to_bf16(L, M, N, ks):
    v, r, d = _af32_operands(M, N, ks)
    got, _ = _launch(L, d, "geglu", compute="bf16", odt=torch.bfloat16)
    _check_bf16("a_f32 geglu %s %s" % (_name(v, 128), _ks_name(ks)), got, _glu_ref(r, "geglu"))


@pytest.mark.parametrize("M,N", AF32_SHAPES)
def test_a_f32_conversion_rounds_ties_to_even(L, M, N):
    """Every A element lies exactly between two bf16 values.  The reference rounds with torch's bfloat16() (nearest even); half-up or truncation
    in the kernel's load would move every product by a bf16 ulp of its A factor, ~2^-9 of the result against a bar of 1e-4.  The launch on the
    pre-rounded values (whose conversion is exact) gives the same bits."""
    K = 128
    a = tie_inputs(M, K, 3 * M + N)
    v = _values(M, N, K, a=("ties", a))
    r = _ref(v, "bf16")
    got, _ = _launch(L, _layout(v, pad_a=4, pad_w=8, wdt=torch.bfloat16), compute="bf16")
    _check("a_f32 ties %s" % _name(v, 128), got, r.z, BF16_COMPUTE_BAR)
    w = _values(M, N, K, a=("ties-rounded", a.bfloat16().float()))
    assert torch.equal(w.w, v.w) and torch.equal(w.bias, v.bias)
    pre, _ = _launch(L, _layout(w, pad_a=4, pad_w=8, wdt=torch.bfloat16), compute="bf16")
    _check_equal("a_f32 ties %s vs pre-rounded A" % _name(v, 128), got, pre)


# ---------------------------------------------------------------------------------------------------------------- 5. bf16 x bf16 SIGMOID
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("M,N", [(3, 144), (273, 272)])
def test_bf16_sigmoid(L, M, N, K):
    """bf16 A and W, fp32 output: the instantiation v2a_gemm keeps on this kernel because the ring kernels have no SIGMOID epilogue."""
    v = _values(M, N, K)
    r = _ref(v, "bf16")
    d = _layout(v, pad_a=8, pad_w=8, adt=torch.bfloat16, wdt=torch.bfloat16)
    got, _ = _launch(L, d, "sigmoid", compute="bf16")
    _check("bf16 sigmoid %s" % _name(v, 128), got, torch.sigmoid(r.z), BF16_COMPUTE_BAR)
