"""GPU: the split-operand ring GEMM (csrc/gemm.hip, gemm_bf16_dma_kernel with S3 = true: a_dtype V2A_BF16_SPLIT, the bf16x3 mode) on every tile
shape it is built for, against float64 and against each other.

v2a_gemm_args.tile_hint picks the instantiation on split operands:

  hint  tile, waves, ring, K per stage   wave tile  note
  1     64x64,   2x2, 3-deep, 64         32x32      REF: every other shape is compared with it bit for bit
  2     128x64,  2x2, 3-deep, 64         64x32
  3     128x128, 2x4, 2-deep, 64         64x32      the only 2-deep ring (ring_wait<0>: vmcnt(0))
  4     64x128,  2x4, 3-deep, 64         32x32
  6     128x256, 2x4, 3-deep, 32         64x64      STORE and GATE_RESID take the pipelined, non-prefetched epilogue; shipped for the frames stream
  7     128x128, 2x4, 3-deep, 32         64x32
  0     by shape: 1 at the shapes here (4 for GEGLU / SWIGLU)
  5     the 256x256 8-phase kernel (csrc/gemm_8phase.hip): joins only where its sum order is compared with the ring's

Every 32-wide k step adds A_lo W_hi, A_hi W_lo, A_hi W_hi in that order to one accumulator chain, on 64-wide stages (two steps per stage) and on
32-wide ones alike, and the 8-phase kernel forms the same three products per 32 logical k in the same order: the K order of an output element does
not depend on the shape, so STORE / RESID / GATE_RESID results (and the fused RoPE, one fixed contraction) must be equal bit for bit.

Operands come from seeded CPU generators: fp32 a ~ N(0, 1), w ~ N(0, 1) / sqrt(K), split by hi = bf16(x), lo = bf16(x - hi), W as [W_hi | W_lo].
References are float64 products of the fp32 operands.  Outputs are prefilled with NaN, shadows and sums with a sentinel: an element nobody
wrote fails.  Bars (all taken from the existing tests, none from what this file measured):
  fp32 outputs    3e-5 max(max |acc|, 1)     test_gemm_split_native (three bf16 MFMA products per fp32 product leave ~1e-5 relative)
  GEGLU           4e-5 max(max |ref|, 1)     test_gemm_split_native
  GELU / SWIGLU   2e-5 max |ref|             test_clip_gpu, test_dinov2_gpu
  row_ssq         5e-5 max |ref|             test_gemm_split_native_folded_norm_consumer
  norm_ssq        rtol 1e-5, atol 1e-6 against float64 of the stored output
  shadows         bit equality with _split_planes(out [* gamma row])
  GEGLU / SWIGLU / GELU are not compared between shapes (the store forms may lower exp differently).

Sections: 1 the K loop (1 .. 7 stages of 64, 2 .. 14 of 32: fewer stages than the ring holds, as many, every residue modulo depths 2 and 3);
2 segment switches in the prologue, on consecutive stages and twice in the first ring trip, on two operand layouts; 3 every epilogue at ragged
tile edges -- (273, 272 | 288) a second band of 17 rows and a 16- / 32-column last tile, (28, 512) one partial slab, (333, 416) full and partial
wave tiles in one launch, a batch element ending inside the launch; 4 refusals; 5 the shipped calls of the frames and audio streams in miniature.

Every case prints its largest error ("split-ring <what> hint=<h> err=<e> bar=<b> (<e / b>)") before it asserts.  Largest errors measured on
the MI355X, 453 cases in 1.5 s (no bar was set from them):
  1 K loop            2.7e-5 of 1.4e-4 (K = 64), the same on every hint: all of 1, 2, 3, 4, 6, 7 and 5 equal bit for bit at every K
  2 segments          2.1e-5 of 1.2e-4; layouts, the one-segment call and REF equal bit for bit on every hint
  3 STORE / RoPE      2.2e-5 / 2.3e-5 of 1.2e-4        RESID (+ relu) 2.2e-5 (1.9e-5) of 1.2e-4     GATE_RESID, producer 2.2e-5 of 1.5e-4
    norm_ssq          1.4e-7 relative                  row_ssq 1.4e-4 of 7.6e-4 (GEGLU, hint 6)     GEGLU 6.5e-5 of 3.8e-4
    SWIGLU            5.7e-5 of 1.8e-4 (planes)        GELU 3.0e-5 of 8.2e-5 (planes)
    0, 1, 2, 3, 4, 6, 7 equal bit for bit on STORE / RoPE / RESID / GATE_RESID, shadows and norm_ssq included; 5 on the fp32 outputs of the four
  5 shipped calls     2.7e-5 of 1.2e-4 (frames out, hint 6); q2 3.2e-5 of 3.3e-4; equal to REF bit for bit"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
RING = [1, 2, 3, 4, 6, 7]
REF = 1                          # 64x64, 2x2 waves, 3-deep ring, 64-wide stages
HINT_8PHASE = 5
EPI_HINTS = RING + [0]
SHAPES = [(273, 272), (28, 512), (333, 416)]
SHAPES32 = [(273, 288), (28, 512), (333, 416)]      # for the epilogues that need N % 32 == 0
RPB = {273: 150, 28: 23, 333: 150}                  # a batch element ends inside the launch
SWITCH_ROW = {273: 100, 28: 9, 333: 100}            # strictly inside a tile
K_EPI = 128
K_LOOP = [64, 128, 192, 256, 320, 384, 448]
STEP, NSTEPS = 3, 5
ROPE_OFF = 5
NORM_DIM = 192                                      # row_ssq: 6 partial sums, the row padded to 8 with zeros
NAN = float("nan")
SHADOW_SENTINEL, SSQ_SENTINEL = -3.0, -1.0


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------------------- float64 reference helpers
# (checked against torch and against each other on the CPU by tests/test_gemm_split_ring_refs.py)
def _split_planes(x):
    """fp32 (rows, k) -> bf16 (rows, 2k) = [hi | lo] (the V2A_BF16_SPLIT layout)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, lo], -1).contiguous()


def _rope_table(n):
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(n).float()[:, None] * inv[None, :]
    return torch.stack((ang.cos(), ang.sin()), -1).contiguous()


def _rope_ref(z, tab, rope_cols, rows_per_batch, pos_offset):
    """fp64: interleaved pairs (2i, 2i + 1) of every 64-column head of the first rope_cols columns rotated by the table row of the position."""
    M = z.shape[0]
    pos = torch.arange(M) % rows_per_batch + pos_offset
    cos, sin = tab[pos, :, 0].double(), tab[pos, :, 1].double()              # (M, 32)
    x = z[:, :rope_cols].reshape(M, rope_cols // 64, 32, 2)
    even = x[..., 0] * cos[:, None] - x[..., 1] * sin[:, None]
    odd = x[..., 1] * cos[:, None] + x[..., 0] * sin[:, None]
    out = z.clone()
    out[:, :rope_cols] = torch.stack((even, odd), -1).reshape(M, rope_cols)
    return out


def _glu_perm(N):
    """Rows of a [N / 2 value | N / 2 gate] weight in the order the GLU epilogues want them: [16 value | 16 gate] per 16 outputs."""
    half = N // 2
    return torch.cat([torch.cat([torch.arange(j * 16, j * 16 + 16), half + torch.arange(j * 16, j * 16 + 16)]) for j in range(half // 16)])


def _glu_unpack(z):
    """(M, N) pre-activations of packed rows -> the (M, N / 2) values and gates."""
    M, N = z.shape
    z = z.reshape(M, N // 32, 2, 16)
    return z[:, :, 0].reshape(M, N // 2), z[:, :, 1].reshape(M, N // 2)


def _gate_rows(gate, step, M, rpb):
    """gate (steps, batch, N) -> the (M, N) gate of every row: table row [step][m / rpb]."""
    return gate[step][torch.arange(M) // rpb]


def _gamma_rows(gam, step, M, rpb, switch_row):
    """gam (steps, batch, 2, N) -> the (M, N) gamma of every row: [step][m / rpb][m >= switch_row]."""
    m = torch.arange(M)
    return gam[step][m // rpb, (m >= switch_row).long()]


# ------------------------------------------------------------------------------------------------------------- operands, made once per shape
_OPS, _REF = {}, {}


def _operands(M, N, ks=(K_EPI,)):
    """fp32 operands of one (M, N, K segments), their split device copies ([hi | lo] rows, one standard segment per entry of ks) and the
    float64 product; made once, shared by the cases of that shape, never modified."""
    key = (M, N, tuple(ks))
    if key not in _OPS:
        K = sum(ks)
        g = torch.Generator().manual_seed(1000 * M + N + 7 * K + len(ks))
        a = [torch.randn(M, k, generator=g) for k in ks]
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = 0.1 * torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g)
        acc = torch.cat(a, 1).double() @ w.double().t()
        _OPS[key] = dict(M=M, N=N, ks=tuple(ks), a=a, segs=[(_split_planes(x).to(DEV), 2 * k, k) for x, k in zip(a, ks)],
                         w=_split_planes(w).to(DEV), bias=bias.to(DEV), res=res.to(DEV), acc=acc, z=acc + bias.double(), res64=res.double(),
                         scale=max(float(acc.abs().max()), 1.0))
    return _OPS[key]


def _gemm(L, o, out, hint, segs=None, **kw):
    kw.setdefault("bias", o["bias"])
    L.gemm(segs if segs is not None else o["segs"], o["w"], out, M=o["M"], N=o["N"], compute=L.BF16, a_split=True, tile_hint=hint, **kw)
    return out


def _nan_out(o, dtype=torch.float32, cols=None):
    return torch.full((o["M"], cols or o["N"]), NAN, dtype=dtype, device=DEV)


def _shadow(o, cols=None):
    return torch.full((o["M"], cols or 2 * o["N"]), SHADOW_SENTINEL, dtype=torch.bfloat16, device=DEV)


def _ref(key, launch):
    """The same call on tile_hint REF, launched once per case key and shared."""
    if key not in _REF:
        _REF[key] = launch(REF)
    return _REF[key]


def _check(what, hint, got, ref, bar):
    got = got.cpu().double()
    err = float((got - ref).abs().max())
    print("split-ring %s hint=%d err=%.3g bar=%.3g (%.2f)" % (what, hint, err, bar, err / bar))
    assert not bool(torch.isnan(got).any())
    assert err < bar, (err, bar)


def _check_f32(what, hint, got, ref, o):
    _check(what, hint, got, ref, 3e-5 * o["scale"])


def _planes_sum(t, n):
    """(M, >= 2n) hi | lo planes -> their fp64 sum."""
    t = t.float().cpu().double()
    return t[:, :n] + t[:, n:2 * n]


def _assert_shadow(sh, of):
    """A split shadow is the planes of the fp32 value it shadows, bit for bit."""
    assert torch.equal(sh.cpu(), _split_planes(of.cpu()))


# ------------------------------------------------------------------------------------------------------------- 1. the K loop
@pytest.mark.parametrize("K", K_LOOP)
@pytest.mark.parametrize("hint", RING)
def test_k_loop(L, hint, K):
    """1 .. 7 stages of 64 k (2 .. 14 of 32): the prologue guard with fewer stages than the ring issues ahead, exactly as many, and every residue of
    the unrolled ring of depth 2 and 3; ragged M and N, fp32 STORE with a bias.  Float64 parity, and bit for bit what REF gives."""
    o = _operands(333, 456, (K,))
    run = lambda h: _gemm(L, o, _nan_out(o), h)
    got = run(hint)
    _check_f32("k-loop K=%d" % K, hint, got, o["z"], o)
    assert torch.equal(got, _ref(("k-loop", K), run))


@pytest.mark.parametrize("K", K_LOOP)
def test_k_loop_8phase_sums_in_ring_order(L, K):
    """tile_hint 5, the 8-phase kernel (2 .. 14 stages of 32 logical k): per 32 k the same three products in the same order into one accumulator
    chain, so its STORE result equals the ring's bit for bit."""
    o = _operands(333, 456, (K,))
    run = lambda h: _gemm(L, o, _nan_out(o), h)
    got = run(HINT_8PHASE)
    _check_f32("k-loop 8-phase K=%d" % K, HINT_8PHASE, got, o["z"], o)
    assert torch.equal(got, _ref(("k-loop", K), run))


# ------------------------------------------------------------------------------------------------------------- 2. segment switches
SEG_KS = [(64, 128, 64), (64, 64, 64), (128, 64, 192)]      # a switch in the prologue / on consecutive stages / twice within the first ring trip
_LAYOUTS = {}


def _layouts(o):
    """The A operand of a three-segment case in three layouts (made once per case):
    strided -- three standard segments in rows wider than 2k (strides 2k + 64, + 128, + 192), the padding filled with ones;
    wide    -- the first two as the halves of one [x_hi | s_hi | x_lo | s_lo] buffer (lo plane k0 + k1 further, not k), the third standard;
    cat     -- one standard segment of the concatenated operand."""
    key = (o["M"], o["N"], o["ks"])
    if key not in _LAYOUTS:
        M, (k0, k1, k2) = o["M"], o["ks"]
        planes = [_split_planes(x) for x in o["a"]]
        strided = []
        for i, (pl, k) in enumerate(zip(planes, o["ks"])):
            ld = 2 * k + 64 * (i + 1)
            buf = torch.ones(M, ld, dtype=torch.bfloat16)
            buf[:, :2 * k] = pl
            strided.append((buf.to(DEV), ld, k))
        xs, ss = planes[0], planes[1]
        wide = torch.cat([xs[:, :k0], ss[:, :k1], xs[:, k0:], ss[:, k1:]], 1).contiguous().to(DEV)
        d2 = k0 + k1
        wide_segs = [(wide, 2 * d2, k0, d2), (wide[:, k0:], 2 * d2, k1, d2), (planes[2].to(DEV), 2 * k2, k2)]
        K = sum(o["ks"])
        cat = [(_split_planes(torch.cat(o["a"], 1)).to(DEV), 2 * K, K)]
        _LAYOUTS[key] = dict(strided=strided, wide=wide_segs, cat=cat)
    return _LAYOUTS[key]


@pytest.mark.parametrize("epi", ["store", "resid_shadow"])
@pytest.mark.parametrize("ks", SEG_KS)
@pytest.mark.parametrize("M", [273, 28])
@pytest.mark.parametrize("hint", RING)
def test_segment_switches(L, hint, M, ks, epi):
    """The countdown that switches a_run, the lo-plane distance and the row stride, while the ring is still filling and on consecutive stages, with
    different hi -> lo distances per segment.  Float64 parity; the layouts equal each other, the one-segment call and REF bit for bit."""
    o = _operands(M, 512, ks)
    lay = _layouts(o)

    def run(h, segs):
        if epi == "store":
            return (_gemm(L, o, _nan_out(o), h, segs=segs),)
        sh = _shadow(o)
        out = _gemm(L, o, _nan_out(o), h, segs=segs, epilogue=L.EPI_RESID, resid=o["res"], out_bf16=sh, ld_out_bf16=2 * o["N"], out_bf16_split=True)
        return out, sh

    got = run(hint, lay["strided"])
    exact = o["z"] if epi == "store" else o["res64"] + o["z"]
    _check_f32("segments %s M=%d ks=%s" % (epi, M, ks), hint, got[0], exact, o)
    if epi != "store":
        _assert_shadow(got[1], got[0])
    ref = _ref(("segments", M, ks, epi), lambda h: run(h, lay["strided"]))
    for name in ("wide", "cat"):
        other = run(hint, lay[name])
        for x, y in zip(got, other):
            assert torch.equal(x, y), name
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------- 3. epilogues at ragged tile edges
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_store(L, hint, M, N):
    o = _operands(M, N)
    run = lambda h: _gemm(L, o, _nan_out(o), h, rows_per_batch=RPB[M])
    got = run(hint)
    _check_f32("store %dx%d" % (M, N), hint, got, o["z"], o)
    assert torch.equal(got, _ref(("store", M, N), run))


def _rope_kw(M, N):
    rope_cols = 256 if N >= 256 else 128
    tab = _rope_table(ROPE_OFF + RPB[M])
    return tab, rope_cols, dict(rope_table=tab.to(DEV), rope_cols=rope_cols, rope_pos_offset=ROPE_OFF, rows_per_batch=RPB[M])


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_store_rope_positions_wrap(L, hint, M, N):
    """STORE + fused RoPE over the first 256 columns at position offset 5; positions wrap at rows_per_batch inside the launch (150: inside the
    second 64-row band; 23: inside a slab).  rope_rotate4 is one fixed contraction: equal to REF bit for bit."""
    o = _operands(M, N)
    tab, rope_cols, kw = _rope_kw(M, N)
    run = lambda h: _gemm(L, o, _nan_out(o), h, **kw)
    got = run(hint)
    _check_f32("rope %dx%d" % (M, N), hint, got, _rope_ref(o["z"], tab, rope_cols, RPB[M], ROPE_OFF), o)
    assert torch.equal(got, _ref(("rope", M, N), run))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_resid_split_shadow(L, hint, M, N, relu):
    """RESID (and RESID + relu) with a split shadow of row stride 2N; once more with the shadow in the second half of a 4N-wide buffer
    ([. | hi | . | lo], out_bf16_lo_offset = 2N): equal plane by plane, the other half untouched."""
    o = _operands(M, N)
    kw = dict(epilogue=L.EPI_RESID, resid=o["res"], out_bf16_split=True, relu=relu, rows_per_batch=RPB[M])

    def run(h):
        sh = _shadow(o)
        return _gemm(L, o, _nan_out(o), h, out_bf16=sh, ld_out_bf16=2 * N, **kw), sh

    out, sh = run(hint)
    exact = o["res64"] + o["z"]
    _check_f32("resid%s %dx%d" % ("+relu" if relu else "", M, N), hint, out, exact.clamp_min(0) if relu else exact, o)
    _assert_shadow(sh, out)
    wide = _shadow(o, 4 * N)
    out2 = _gemm(L, o, _nan_out(o), hint, out_bf16=wide[:, N:], ld_out_bf16=4 * N, out_bf16_lo_offset=2 * N, **kw)
    assert torch.equal(out2, out)
    assert torch.equal(wide[:, N:2 * N], sh[:, :N]) and torch.equal(wide[:, 3 * N:], sh[:, N:])
    assert bool((wide[:, :N] == SHADOW_SENTINEL).all()) and bool((wide[:, 2 * N:3 * N] == SHADOW_SENTINEL).all())
    ref_out, ref_sh = _ref(("resid", M, N, relu), run)
    assert torch.equal(out, ref_out) and torch.equal(sh, ref_sh)


_TABLES = {}


def _tables(M, N):
    """Gate (steps, batch, N) and gamma (steps, batch, 2, N) tables of a shape, on the host and on the device."""
    if (M, N) not in _TABLES:
        B = (M + RPB[M] - 1) // RPB[M]
        g = torch.Generator().manual_seed(17 * N + M)
        gate = torch.rand(NSTEPS, B, N, generator=g)
        gam = 1.0 + 0.3 * torch.randn(NSTEPS, B, 2, N, generator=g)
        _TABLES[(M, N)] = dict(gate=gate, gam=gam, gate_d=gate.to(DEV), gam_d=gam.to(DEV), step=torch.tensor([STEP], dtype=torch.int32, device=DEV))
    return _TABLES[(M, N)]


def _gate_kw(L, t, M):
    gd = t["gate_d"]
    return dict(epilogue=L.EPI_GATE_RESID, gate=gd, step=t["step"], gate_step_stride=gd.stride(0), gate_batch_stride=gd.stride(1), rows_per_batch=RPB[M])


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_gate_resid_step_and_batch(L, hint, M, N):
    """GATE_RESID in place on the residual: the gate row is [device step 3 of 5][batch element], both strides non-zero, with a bias."""
    o = _operands(M, N)
    t = _tables(M, N)

    def run(h):
        out = o["res"].clone()
        return _gemm(L, o, out, h, resid=out, **_gate_kw(L, t, M))

    got = run(hint)
    _check_f32("gate %dx%d" % (M, N), hint, got, o["res64"] + _gate_rows(t["gate"], STEP, M, RPB[M]).double() * o["z"], o)
    assert torch.equal(got, _ref(("gate", M, N), run))


@pytest.mark.parametrize("M,N", SHAPES32)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_gate_resid_folded_norm_producer(L, hint, M, N):
    """GATE_RESID as the producer of a folded RMSNorm: gamma [step][batch element][slot], the second slot from a switch row strictly inside a
    tile; split shadow = planes of out * gamma row, sums of squares per 32 columns; the fp32 output is that of the unfolded call."""
    o = _operands(M, N)
    t = _tables(M, N)
    gd = t["gam_d"]
    sw = SWITCH_ROW[M]
    kw = dict(resid=o["res"], **_gate_kw(L, t, M))
    nkw = dict(norm_gamma=gd, norm_step_stride=gd.stride(0), norm_batch_stride=gd.stride(1), norm_switch_row=sw, norm_switch_offset=gd.stride(2))

    def run(h):
        sh, ssq = _shadow(o), torch.full((M, N // 32), SSQ_SENTINEL, device=DEV)
        return _gemm(L, o, _nan_out(o), h, out_bf16=sh, ld_out_bf16=2 * N, out_bf16_split=True, norm_ssq=ssq, **nkw, **kw), sh, ssq

    out, sh, ssq = run(hint)
    plain = _gemm(L, o, _nan_out(o), hint, **kw)
    _check_f32("producer %dx%d" % (M, N), hint, out, o["res64"] + _gate_rows(t["gate"], STEP, M, RPB[M]).double() * o["z"], o)
    assert torch.equal(out, plain)                                          # the fp32 result is untouched by the fold
    _assert_shadow(sh, out.cpu() * _gamma_rows(t["gam"], STEP, M, RPB[M], sw))
    ref = (out.cpu().double() ** 2).reshape(M, N // 32, 32).sum(-1)
    print("split-ring producer %dx%d hint=%d ssq rel err=%.3g" % (M, N, hint, float(((ssq.cpu().double() - ref).abs() / ref).max())))
    torch.testing.assert_close(ssq.cpu().double(), ref, rtol=1e-5, atol=1e-6)
    for x, y in zip((out, sh, ssq), _ref(("producer", M, N), run)):         # the sums too: one butterfly over the 8 lanes of 32 columns
        assert torch.equal(x, y)


_SSQ = {}


def _row_ssq(M):
    """Partial sums of squares of the rows of a NORM_DIM-wide producer (6 of 8 columns used) and the scale they stand for."""
    if M not in _SSQ:
        ssq = torch.zeros(M, 8)
        ssq[:, :NORM_DIM // 32] = torch.rand(M, NORM_DIM // 32, generator=torch.Generator().manual_seed(M)) * 40 + 1
        _SSQ[M] = (ssq.to(DEV), math.sqrt(NORM_DIM) / ssq.double().sum(-1).sqrt().clamp_min(1e-12))
    return _SSQ[M]


@pytest.mark.parametrize("epi", ["store", "store_rope", "geglu"])
@pytest.mark.parametrize("M,N", SHAPES32)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_row_ssq_consumer(L, hint, M, N, epi):
    """row_ssq: accumulator row m is scaled by sqrt(d) / max(sqrt(sum of its partial sums), 1e-12) before bias / RoPE / GEGLU."""
    o = _operands(M, N)
    ssq, rstd = _row_ssq(M)
    z = o["acc"] * rstd[:, None] + o["bias"].cpu().double()
    kw = dict(row_ssq=ssq, row_norm_dim=NORM_DIM)
    if epi == "store":
        got, ref = _gemm(L, o, _nan_out(o), hint, rows_per_batch=RPB[M], **kw), z
    elif epi == "store_rope":
        tab, rope_cols, rkw = _rope_kw(M, N)
        got, ref = _gemm(L, o, _nan_out(o), hint, **rkw, **kw), _rope_ref(z, tab, rope_cols, RPB[M], ROPE_OFF)
    else:
        out = _gemm(L, o, _nan_out(o, torch.bfloat16), hint, epilogue=L.EPI_GEGLU, ldo=N, out_split=True, **kw)
        v, gt = _glu_unpack(z)
        got, ref = _planes_sum(out, N // 2), v * torch.nn.functional.gelu(gt)
    _check("consumer %s %dx%d" % (epi, M, N), hint, got, ref, 5e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("M,N", SHAPES32)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_geglu_split_output(L, hint, M, N):
    """GEGLU on W rows packed [16 value | 16 gate], output as hi | lo planes of the N / 2 hidden values (lo plane N / 2 further)."""
    o = _operands(M, N)
    out = _gemm(L, o, _nan_out(o, torch.bfloat16), hint, epilogue=L.EPI_GEGLU, ldo=N, out_split=True)
    v, gt = _glu_unpack(o["z"])
    ref = v * torch.nn.functional.gelu(gt)
    _check("geglu %dx%d" % (M, N), hint, _planes_sum(out, N // 2), ref, 4e-5 * max(float(ref.abs().max()), 1.0))


@pytest.mark.parametrize("split_out", [False, True])
@pytest.mark.parametrize("M,N", SHAPES32)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_swiglu(L, hint, M, N, split_out):
    o = _operands(M, N)
    v, gt = _glu_unpack(o["z"])
    ref = v * torch.nn.functional.silu(gt)
    if split_out:
        got = _planes_sum(_gemm(L, o, _nan_out(o, torch.bfloat16), hint, epilogue=L.EPI_SWIGLU, ldo=N, out_split=True), N // 2)
    else:
        got = _gemm(L, o, _nan_out(o, cols=N // 2), hint, epilogue=L.EPI_SWIGLU)
    _check("swiglu %s %dx%d" % ("planes" if split_out else "fp32", M, N), hint, got, ref, 2e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("split_out", [False, True])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", EPI_HINTS)
def test_gelu(L, hint, M, N, split_out):
    o = _operands(M, N)
    ref = torch.nn.functional.gelu(o["z"])
    if split_out:
        got = _planes_sum(_gemm(L, o, _nan_out(o, torch.bfloat16, 2 * N), hint, epilogue=L.EPI_GELU, ldo=2 * N, out_split=True), N)
    else:
        got = _gemm(L, o, _nan_out(o), hint, epilogue=L.EPI_GELU)
    _check("gelu %s %dx%d" % ("planes" if split_out else "fp32", M, N), hint, got, ref, 2e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("epi", ["store", "store_rope", "resid", "gate"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_8phase_sums_in_ring_order(L, M, N, epi):
    """tile_hint 5 at the ragged shapes: STORE (+ RoPE) / RESID / GATE_RESID of the 8-phase kernel equal REF bit for bit (same products, same
    order)."""
    o = _operands(M, N)
    t = _tables(M, N)
    if epi == "store":
        run, exact = (lambda h: _gemm(L, o, _nan_out(o), h, rows_per_batch=RPB[M])), o["z"]
    elif epi == "store_rope":
        tab, rope_cols, rkw = _rope_kw(M, N)
        run, exact = (lambda h: _gemm(L, o, _nan_out(o), h, **rkw)), _rope_ref(o["z"], tab, rope_cols, RPB[M], ROPE_OFF)
    elif epi == "resid":
        run, exact = (lambda h: _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_RESID, resid=o["res"], rows_per_batch=RPB[M])), o["res64"] + o["z"]
    else:
        run = lambda h: _gemm(L, o, _nan_out(o), h, resid=o["res"], **_gate_kw(L, t, M))
        exact = o["res64"] + _gate_rows(t["gate"], STEP, M, RPB[M]).double() * o["z"]
    got = run(HINT_8PHASE)
    _check_f32("8-phase %s %dx%d" % (epi, M, N), HINT_8PHASE, got, exact, o)
    assert torch.equal(got, _ref(("8-phase", epi, M, N), run))


# ------------------------------------------------------------------------------------------------------------- 4. refusals
def _refused(L, o, out, match, hint, **kw):
    """The call raises before any launch: the NaN-prefilled output is untouched."""
    with pytest.raises(L.V2AError, match=match):
        _gemm(L, o, out, hint, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_refuses_tile_hint_8(L):
    o = _operands(28, 512)
    _refused(L, o, _nan_out(o), "tile_hint 8 with split operands", 8)


@pytest.mark.parametrize("hint", EPI_HINTS)
def test_refuses_bf16_store(L, hint):
    o = _operands(28, 512)
    _refused(L, o, _nan_out(o, torch.bfloat16), "unsupported epilogue", hint)


@pytest.mark.parametrize("hint", EPI_HINTS)
def test_refuses_fp32_geglu(L, hint):
    """GEGLU on split operands is built with the hi | lo plane output only."""
    o = _operands(28, 512)
    _refused(L, o, _nan_out(o, cols=256), "unsupported epilogue", hint, epilogue=L.EPI_GEGLU)


@pytest.mark.parametrize("hint", EPI_HINTS)
def test_refuses_split_output_of_resid(L, hint):
    o = _operands(28, 512)
    _refused(L, o, _nan_out(o, torch.bfloat16, 1024), "V2A_BF16_SPLIT goes with", hint, epilogue=L.EPI_RESID, resid=o["res"], ldo=1024, out_split=True)


@pytest.mark.parametrize("hint", [6, 7])
def test_refuses_offset_tables_on_32_wide_stages(L, hint):
    """a_row_offset / a_ktile_offset are laid out for 64-wide K tiles: the shapes that stage 32 k refuse them."""
    o = _operands(28, 512)
    t, ld, k = o["segs"][0]
    rows = (torch.arange(28, dtype=torch.int32) * ld).to(DEV)
    ktiles = (torch.arange(k // 64, dtype=torch.int32) * 64).to(DEV)
    _refused(L, o, _nan_out(o), "offset tables", hint, segs=[(t, ld, k, k)], a_row_offset=rows, a_ktile_offset=ktiles)


# ------------------------------------------------------------------------------------------------------------- 5. the shipped calls in miniature
# one clip shortened to 2 x 150 rows, the shipped widths (1024, 1280, 512) divided by 4
MINI_M, MINI_RPB, D_A, D_T, D_F = 300, 150, 256, 320, 128


def _mini_producer_kw(o, seed):
    """norm_gamma [step][batch element][slot] with a switch row inside the first tile, as the adaptive norms launch it."""
    N = o["N"]
    gam = 1.0 + 0.3 * torch.randn(NSTEPS, 2, 2, N, generator=torch.Generator().manual_seed(seed))
    gd = gam.to(DEV)
    kw = dict(norm_gamma=gd, norm_step_stride=gd.stride(0), norm_batch_stride=gd.stride(1), norm_switch_row=100, norm_switch_offset=gd.stride(2),
              step=torch.tensor([STEP], dtype=torch.int32, device=DEV), rows_per_batch=MINI_RPB)
    return kw, _gamma_rows(gam, STEP, MINI_M, MINI_RPB, 100)


def _mini_producer_check(L, what, hint, o, kw, grow, exact):
    N = o["N"]

    def run(h):
        sh, ssq = _shadow(o), torch.full((MINI_M, N // 32), SSQ_SENTINEL, device=DEV)
        return _gemm(L, o, _nan_out(o), h, out_bf16=sh, ld_out_bf16=2 * N, out_bf16_split=True, norm_ssq=ssq, **kw), sh, ssq

    out, sh, ssq = run(hint)
    _check_f32(what, hint, out, exact, o)
    _assert_shadow(sh, out.cpu() * grow)
    torch.testing.assert_close(ssq.cpu().double(), (out.cpu().double() ** 2).reshape(MINI_M, N // 32, 32).sum(-1), rtol=1e-5, atol=1e-6)
    for x, y in zip((out, sh, ssq), _ref((what,), run)):
        assert torch.equal(x, y)


def test_shipped_frames_stream_on_hint_6(L):
    """tile_hint 6 as TUNED_TILES ships it for the frames stream at one clip: cross (three segments, RESID), out (RESID + folded-norm
    producer), ff2 (RESID + split shadow)."""
    o = _operands(MINI_M, D_F, (D_A, D_T, D_F))
    run = lambda h: _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_RESID, resid=o["res"])
    got = run(6)
    _check_f32("shipped f.cross", 6, got, o["res64"] + o["z"], o)
    assert torch.equal(got, _ref(("f.cross",), run))

    o = _operands(MINI_M, D_F, (D_F,))
    kw, grow = _mini_producer_kw(o, 61)
    _mini_producer_check(L, "shipped f.out", 6, o, dict(epilogue=L.EPI_RESID, resid=o["res"], **kw), grow, o["res64"] + o["z"])

    o = _operands(MINI_M, D_F, (4 * D_F,))

    def ff2(h):
        sh = _shadow(o)
        return _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_RESID, resid=o["res"], out_bf16=sh, ld_out_bf16=2 * D_F, out_bf16_split=True), sh

    out, sh = ff2(6)
    _check_f32("shipped f.ff2", 6, out, o["res64"] + o["z"], o)
    _assert_shadow(sh, out)
    for x, y in zip((out, sh), _ref(("f.ff2",), ff2)):
        assert torch.equal(x, y)


def test_shipped_audio_stream_by_shape(L):
    """tile_hint 0 as the audio stream's narrow GEMMs run at one clip: skip (two segments, STORE), out2 (GATE_RESID + folded-norm producer),
    q2 (STORE + RoPE over the heads + row_ssq consumer; 16 gate columns behind the heads)."""
    o = _operands(MINI_M, D_A, (D_A, D_A))
    run = lambda h: _gemm(L, o, _nan_out(o), h)
    got = run(0)
    _check_f32("shipped a.skip", 0, got, o["z"], o)
    assert torch.equal(got, _ref(("a.skip",), run))

    o = _operands(MINI_M, D_A, (D_A,))
    kw, grow = _mini_producer_kw(o, 62)
    gate = torch.rand(NSTEPS, 2, D_A, generator=torch.Generator().manual_seed(63))
    gd = gate.to(DEV)
    kw.update(epilogue=L.EPI_GATE_RESID, resid=o["res"], gate=gd, gate_step_stride=gd.stride(0), gate_batch_stride=gd.stride(1))
    _mini_producer_check(L, "shipped a.out2", 0, o, kw, grow, o["res64"] + _gate_rows(gate, STEP, MINI_M, MINI_RPB).double() * o["z"])

    N = D_A + 16
    o = _operands(MINI_M, N, (D_A,))
    ssq, rstd = _row_ssq(MINI_M)
    tab = _rope_table(MINI_RPB)
    run = lambda h: _gemm(L, o, _nan_out(o), h, rope_table=tab.to(DEV), rope_cols=D_A, rope_pos_offset=0, rows_per_batch=MINI_RPB, row_ssq=ssq,
                          row_norm_dim=NORM_DIM)
    got = run(0)
    ref = _rope_ref(o["acc"] * rstd[:, None] + o["bias"].cpu().double(), tab, D_A, MINI_RPB, 0)
    _check("shipped a.q2", 0, got, ref, 5e-5 * float(ref.abs().max()))
    assert torch.equal(got, _ref(("a.q2",), run))
