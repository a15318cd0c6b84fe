"""GPU: the plain bf16 x bf16 ring GEMM (csrc/gemm.hip, gemm_bf16_dma_kernel) on the tile hints no other test launches, against float64.

v2a_gemm_args.tile_hint picks the instantiation; the ones under test:

  hint  tile, waves, ring            wave tile  note
  6     256x256, 2x4, 2-deep         128x64     no epilogue operand is prefetched: every epilogue is the pipelined form
  10/11 64x64,   2x2, 4- / 5-deep    32x32
  12    128x128, 2x2, 4-deep         64x64
  13    128x128, 2x4, 3-deep         64x32      shipped: the narrow GEMMs of the text and frames streams (dit.py, TUNED_TILES tile 12)
  14    64x64,   2x4, 3-deep         32x16      GEGLU is not built; norm_ssq is refused (a row of a slab has 4 lanes, the sums need 8)
  15    128x64,  4x2, 3-deep         32x32      shipped: the audio stream's narrow GEMMs (TUNED_TILES tile 14)
  16    64x128,  2x4, 3-deep         32x32

They differ in the DMA group -> wave map, the ring depth and its wait chain, the wave tile (the lane -> (row, 4 columns) map of
gemm_epilogue_lds_impl) and in whether epilogue operands are prefetched.  tile_hint 1 (128x256) joins where its STORE / GATE_RESID epilogues
take the pipelined form on plain operands (RoPE positions and per-batch gates that wrap), which is otherwise run on split operands only.

Operands are bf16 tensors from seeded CPU generators, a ~ N(0, 1), w ~ N(0, 1) / sqrt(K); references are float64 products of the bf16-rounded
operands; outputs are prefilled with NaN (shadows and sums with a sentinel), so that an element nobody wrote fails.  Bars:
  fp32 outputs   atol 5e-4, rtol 1e-4 against float64 (test_gemm_deep_ring_k_tails' bar at the same operand scaling), and torch.equal with
                 tile_hint 4 for STORE / RESID / GATE_RESID: the K order of an output element does not depend on the tile
  GEGLU fp32     |err| <= 5e-4 (1 + |value| + |gate|) + 1e-4 |ref|: the fp32 bar pushed through v * gelu(g), whose partial derivatives are
                 bounded by |g| and 1.13 |v|; no bit equality (the store forms lower exp differently)
  bf16 outputs   |err| <= 2^-8 |ref| + 1e-3: one bf16 rounding is 2^-9 relative, doubled because the fp32 error can move a value across a
                 rounding boundary
  folded norm    producer: fp32 output equal to the unfolded call, shadow equal to bf16(out * gamma row), sums rtol 1e-5 / atol 1e-6 against
                 float64 of the stored output; consumer: the bars of test_gemm_folded_norm_consumer
Shapes: (273, 272) a second 256-row band of 17 rows and a 16-column last tile, (28, 512) one partial slab, (333, 416) full and partial wave
tiles in one launch; K = 64 .. 448 gives 1 .. 7 K tiles: fewer than, as many as and every residue modulo the ring depths 2 .. 5.

Every case prints its largest error ("ring-hints <what> hint=<h> ... err=<e>") before it asserts."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEW_HINTS = [6, 10, 11, 12, 13, 14, 15, 16]
PIPELINED_PLAIN = [1]            # 128x256: STORE and GATE_RESID are the pipelined, non-prefetched form
REF_HINT = 4                     # 64x64, 2x2 waves, 3-deep ring
NO_GEGLU = 14
SHAPES = [(273, 272), (28, 512), (333, 416)]
RPB = {273: 150, 28: 23, 333: 150}      # a batch element ends inside the launch
K_EPI = 128
STEP, NSTEPS = 3, 5
F32_BAR = dict(atol=5e-4, rtol=1e-4)
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


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


_OPS, _REF4 = {}, {}


def _operands(M, N, ks=(K_EPI,), ldas=None):
    """Operands of one (M, N, K segments) and their float64 product, made once and shared by the cases of that shape (never modified).
    ldas: row strides of the segments (a segment is then a view into a wider buffer of ones)."""
    key = (M, N, tuple(ks), tuple(ldas or ()))
    if key not in _OPS:
        K = sum(ks)
        g = torch.Generator().manual_seed(1000 * M + N + 7 * K + len(ks))
        a = [torch.randn(M, k, generator=g).bfloat16() for k in ks]
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
        bias = 0.1 * torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g)
        segs = []
        for i, (t, k) in enumerate(zip(a, ks)):
            ld = ldas[i] if ldas else k
            buf = torch.ones(M, ld, dtype=torch.bfloat16)
            buf[:, :k] = t
            segs.append((buf.to(DEV), ld, k))
        acc = torch.cat([t.double() for t in a], 1) @ w.double().t()
        _OPS[key] = dict(M=M, N=N, segs=segs, w=w.to(DEV), bias=bias.to(DEV), res=res.to(DEV), acc=acc, z=acc + bias.double(), res64=res.double())
    return _OPS[key]


def _gemm(L, o, out, hint, **kw):
    L.gemm(o["segs"], o["w"], out, M=o["M"], N=o["N"], compute=L.BF16, bias=o["bias"], tile_hint=hint, **kw)
    return out


def _nan_out(o, dtype=torch.float32, cols=None):
    return torch.full((o["M"], cols or o["N"]), NAN, dtype=dtype, device=DEV)


def _ref4(key, launch):
    """The same call on tile_hint 4, launched once per case key and shared."""
    if key not in _REF4:
        _REF4[key] = launch(REF_HINT)
    return _REF4[key]


def _check_f32(what, hint, got, ref):
    got = got.cpu().double()
    err = float((got - ref).abs().max())
    print("ring-hints %s hint=%d fp32 err=%.3g" % (what, hint, err))
    torch.testing.assert_close(got, ref, **F32_BAR)


def _check_bf16(what, hint, got, ref):
    got = got.float().cpu().double()
    bad = (got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-3)
    print("ring-hints %s hint=%d bf16 err=%.3g over-bar=%.3g" % (what, hint, float((got - ref).abs().max()), float(bad.max())))
    assert not torch.isnan(got).any()
    assert float(bad.max()) <= 0, float(bad.max())


# ------------------------------------------------------------------------------------------------------------- 1. the K loop
_KT = {}


def _k_tail_case(L, K):
    if K not in _KT:
        M, N = 333, 456
        o = _operands(M, N, (K,) if K < 192 else (64, K - 128, 64))
        g = torch.Generator().manual_seed(K)
        gate = torch.randn(1, N, generator=g)
        kw = dict(epilogue=L.EPI_GATE_RESID, resid=o["res"], gate=gate.to(DEV), gate_step_stride=0, gate_batch_stride=0, rows_per_batch=M)
        ref4 = _gemm(L, o, _nan_out(o), REF_HINT, **kw)
        _KT[K] = (o, kw, ref4, o["res64"] + gate.double() * o["z"])
    return _KT[K]


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 448])
@pytest.mark.parametrize("hint", NEW_HINTS)
def test_k_loop_ring_tails(L, hint, K):
    """1 .. 7 K tiles on ring depths 2 .. 5 (fewer tiles than the prologue issues, exactly as many, every residue of the unrolled ring), three A
    segments from K = 192 on, ragged M and N, GATE_RESID with a bias: bit for bit what tile_hint 4 gives, and float64 parity."""
    o, kw, ref4, exact = _k_tail_case(L, K)
    got = _gemm(L, o, _nan_out(o), hint, **kw)
    _check_f32("k-tail K=%d" % K, hint, got, exact)
    assert torch.equal(got, ref4)


# ------------------------------------------------------------------------------------------------------------- 2. epilogues at the tile edges
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", NEW_HINTS)
def test_store(L, hint, M, N, odt):
    o = _operands(M, N)
    run = lambda h: _gemm(L, o, _nan_out(o, odt), h, rows_per_batch=RPB[M])
    got = run(hint)
    if odt == torch.float32:
        _check_f32("store %dx%d" % (M, N), hint, got, o["z"])
        assert torch.equal(got, _ref4(("store", M, N), run))
    else:
        _check_bf16("store %dx%d" % (M, N), hint, got, o["z"])


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rpb", [23, 150])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", NEW_HINTS + PIPELINED_PLAIN)
def test_store_rope_positions_wrap(L, hint, M, N, rpb, odt):
    """STORE + RoPE over the first 128 columns at position offset 5: positions wrap inside a slab (23) and inside the first tile (150)."""
    rope_cols, off = 128, 5
    o = _operands(M, N)
    tab = _rope_table(off + rpb)
    got = _gemm(L, o, _nan_out(o, odt), hint, rope_table=tab.to(DEV), rope_cols=rope_cols, rope_pos_offset=off, rows_per_batch=rpb)
    ref = _rope_ref(o["z"], tab, rope_cols, rpb, off)
    (_check_f32 if odt == torch.float32 else _check_bf16)("rope %dx%d rpb=%d" % (M, N, rpb), hint, got, ref)


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N", [(28, 512), (333, 416)])
@pytest.mark.parametrize("hint", NEW_HINTS)
def test_geglu(L, hint, M, N, odt):
    """GEGLU on W rows packed [16 value | 16 gate]; tile_hint 14 (16-column wave tiles) has no GEGLU form: refused before any launch."""
    o = _operands(M, N)
    out = _nan_out(o, odt, N // 2)
    if hint == NO_GEGLU:
        with pytest.raises(L.V2AError, match="unsupported epilogue"):
            _gemm(L, o, out, hint, epilogue=L.EPI_GEGLU, ldo=N // 2, rows_per_batch=RPB[M])
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        return
    _gemm(L, o, out, hint, epilogue=L.EPI_GEGLU, ldo=N // 2, rows_per_batch=RPB[M])
    z = o["z"].reshape(M, N // 32, 2, 16)
    v, gt = z[:, :, 0].reshape(M, N // 2), z[:, :, 1].reshape(M, N // 2)
    ref = v * torch.nn.functional.gelu(gt)
    if odt == torch.bfloat16:
        _check_bf16("geglu %dx%d" % (M, N), hint, out, ref)
        return
    got = out.cpu().double()
    bad = (got - ref).abs() - (5e-4 * (1 + v.abs() + gt.abs()) + 1e-4 * ref.abs())
    print("ring-hints geglu %dx%d hint=%d fp32 err=%.3g over-bar=%.3g" % (M, N, hint, float((got - ref).abs().max()), float(bad.max())))
    assert not torch.isnan(got).any()
    assert float(bad.max()) <= 0, float(bad.max())


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", NEW_HINTS)
def test_resid(L, hint, M, N):
    o = _operands(M, N)
    run = lambda h: _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_RESID, resid=o["res"], rows_per_batch=RPB[M])
    got = run(hint)
    _check_f32("resid %dx%d" % (M, N), hint, got, o["res64"] + o["z"])
    assert torch.equal(got, _ref4(("resid", M, N), run))


_GATES = {}


def _gate(N, rows):
    if (N, rows) not in _GATES:
        _GATES[(N, rows)] = torch.rand(rows, N, generator=torch.Generator().manual_seed(17 * N + rows))
    return _GATES[(N, rows)]


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", NEW_HINTS)
def test_gate_resid_at_device_step(L, hint, M, N):
    """GATE_RESID with the gate row taken at a non-zero device step counter."""
    o = _operands(M, N)
    gate = _gate(N, NSTEPS)
    gd, step = gate.to(DEV), torch.tensor([STEP], dtype=torch.int32, device=DEV)
    run = lambda h: _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_GATE_RESID, resid=o["res"], gate=gd, step=step, gate_step_stride=N,
                          rows_per_batch=RPB[M])
    got = run(hint)
    _check_f32("gate-step %dx%d" % (M, N), hint, got, o["res64"] + gate[STEP].double() * o["z"])
    assert torch.equal(got, _ref4(("gate-step", M, N), run))


@pytest.mark.parametrize("rpb", [23, 150])
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("hint", NEW_HINTS + PIPELINED_PLAIN)
def test_gate_resid_per_batch(L, hint, M, N, rpb):
    """GATE_RESID with one gate row per batch element: many (23) and two (150) elements under a tile."""
    o = _operands(M, N)
    B = (M + rpb - 1) // rpb
    gate = _gate(N, B)
    gd = gate.to(DEV)
    run = lambda h: _gemm(L, o, _nan_out(o), h, epilogue=L.EPI_GATE_RESID, resid=o["res"], gate=gd, gate_batch_stride=N, rows_per_batch=rpb)
    got = run(hint)
    _check_f32("gate-batch %dx%d rpb=%d" % (M, N, rpb), hint, got, o["res64"] + gate[torch.arange(M) // rpb].double() * o["z"])
    assert torch.equal(got, _ref4(("gate-batch", M, N, rpb), run))


# ------------------------------------------------------------------------------------------------------------- 3. folded RMSNorm
SHADOW_SENTINEL, SSQ_SENTINEL = -3.0, -1.0
PRODUCER_HINTS = [6, 10, 11, 12, 13, 15, 16]        # 14 cannot form the sums: test_hint14_* below


def _producer_case(L, epi, rpb_gamma=0):
    """test_gemm_folded_norm_producer's setup: step-indexed gamma (rpb_gamma = 0) or one gamma row per batch element of rpb_gamma rows, a switch
    row from which the second gamma vector applies.  Returns the operands, the call's keywords and the gamma of every row."""
    M, N, K = 333, 416, 192
    o = _operands(M, N, (K,))
    g = torch.Generator().manual_seed(len(epi) + rpb_gamma)
    if rpb_gamma:
        sw = 141
        gam = 1.0 + 0.3 * torch.randn((M + rpb_gamma - 1) // rpb_gamma, 2, N, generator=g)
        gd = gam.to(DEV)
        kw = dict(norm_gamma=gd[0, 0], norm_batch_stride=gd.stride(0), rows_per_batch=rpb_gamma)
        pair = gam[torch.arange(M) // rpb_gamma]                             # (M, 2, N)
    else:
        sw = 222
        gam = 1.0 + 0.3 * torch.randn(3, 2, N, generator=g)                   # [step][slot][N]
        gd = gam.to(DEV)
        kw = dict(norm_gamma=gd[0, 0], norm_step_stride=gd.stride(0), step=torch.tensor([2], dtype=torch.int32, device=DEV), rows_per_batch=111)
        pair = gam[2][None].expand(M, 2, N)
    kw.update(resid=o["res"], norm_switch_row=sw, norm_switch_offset=N)
    grow = torch.where((torch.arange(M) >= sw)[:, None], pair[:, 1], pair[:, 0]).to(DEV)
    if epi == "gate_resid":
        gate = torch.rand(3, N, generator=g).to(DEV)
        kw.update(epilogue=L.EPI_GATE_RESID, gate=gate, gate_step_stride=N if not rpb_gamma else 0)
    else:
        kw.update(epilogue=L.EPI_RESID)
    return o, kw, grow


def _producer_check(L, hint, epi, rpb_gamma, with_ssq=True):
    o, kw, grow = _producer_case(L, epi, rpb_gamma)
    M, N = o["M"], o["N"]
    sh = torch.full((M, N), SHADOW_SENTINEL, dtype=torch.bfloat16, device=DEV)
    ssq = torch.full((M, N // 32), SSQ_SENTINEL, device=DEV)
    out = _gemm(L, o, _nan_out(o), hint, out_bf16=sh, **(dict(norm_ssq=ssq) if with_ssq else {}), **kw)
    plain = _gemm(L, o, _nan_out(o), hint, **{k: v for k, v in kw.items() if not k.startswith("norm_")})
    assert not bool(torch.isnan(plain).any())
    assert torch.equal(out, plain)                                          # the fp32 result is untouched by the fold
    assert torch.equal(sh, (out * grow).bfloat16())
    if not with_ssq:
        assert bool((ssq == SSQ_SENTINEL).all())
        return
    ref = (out.cpu().double() ** 2).reshape(M, N // 32, 32).sum(-1)
    rel = float(((ssq.cpu().double() - ref).abs() / ref).max())
    print("ring-hints producer %s rpb=%d hint=%d ssq rel err=%.3g" % (epi, rpb_gamma, hint, rel))
    torch.testing.assert_close(ssq.cpu().double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("epi", ["resid", "gate_resid"])
@pytest.mark.parametrize("hint", PRODUCER_HINTS)
def test_folded_norm_producer(L, hint, epi):
    _producer_check(L, hint, epi, 0)


@pytest.mark.parametrize("rpb", [23, 150])
@pytest.mark.parametrize("epi", ["resid", "gate_resid"])
@pytest.mark.parametrize("hint", PRODUCER_HINTS)
def test_folded_norm_producer_per_batch_gamma(L, hint, epi, rpb):
    _producer_check(L, hint, epi, rpb)


@pytest.mark.parametrize("epi", ["resid", "gate_resid"])
def test_hint14_refuses_norm_ssq(L, epi):
    """16-column wave tiles: a row of a slab has 4 lanes, the sum of 32 columns is a butterfly over 8 -- the sums would mix two rows, and two waves
    would write one entry.  The host refuses the combination before any launch; nothing is written."""
    o, kw, _ = _producer_case(L, epi)
    M, N = o["M"], o["N"]
    out = _nan_out(o)
    sh = torch.full((M, N), SHADOW_SENTINEL, dtype=torch.bfloat16, device=DEV)
    ssq = torch.full((M, N // 32), SSQ_SENTINEL, device=DEV)
    with pytest.raises(L.V2AError, match="32x16.*at least 32 columns"):
        _gemm(L, o, out, 14, out_bf16=sh, norm_ssq=ssq, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((sh == SHADOW_SENTINEL).all()) and bool((ssq == SSQ_SENTINEL).all())


@pytest.mark.parametrize("rpb", [0, 23, 150])
@pytest.mark.parametrize("epi", ["resid", "gate_resid"])
def test_hint14_gamma_shadow_without_sums(L, epi, rpb):
    """norm_gamma alone (the shadow carries gamma, no sums are asked for) still runs on 16-column wave tiles."""
    _producer_check(L, 14, epi, rpb, with_ssq=False)


@pytest.mark.parametrize("epi", ["store_bf16", "store_f32", "geglu", "store_rope"])
@pytest.mark.parametrize("hint", [6, 13, 15, 16])
def test_folded_norm_consumer(L, hint, epi):
    """row_ssq: accumulator row m is scaled by sqrt(d) / max(sqrt(sum of its partial sums), 1e-12) before bias / GELU / RoPE
    (test_gemm_folded_norm_consumer's setup and bars; the rotation reference is the float64 _rope_ref on the same table)."""
    M, N, K, d = 300, 512, 256, 192                                         # 6 partial sums: the row is padded to 8 with zeros
    g = torch.Generator().manual_seed(hint + 31 * len(epi))
    a = torch.randn(M, K, generator=g).bfloat16()
    a[5] = 0                                                                # an all-zero row: eps clamp, 0 * huge = 0, no NaN
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    bias = 0.1 * torch.randn(N, generator=g)
    ssq = torch.zeros(M, 8)
    ssq[:, :d // 32] = torch.rand(M, d // 32, generator=g) * 40 + 1
    ssq[5] = 0.0
    rstd = math.sqrt(d) / ssq.double().sum(-1).sqrt().clamp_min(1e-12)
    z = (a.double() @ w.double().t()) * rstd[:, None] + bias.double()
    z[5] = bias.double()                                                    # 0 * (sqrt(d) / 1e-12) = 0
    kw = dict(M=M, N=N, compute=L.BF16, bias=bias.to(DEV), tile_hint=hint, row_ssq=ssq.to(DEV), row_norm_dim=d)
    segs = [(a.to(DEV), K, K)]
    if epi == "geglu":
        out = torch.full((M, N // 2), NAN, dtype=torch.bfloat16, device=DEV)
        L.gemm(segs, w.to(DEV), out, epilogue=L.EPI_GEGLU, ldo=N // 2, **kw)
        zz = z.reshape(M, N // 32, 2, 16)
        ref = (zz[:, :, 0] * torch.nn.functional.gelu(zz[:, :, 1])).reshape(M, N // 2)
        tol = dict(rtol=2e-2, atol=2e-2)
    elif epi == "store_rope":
        out = torch.full((M, N), NAN, dtype=torch.bfloat16, device=DEV)
        tab = _rope_table(M)
        L.gemm(segs, w.to(DEV), out, rope_table=tab.to(DEV), rope_cols=128, rope_pos_offset=0, rows_per_batch=M, **kw)
        ref = _rope_ref(z, tab, 128, M, 0)
        tol = dict(rtol=2e-2, atol=3e-2)
    else:
        out = torch.full((M, N), NAN, dtype=torch.bfloat16 if epi == "store_bf16" else torch.float32, device=DEV)
        L.gemm(segs, w.to(DEV), out, **kw)
        ref = z
        tol = dict(rtol=1e-2, atol=2e-2) if epi == "store_bf16" else dict(rtol=1e-4, atol=5e-4)
    got = out.float().cpu().double()
    print("ring-hints consumer %s hint=%d err=%.3g" % (epi, hint, float((got - ref).abs().max())))
    torch.testing.assert_close(got, ref, **tol)


# ---- the shipped calls in miniature: how dit.py launches tiles 14 and 12 (tile_hint 15 and 13) at one clip
def _shadowed_resid(L, hint, M, N, ks, ldas):
    """RESID over K segments of different row strides with a plain bf16 shadow inside a wider buffer (the next GEMM's operand)."""
    o = _operands(M, N, ks, ldas)
    ld2 = 2 * N
    sh = torch.full((M, ld2), SHADOW_SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = _gemm(L, o, _nan_out(o), hint, epilogue=L.EPI_RESID, resid=o["res"], out_bf16=sh, ld_out_bf16=ld2)
    _check_f32("shipped resid %dx%d segs=%d" % (M, N, len(ks)), hint, out, o["res64"] + o["z"])
    assert torch.equal(sh[:, :N], out.bfloat16())
    assert bool((sh[:, N:] == SHADOW_SENTINEL).all())                       # the rest of the wide rows stays untouched


def test_shipped_audio_tile_three_segments_then_store(L):
    """tile_hint 15 as the audio stream runs it: the cross-condition GEMM over [x | text | frames] segments with the residual and the bf16 shadow,
    then the skip projection over two segments with a plain store."""
    M, N = 333, 128
    _shadowed_resid(L, 15, M, N, (128, 192, 64), (256, 192, 64))
    o = _operands(M, N, (128, 192), (256, 192))
    _check_f32("shipped store %dx%d segs=2" % (M, N), 15, _gemm(L, o, _nan_out(o), 15), o["z"])


@pytest.mark.parametrize("N", [128, 320])
def test_shipped_side_tile_two_segments(L, N):
    """tile_hint 13 as the text / frames streams run it: the cross-condition GEMM over [x | own stream] with the residual."""
    _shadowed_resid(L, 13, 333, N, (128, 192), (256, 192))
