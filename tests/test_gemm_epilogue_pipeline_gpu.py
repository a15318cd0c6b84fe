"""GPU: the LDS-staged vector epilogue with its operands off the store chain (csrc/gemm_common.h, gemm_epilogue_lds) -- slab-invariant operands
(bias pieces, the device step counter, gate / gamma pieces of one or two batch elements) loaded once ahead of the slab loop, row operands (cos/sin
rows, residual rows) requested one slab ahead, row positions from one division per wave -- on the 256x256 8-phase kernel (tile_hint 5, split
operands) and, for the residual epilogues, on the 128x256 ring tile (tile_hint 6), the ring instantiation that takes the same path.

Logical K = 64 throughout (two stages: the shortest K loop the host admits), so a case is a few launches of a few microseconds.  Shapes are the
smallest at which the pipeline can go wrong:
  M = 28           one partial slab, every later slab (and the whole second wave row) behind the last row
  M = 273          the second 256-row band holds 17 rows: a full slab, a one-row slab, then skipped slabs
  M = 300, N = 272 a 16-column last tile (three of its four wave columns hold no column at all); full and partial wave tiles in one launch
  rows_per_batch   23 (shorter than a wave tile: several wraps per wave, positions wrap inside a slab), 150 (one wrap inside the first tile, in
                   the second wave row: waves with one and with two batch elements), 782 with M = 800 (the production length: a wrap inside
                   the fourth tile)
  GEGLU            N = 512 with dense rows (eight columns per lane, 16-byte stores) and with a row stride that is no multiple of 8 (four columns
                   per lane).  The host admits GEGLU for N % 32 == 0 only, so N / 2 is always a multiple of 8: the row stride and
                   v2a_tuning.reserved[0] bit 7 are what select the four-column form.

Bars: those of tests/test_gemm_8phase_split_gpu.py -- 3e-5 (GEGLU: 4e-5) of the largest reference value against the fp64 product, and bit
equality (torch.equal) for shadow planes against _split_planes of the fp32 output the same launch wrote.  Sums of squares (32 fp32 squares per
entry, summed in a butterfly): 1e-5 relative against fp64 of the stored fp32 output (32 roundings of 2^-24 are 2e-6)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HINT_8PHASE = 5
HINT_RING_128x256 = 6
K = 64
STEP = 3                       # device step counter: a non-zero row of the step-indexed gate / gamma tables
NSTEPS = 5


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


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


_CACHE = {}


def _operands(M, N):
    """Operands and the fp64 product of one (M, N), computed once and shared by the cases of that shape (never modified)."""
    if (M, N) not in _CACHE:
        g = torch.Generator().manual_seed(1000 * M + N)
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = 0.1 * torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g)
        acc = a.double() @ w.double().t()
        _CACHE[(M, N)] = dict(segs=[(_split_planes(a).to(DEV), 2 * K, K)], wd=_split_planes(w).to(DEV), bias=bias, res=res, acc=acc,
                              w=w, a=a, scale=max(float(acc.abs().max()), 1.0))
    return _CACHE[(M, N)]


def _kw(L, M, N, hint):
    return dict(M=M, N=N, compute=L.BF16, a_split=True, tile_hint=hint)


SHAPES = [(28, 512), (273, 512), (300, 272)]


@pytest.mark.parametrize("M,N", SHAPES)
def test_store_bias(L, M, N):
    """STORE with a bias and no row operand: partial and skipped slabs, the 16-column last tile."""
    o = _operands(M, N)
    out = torch.full((M, N), float("nan"), device=DEV)
    L.gemm(o["segs"], o["wd"], out, bias=o["bias"].to(DEV), **_kw(L, M, N, HINT_8PHASE))
    err = float((out.cpu().double() - (o["acc"] + o["bias"].double())).abs().max())
    print("store M=%d N=%d: err %.3g (bar %.3g)" % (M, N, err, 3e-5 * o["scale"]))
    assert err < 3e-5 * o["scale"], err


@pytest.mark.parametrize("M,rpb", [(300, 23), (273, 23), (300, 150), (28, 23), (800, 782)])
def test_store_rope_positions_wrap(L, M, rpb):
    """STORE + RoPE over 128 of N = 272 columns (the rotated columns end inside the first tile, in its second wave column) at a non-zero
    position offset: positions wrap inside a slab (23), inside the first tile (150), inside the fourth tile (782)."""
    N, rope_cols, off = 272, 128, 5
    o = _operands(M, N)
    tab = _rope_table(off + rpb)
    out = torch.full((M, N), float("nan"), device=DEV)
    L.gemm(o["segs"], o["wd"], out, bias=o["bias"].to(DEV), rope_table=tab.to(DEV), rope_cols=rope_cols, rope_pos_offset=off,
           rows_per_batch=rpb, **_kw(L, M, N, HINT_8PHASE))
    ref = _rope_ref(o["acc"] + o["bias"].double(), tab, rope_cols, rpb, off)
    err = float((out.cpu().double() - ref).abs().max())
    print("store + rope M=%d rpb=%d: err %.3g (bar %.3g)" % (M, rpb, err, 3e-5 * o["scale"]))
    assert err < 3e-5 * o["scale"], err


@pytest.mark.parametrize("form", ["wide", "stride", "bit7"])
@pytest.mark.parametrize("M", [273, 28])
def test_geglu_split_bias_both_store_forms(L, M, form):
    """GEGLU with hi | lo output planes and a bias at N = 512: the eight-column form (dense rows), the four-column form through a row stride
    that is no multiple of 8, and through v2a_tuning.reserved[0] bit 7 -- that one against the eight-column result of the same operands.
    The two forms are not equal bit for bit, before this change or after it: the compiler lowers the __expf of gelu_fast_f to a bare v_exp_f32 in
    one form and to its range-reduced expansion in the other (gfx950 listing of <GEGLU, bf16, 1, SPLIT>: 256 v_exp_f32, 128 v_ldexp_f32).  Both are
    good to about an ulp, so erf differs by <= 2^-22 and the fp32 value by less than 2^-21 of |value| * |gate|; each plane pair then keeps its value
    to 2^-18 of it (the rounding of the lo plane, itself <= 2^-9 of the value).  Bar: 2 * 2^-18 + 2^-21 < 1e-5 of the largest reference value."""
    N = 512
    half = N // 2
    o = _operands(M, N)
    perm = torch.cat([torch.cat([torch.arange(j * 16, j * 16 + 16), half + torch.arange(j * 16, j * 16 + 16)]) for j in range(half // 16)])
    wp, bp = _split_planes(o["w"][perm]).to(DEV), o["bias"][perm].to(DEV)      # W rows regrouped [16 value | 16 gate]
    ldo = N + 4 if form == "stride" else N
    out = torch.zeros(M, ldo, dtype=torch.bfloat16, device=DEV)
    kw = dict(epilogue=L.EPI_GEGLU, bias=bp, ldo=ldo, out_split=True, **_kw(L, M, N, HINT_8PHASE))
    if form == "bit7":
        wide = torch.zeros(M, ldo, dtype=torch.bfloat16, device=DEV)
        L.gemm(o["segs"], wp, wide, **kw)
        L.set_tuning(reserved=128)
    try:
        L.gemm(o["segs"], wp, out, **kw)
        torch.cuda.synchronize()
    finally:
        L.set_tuning()
    z = o["acc"] + o["bias"].double()
    ref = z[:, :half] * torch.nn.functional.gelu(z[:, half:])
    got = out[:, :half].float().cpu().double() + out[:, half:N].float().cpu().double()
    err, bar = float((got - ref).abs().max()), 4e-5 * max(float(ref.abs().max()), 1.0)
    print("geglu %s M=%d: err %.3g (bar %.3g)" % (form, M, err, bar))
    assert err < bar, err
    if form == "stride":
        assert float(out[:, N:].abs().max()) == 0          # the padding of the rows stays untouched
    if form == "bit7":
        gotw = wide[:, :half].float().cpu().double() + wide[:, half:N].float().cpu().double()
        dev, bar2 = float((got - gotw).abs().max()), 1e-5 * max(float(ref.abs().max()), 1.0)
        print("geglu four-column against eight-column M=%d: %.3g (bar %.3g), %d of %d stored values differ" %
              (M, dev, bar2, int((out != wide).sum()), out.numel()))
        assert dev < bar2, dev


def test_skipped_bands_switch_bit9(L):
    """v2a_tuning.reserved[0] bit 9 (multiply the row bands behind the last row too) changes no stored value."""
    M, N = 28, 512
    o = _operands(M, N)
    a, b = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    L.gemm(o["segs"], o["wd"], a, bias=o["bias"].to(DEV), **_kw(L, M, N, HINT_8PHASE))
    L.set_tuning(reserved=512)
    try:
        L.gemm(o["segs"], o["wd"], b, bias=o["bias"].to(DEV), **_kw(L, M, N, HINT_8PHASE))
        torch.cuda.synchronize()
    finally:
        L.set_tuning()
    assert torch.equal(a, b)


@pytest.mark.parametrize("hint", [HINT_8PHASE, HINT_RING_128x256])
@pytest.mark.parametrize("M,N", SHAPES)
def test_resid_split_shadow(L, M, N, hint):
    """RESID with a split shadow: residual rows one slab ahead; the shadow is the planes of the fp32 output."""
    o = _operands(M, N)
    out = torch.full((M, N), float("nan"), device=DEV)
    sh = torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    L.gemm(o["segs"], o["wd"], out, epilogue=L.EPI_RESID, resid=o["res"].to(DEV), bias=o["bias"].to(DEV), out_bf16=sh, ld_out_bf16=2 * N,
           out_bf16_split=True, **_kw(L, M, N, hint))
    err = float((out.cpu().double() - (o["res"].double() + o["acc"] + o["bias"].double())).abs().max())
    print("resid hint %d M=%d N=%d: err %.3g (bar %.3g)" % (hint, M, N, err, 3e-5 * o["scale"]))
    assert err < 3e-5 * o["scale"], err
    assert torch.equal(sh.cpu(), _split_planes(out.cpu()))


def _batch_of(M, rpb):
    return torch.arange(M) // rpb


@pytest.mark.parametrize("hint", [HINT_8PHASE, HINT_RING_128x256])
@pytest.mark.parametrize("M,N,rpb", [(300, 512, 0), (300, 512, -23), (300, 512, 150), (273, 512, 23), (300, 272, 150), (28, 512, 23),
                                     (300, 512, 300)])
def test_gate_resid_at_device_step(L, M, N, rpb, hint):
    """GATE_RESID in place (resid == out, as the sampler runs it) with the gate row taken at a non-zero device step counter: shared over the
    batch (rpb = 0; -23 = shared, with rows_per_batch = 23 given all the same), and per batch element with one (300), two (150) and many (23)
    elements under a wave tile."""
    o = _operands(M, N)
    g = torch.Generator().manual_seed(7 * M + N + rpb)
    step = torch.tensor([STEP], dtype=torch.int32, device=DEV)
    if rpb <= 0:
        gate = torch.rand(NSTEPS, N, generator=g)
        grow = gate[STEP][None, :].expand(M, N)
        kw = dict(gate_step_stride=N, rows_per_batch=-rpb)
    else:
        B = (M + rpb - 1) // rpb
        gate = torch.rand(NSTEPS, B, N, generator=g)
        grow = gate[STEP][_batch_of(M, rpb)]
        kw = dict(gate_step_stride=B * N, gate_batch_stride=N, rows_per_batch=rpb)
    out = o["res"].clone().to(DEV)
    L.gemm(o["segs"], o["wd"], out, epilogue=L.EPI_GATE_RESID, resid=out, gate=gate.to(DEV), step=step, bias=o["bias"].to(DEV),
           **kw, **_kw(L, M, N, hint))
    ref = o["res"].double() + grow.double() * (o["acc"] + o["bias"].double())
    err = float((out.cpu().double() - ref).abs().max())
    print("gate hint %d M=%d N=%d rpb=%d: err %.3g (bar %.3g)" % (hint, M, N, rpb, err, 3e-5 * o["scale"]))
    assert err < 3e-5 * o["scale"], err


@pytest.mark.parametrize("hint", [HINT_8PHASE, HINT_RING_128x256])
@pytest.mark.parametrize("M,rpb,sw", [(300, 150, 141), (300, 23, 141), (273, 300, 261), (300, 0, 141)])
def test_gate_resid_folded_norm_producer(L, M, rpb, sw, hint):
    """GATE_RESID as a folded-norm producer: the split shadow carries gamma, per batch element (rpb > 0) or shared, with a switch row that falls
    inside a slab (141 = slab 8 of the first tile, row 13; 261 = the one full slab of the second band) -- rows from it on take the second gamma
    vector -- and the sums of squares per 32 columns."""
    N = 512
    o = _operands(M, N)
    g = torch.Generator().manual_seed(11 * M + rpb + sw)
    step = torch.tensor([STEP], dtype=torch.int32, device=DEV)
    B = (M + rpb - 1) // rpb if rpb else 1
    gate = torch.rand(NSTEPS, B, N, generator=g)
    gam = 1 + 0.2 * torch.randn(NSTEPS, B, 2 * N, generator=g)              # [gamma before the switch row | gamma from it on]
    b = _batch_of(M, rpb) if rpb else torch.zeros(M, dtype=torch.long)
    second = (torch.arange(M) >= sw)[:, None]
    gam_rows = torch.where(second, gam[STEP][b][:, N:], gam[STEP][b][:, :N])
    kw = dict(gate_step_stride=B * N, norm_step_stride=B * 2 * N, norm_switch_row=sw, norm_switch_offset=N)
    if rpb:
        kw.update(gate_batch_stride=N, norm_batch_stride=2 * N, rows_per_batch=rpb)
    out = o["res"].clone().to(DEV)
    sh = torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    ssq = torch.zeros(M, N // 32, device=DEV)
    L.gemm(o["segs"], o["wd"], out, epilogue=L.EPI_GATE_RESID, resid=out, gate=gate.to(DEV), step=step, bias=o["bias"].to(DEV),
           out_bf16=sh, ld_out_bf16=2 * N, out_bf16_split=True, norm_gamma=gam.to(DEV), norm_ssq=ssq, **kw, **_kw(L, M, N, hint))
    ref = o["res"].double() + gate[STEP][b].double() * (o["acc"] + o["bias"].double())
    err = float((out.cpu().double() - ref).abs().max())
    print("gate + norm hint %d M=%d rpb=%d: err %.3g (bar %.3g)" % (hint, M, rpb, err, 3e-5 * o["scale"]))
    assert err < 3e-5 * o["scale"], err
    assert torch.equal(sh.cpu(), _split_planes(out.cpu() * gam_rows))
    ssq_ref = (out.cpu().double() ** 2).reshape(M, N // 32, 32).sum(-1)
    assert float(((ssq.cpu().double() - ssq_ref).abs() / ssq_ref).max()) < 1e-5
