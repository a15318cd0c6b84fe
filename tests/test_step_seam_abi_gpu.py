"""GPU: the two launches that finish an armed bf16x3 sampler evaluation, called directly through the C ABI and held to float64 and to the bits
the header promises -- v2a_gemm_cfg_euler (csrc/gemm.hip, the one-launch step seam: gemm_bf16_dma_kernel<V2A_EPI_CFG_EULER, 64x64, 3-deep ring>
with the row map seam_row and the epilogue gemm_epilogue_cfg_euler) and v2a_cfg_euler_planes (csrc/rowops.hip, cfg_euler_planes_kernel).
tests/test_step_seam_gpu.py and tests/test_fold_embed_gpu.py compare them with the launches they replace, through the engine and at the engine's
buffer geometry; both sides of those comparisons share cfg_euler_axpy and the split ring.  Here every operand the header names is varied by itself.

Operands come from seeded CPU generators (as tests/test_gemm_split_ring_gpu.py): fp32 a ~ N(0, 1) with row m scaled by 1 + m / mh (a swapped or
clamped-into-range row cannot pass), w ~ N(0, 1) / sqrt(K), split by hi = bf16(x), lo = bf16(x - hi), W as [W_hi | W_lo]; bias = 0.1 randn,
y ~ randn, dt five distinct values in [0.05, 0.25].  `out` is prefilled with NaN; `planes`, the padding columns of `out` and a guard tail of 64
floats behind y with the sentinel -7.25: an element nobody wrote fails, and so does one somebody should not have written.

Bars, each taken from an existing test, none from what this file measured:
  out   bit for bit L.gemm(..., tile_hint=1) on the same operands        REF of test_gemm_split_ring_gpu.py; include/v2a_cfm.h promises it
        |out - float64 (a w^T [* row scale] + bias)| < 3e-5 max(max |acc|, 1)          test_gemm_split_native
        with row_ssq: < 5e-5 max |ref|                                                  test_gemm_split_native_folded_norm_consumer
  y     bit for bit L.cfg_euler (plain kernel, same dt / step / strength) on the seam's own stored out
        |y - float64 (y + h (pc + s (pc - pn)))| on that stored out <= tol_euler        test_rowops_gpu.py (imported, with _euler_ref)
        over three launches: the sum of the three tol_euler terms along the float64 sequence, which is evaluated on the fp32 predictions the
        three-launch sequence stored (the seam's last `out` must equal the last of them bit for bit; the earlier ones are overwritten)
  planes  frame rows of BOTH halves == L.split_planes(y_new) bit for bit; register rows, trailing rows, the columns between and behind the
        planes still the sentinel
  counters  arrive[0] == 0 and step[0] one higher after every launch
v2a_cfg_euler_planes: float64 and tol_euler for y (with APG: the reference formed from _apg_sums_ref, as test_cfg_euler does), y bit for bit
the plain kernel's, planes bit for bit L.split_planes(y_new), sentinels everywhere else -- the second half of the plane buffer when copies = 1.

Cases, (B, row_off, T, rows_per_seq), K = 128 and N = 64 unless said:
  1 row map and bands   (1,4,28,32) one full band, one workgroup; (1,4,5,9) mh = 9, most tile rows clamped loads; (1,4,41,45) a 13-row last
                        band; (3,4,15,23) mh = 69, sequence ends and register rows inside bands, four trailing rows per sequence; (2,0,32,32)
  2 columns and grid    N = 128, 192, 320 at (3,4,15,23); (8,4,103,107) N = 640 K = 64: 27 bands x 10 = 270 workgroups
  3 K loop              K = 64, 192, 256, 448 at (1,4,41,45)
  4 segments            two and three K segments, rows wider than 2k and the [x_hi | s_hi | x_lo | s_lo] layout (hi -> lo distance k0 + k1),
                        at (3,4,15,23) and (1,4,41,45): bit for bit the one-segment call
  5 epilogue operands   no bias; row_ssq at (1,4,41,45) and (3,4,15,23); ldo = N + 8; lo_offset = N + 8 with ld = lo_offset + N + 12;
                        cfg_strength 0, 2, -0.5
  6 step counter        from step = 2, three launches with no host sync between them and fresh a operands, at the 270-workgroup and the
                        one-workgroup shape: step == 5, arrive == 0, y against the float64 sequence and bit for bit the three-launch sequence
  7 graph replay        one captured launch replayed three times == three eager launches bit for bit (y, planes, out, step, arrive)
  8 refusals            20 argument errors that name v2a_gemm_cfg_euler and leave out, y, planes, step and arrive untouched
  9 cfg_euler_planes    8 cases: an orthogonal array over {copies 1 | 2, 3 trailing rows, plane row_off 6 != 4, lo_offset = C + 8 with
                        ld = lo_offset + C + 4} (every pair of the four), C in {4, 68, 260}, T in {1, 37}, B in {1, 3}, batch stride padded by 16
                        floats, device step 0 and 3, APG on (keep = 0.3) and off

Every case prints "step-seam <section> <case> <what> err=<e> bar=<b> (<e / b>)" before it asserts, and the module prints the largest ratio per
section and its case count and wall time when it is done (pytest -s); profiles/step_seam_parity.txt records them.

Largest errors measured on the MI355X, 66 cases in 0.5 s (1.3 s with collection and the library load); no bar was set from them.  out: error
of bar; y: largest |got - ref| / tol_euler, against 1:
  1 rows        out 5.2e-5 of 2.7e-4    y 0.25        6 sequence    out 8.3e-5 of 3.9e-4    y over three launches 0.18 of the summed bar
  2 columns     out 8.3e-5 of 3.9e-4    y 0.29        7 graph       bit for bit
  3 K loop      out 4.7e-5 of 2.7e-4    y 0.25        8 refusals    20 of 20 refused with nothing written; the unchanged call 5.1e-5 of 3.2e-4
  4 segments    out 5.0e-5 of 2.7e-4    y 0.25        9 planes      y 0.31 (C = 260, T = 37, B = 3, APG)
  5 epilogue    out 5.3e-5 of 2.8e-4    y 0.24        5 row_ssq     out 6.9e-5 of 6.1e-4    y 0.24
Every bit comparison held: out against v2a_gemm on tile_hint 1, y against v2a_cfg_euler on the stored out, planes against split_planes(y_new),
two and three K segments in both layouts against the one-segment call, the one launch against the three it replaces.  No kernel was changed."""
import math
import time

import pytest
import torch

from test_rowops_gpu import _apg_sums_ref, _euler_ref, tol_euler

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -7.25                     # exact in fp32 and in bf16
GUARD = 64                       # floats behind y
NDT = 5
NORM_DIM = 192                   # row_ssq: 6 partial sums, the row padded to 8 with zeros (as test_gemm_split_ring_gpu.py)
REF_HINT = 1                     # 64x64, 2x2 waves, 3-deep ring, 64-wide stages

ONE_BAND = (1, 4, 28, 32)
TINY = (1, 4, 5, 9)
TAIL13 = (1, 4, 41, 45)
RAGGED = (3, 4, 15, 23)
NO_REGS = (2, 0, 32, 32)
BIG = (8, 4, 103, 107)           # with N = 640: 27 bands x 10 column tiles = 270 workgroups
BIG_N, BIG_K = 640, 64
ROW_SHAPES = [ONE_BAND, TINY, TAIL13, RAGGED, NO_REGS]
SEAM_N = [128, 192, 320]
SEAM_K = [64, 192, 256, 448]
SEG_KS = [(64, 128), (128, 64), (64, 128, 64), (128, 64, 192)]
STRENGTHS = [0.0, 2.0, -0.5]


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------------------- float64 reference helpers
# (checked on the CPU by tests/test_step_seam_refs.py against Python loops, torch and the oracle's sampler)
def row_map(B, rps):
    """Row m of the 2 B rps rows of the seam's GEMM -> (half, b, r): half 0 conditional / 1 null, clip b, row r of the clip's sequence."""
    m = torch.arange(2 * B * rps)
    mh = B * rps
    return m // mh, (m % mh) // rps, m % rps


def updates_y(rps, row_off, T):
    """Which rows of a sequence update y (and have plane rows written): [row_off, row_off + T)."""
    r = torch.arange(rps)
    return (r >= row_off) & (r < row_off + T)


def pred_halves(out, B, rps, row_off, T):
    """(2 B rps, C) predictions -> pc, pn (B, T, C): the frame rows of the conditional and of the null half."""
    v = out.reshape(2, B, rps, out.shape[-1])[:, :, row_off:row_off + T]
    return v[0], v[1]


def plane_rows(B, T, rps, row_off, copies):
    """(copies, B, T) rows of the plane buffer that element (b, i, :) of y goes to: (k B + b) rps + row_off + i."""
    k, b, i = torch.arange(copies)[:, None, None], torch.arange(B)[None, :, None], torch.arange(T)[None, None, :]
    return (k * B + b) * rps + row_off + i


def split_planes(x):
    """fp32 (..., c) -> bf16 (..., 2c) = [hi | lo]."""
    hi = x.bfloat16()
    return torch.cat([hi, (x - hi.float()).bfloat16()], -1)


def expected_planes(y_new, rows, ld, lo, rps, row_off, copies):
    """The whole plane buffer (rows, ld) after a launch on a sentinel-filled buffer: hi | lo planes of y_new (B, T, C) at plane_rows, columns
    [0, C) and [lo, lo + C); the sentinel everywhere else."""
    B, T, C = y_new.shape
    want = torch.full((rows, ld), SENT, dtype=torch.bfloat16)
    pl = split_planes(y_new)
    idx = plane_rows(B, T, rps, row_off, copies).reshape(copies, -1)
    for k in range(copies):
        want[idx[k], :C] = pl.reshape(B * T, 2 * C)[:, :C]
        want[idx[k], lo:lo + C] = pl.reshape(B * T, 2 * C)[:, C:]
    return want


def sequence_ref(y0, preds, hs, s):
    """Float64 Euler sequence y_{k+1} = y_k + h_k (pc_k + s (pc_k - pn_k)) over preds = [(pc, pn), ...]; returns (y_end, the sum of the tol_euler
    terms along it)."""
    y, tol = y0.double(), 0.0
    for (pc, pn), h in zip(preds, hs):
        nxt, par = _euler_ref(y, pc, pn, h, s, None, 0.0)
        tol = tol + tol_euler(y, pc, pn, par, h, s)
        y = nxt
    return y, tol


def row_scale(ssq):
    """What a row_ssq consumer multiplies accumulator row m by: sqrt(d) / max(sqrt(sum of the row's partial sums), 1e-12)."""
    return math.sqrt(NORM_DIM) / ssq.double().sum(-1).sqrt().clamp_min(1e-12)


# ------------------------------------------------------------------------------------------------------------- cases, made once on the CPU
_CASES, _DEVS = {}, {}


def seam_case(shape, N=64, ks=(128,), nbuf=1):
    """The fp32 operands of one (B, row_off, T, rows_per_seq), N and K segments: nbuf A operands (row m scaled by 1 + m / mh), w, bias, y, dt,
    row_ssq partial sums and the float64 products.  Made once, never modified."""
    key = (shape, N, tuple(ks), nbuf)
    if key not in _CASES:
        B, row_off, T, rps = shape
        mh, K = B * rps, sum(ks)
        M = 2 * mh
        g = torch.Generator().manual_seed(100003 * B + 1009 * rps + 101 * T + 13 * row_off + 7 * N + K + len(ks))
        mag = (1.0 + torch.arange(M) / mh)[:, None]
        a = [[torch.randn(M, k, generator=g) * mag for k in ks] for _ in range(nbuf)]
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = 0.1 * torch.randn(N, generator=g)
        y = torch.randn(B, T, N, generator=g)
        dt = 0.05 + 0.2 * torch.rand(NDT, generator=g)
        assert len(set(dt.tolist())) == NDT and 0.05 <= float(dt.min()) and float(dt.max()) <= 0.25
        ssq = torch.zeros(M, 8)
        ssq[:, :NORM_DIM // 32] = torch.rand(M, NORM_DIM // 32, generator=g) * 40 + 1
        acc = [torch.cat(x, 1).double() @ w.double().t() for x in a]
        _CASES[key] = dict(key=key, B=B, row_off=row_off, T=T, rps=rps, mh=mh, M=M, N=N, K=K, ks=tuple(ks), a=a, w=w, bias=bias, y=y, dt=dt, ssq=ssq,
                           rstd=row_scale(ssq), acc=acc)
    return _CASES[key]


def _dev(c):
    if c["key"] not in _DEVS:
        _DEVS[c["key"]] = dict(segs=[[(split_planes(x).contiguous().to(DEV), 2 * k, k) for x, k in zip(buf, c["ks"])] for buf in c["a"]],
                               w=split_planes(c["w"]).contiguous().to(DEV), bias=c["bias"].to(DEV), dt=c["dt"].to(DEV), ssq=c["ssq"].to(DEV))
    return _DEVS[c["key"]]


def segment_layouts(c, buf=0):
    """The A operand of a two- or three-segment case in three layouts:
    strided -- standard segments in rows wider than 2k (strides 2k + 64, + 128, + 192), the padding filled with ones: hi -> lo distances k_i;
    wide    -- the first two as the halves of one [x_hi | s_hi | x_lo | s_lo] buffer (lo plane k0 + k1 further, not k), a third standard;
    cat     -- one standard segment of the concatenated operand."""
    ks, M = c["ks"], c["M"]
    planes = [split_planes(x) for x in c["a"][buf]]
    strided = []
    for i, (pl, k) in enumerate(zip(planes, ks)):
        ld = 2 * k + 64 * (i + 1)
        b = torch.ones(M, ld, dtype=torch.bfloat16)
        b[:, :2 * k] = pl
        strided.append((b.to(DEV), ld, k))
    k0, k1 = ks[0], ks[1]
    xs, ss = planes[0], planes[1]
    wide = torch.cat([xs[:, :k0], ss[:, :k1], xs[:, k0:], ss[:, k1:]], 1).contiguous().to(DEV)
    d2 = k0 + k1
    wide_segs = [(wide, 2 * d2, k0, d2), (wide[:, k0:], 2 * d2, k1, d2)]
    if len(ks) == 3:
        wide_segs.append((planes[2].contiguous().to(DEV), 2 * ks[2], ks[2]))
    K = sum(ks)
    cat = [(split_planes(torch.cat(c["a"][buf], 1)).contiguous().to(DEV), 2 * K, K)]
    return dict(strided=strided, wide=wide_segs, cat=cat)


# ------------------------------------------------------------------------------------------------------------- buffers and launches
class State:
    """The buffers one launch writes: out (M, ldo) NaN with sentinel padding columns, planes (M, ld) sentinel, y with a sentinel guard tail, the
    step and the arrival counter."""

    def __init__(self, c, step0=0, ldo=None, lo=None, ld=None):
        N = c["N"]
        self.ldo, self.lo = ldo or N, lo or N
        self.ld = ld or self.lo + N
        self.out = torch.full((c["M"], self.ldo), SENT, device=DEV)
        self.out[:, :N] = NAN
        self.planes = torch.full((c["M"], self.ld), SENT, dtype=torch.bfloat16, device=DEV)
        self.n = c["y"].numel()
        self.y = torch.full((self.n + GUARD,), SENT, device=DEV)
        self.y[:self.n] = c["y"].reshape(-1).to(DEV)
        self.step = torch.tensor([step0], dtype=torch.int32, device=DEV)
        self.arrive = torch.zeros(1, dtype=torch.int32, device=DEV)

    def tensors(self):
        return dict(out=self.out, y=self.y, planes=self.planes, step=self.step, arrive=self.arrive)

    def snapshot(self):
        return {k: v.clone() for k, v in self.tensors().items()}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _gemm_kw(L, c, st, bias=True, ssq=False):
    d = _dev(c)
    kw = dict(M=c["M"], N=c["N"], compute=L.BF16, a_split=True, ldo=st.ldo, bias=d["bias"] if bias else None)
    if ssq:
        kw.update(row_ssq=d["ssq"], row_norm_dim=NORM_DIM)
    return kw


def seam_launch(L, c, st, strength, buf=0, segs=None, bias=True, ssq=False, gemm_over=None, seam_over=None):
    """One v2a_gemm_cfg_euler launch on the state's buffers; gemm_over / seam_over replace single arguments (the refusals)."""
    d = _dev(c)
    kw = _gemm_kw(L, c, st, bias, ssq)
    kw.update(gemm_over or {})
    sk = dict(y=st.y, dt=d["dt"], step=st.step, arrive=st.arrive, planes=dict(out=st.planes, ld=st.ld, lo_offset=st.lo), B=c["B"], T=c["T"],
              row_off=c["row_off"], rows_per_seq=c["rps"], cfg_strength=strength)
    sk.update(seam_over or {})
    L.gemm_cfg_euler(segs if segs is not None else d["segs"][buf], d["w"], st.out, **sk, **kw)


def _dense_pred(c, out):
    return out if out.shape[1] == c["N"] else out[:, :c["N"]].contiguous()


def three_launches(L, c, st, strength, buf=0, bias=True, ssq=False):
    """What the seam replaces, on the state's buffers: v2a_gemm on the REF tile, v2a_cfg_euler_planes with copies = 2, v2a_step_advance."""
    d = _dev(c)
    L.gemm(d["segs"][buf], d["w"], st.out, tile_hint=REF_HINT, **_gemm_kw(L, c, st, bias, ssq))
    L.cfg_euler(st.y, _dense_pred(c, st.out), B=c["B"], T=c["T"], C_=c["N"], pred_batch_stride=c["rps"] * c["N"], row_off=c["row_off"],
                cfg_strength=strength, dt=d["dt"], step=st.step,
                planes=dict(out=st.planes, ld=st.ld, lo_offset=st.lo, row_off=c["row_off"], rows_per_seq=c["rps"], copies=2))
    L.step_advance(st.step)


# ------------------------------------------------------------------------------------------------------------- reporting
_WORST, _T0, _NCASES = {}, [None], [0]


def _report(section, case, what, err, bar):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    w = _WORST.get((section, what))
    if w is None or ratio > w[2]:
        _WORST[(section, what)] = (err, bar, ratio)
    print("step-seam %-12s %-52s %-10s err=%.3g bar=%.3g (%.2f)" % (section, case, what, err, bar, ratio))
    return ratio


def _report_tol(section, case, what, got, ref, tol):
    """Per-element tolerance: prints the largest |got - ref| / tol (as err against bar 1) and returns it."""
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    ratio = _report(section, case, what, float(((got.double() - ref).abs() / tol).max()), 1.0)
    assert bool(torch.isfinite(got).all()), (section, case, what)
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _summary():
    _T0[0] = time.time()
    yield
    print("\nstep-seam parity: largest error per section (err, bar, err / bar); y and y-seq: |got - ref| / tol_euler against 1")
    for (section, what), (err, bar, ratio) in sorted(_WORST.items()):
        print("  %-12s %-10s %.3g of %.3g (%.2f)" % (section, what, err, bar, ratio))
    print("  %d cases in %.1f s" % (_NCASES[0], time.time() - _T0[0]))


@pytest.fixture(autouse=True)
def _count():
    _NCASES[0] += 1
    yield


# ------------------------------------------------------------------------------------------------------------- the check of one launch
def check_launch(L, section, case, c, st, step0, strength, buf=0, bias=True, ssq=False):
    """Everything the header says about one launch on a fresh State: counters, out (bits of v2a_gemm, float64), y (bits of v2a_cfg_euler on the
    stored out, float64 on the stored out), planes and every sentinel."""
    torch.cuda.synchronize()
    B, T, N, rps, row_off, M = c["B"], c["T"], c["N"], c["rps"], c["row_off"], c["M"]
    d = _dev(c)
    # out
    o = st.out.cpu()
    got = o[:, :N]
    plain = torch.full_like(st.out, NAN)
    L.gemm(d["segs"][buf], d["w"], plain, tile_hint=REF_HINT, **_gemm_kw(L, c, st, bias, ssq))
    same = _same_bits(st.out[:, :N], plain[:, :N])
    acc = c["acc"][buf]
    z = acc * c["rstd"][:, None] if ssq else acc
    if bias:
        z = z + c["bias"].double()
    bar = 5e-5 * float(z.abs().max()) if ssq else 3e-5 * max(float(acc.abs().max()), 1.0)
    r_out = _report(section, case, "out", float((got.double() - z).abs().max()), bar)
    # y
    yf = st.y.cpu()
    y_new = yf[:st.n].reshape(B, T, N)
    pc, pn = pred_halves(got, B, rps, row_off, T)
    h = float(c["dt"][step0])
    ref, par = _euler_ref(c["y"], pc, pn, h, strength, None, 0.0)
    r_y = _report_tol(section, case, "y", y_new, ref, tol_euler(c["y"], pc, pn, par, h, strength))
    y2 = c["y"].to(DEV).clone()
    L.cfg_euler(y2, _dense_pred(c, st.out), B=B, T=T, C_=N, pred_batch_stride=rps * N, row_off=row_off, cfg_strength=strength, dt=d["dt"],
                step=torch.tensor([step0], dtype=torch.int32, device=DEV))
    same_y = _same_bits(y_new, y2.cpu())
    # planes
    want = expected_planes(y_new, M, st.ld, st.lo, rps, row_off, 2)
    pl = st.planes.cpu()
    # every figure is printed: now the assertions
    assert int(st.arrive.item()) == 0, "arrive is 0 again when the launch has ended"
    assert int(st.step.item()) == step0 + 1, "the step counter is one higher"
    assert bool((o[:, N:] == SENT).all()), "padding columns of out"
    assert not bool(torch.isnan(got).any()), "a row or column of out nobody wrote"
    assert bool((yf[st.n:] == SENT).all()), "the guard tail behind y"
    assert same, "out carries the bits of the v2a_gemm launch (tile_hint 1)"
    assert r_out < 1.0, (section, case, "out", r_out)
    assert r_y <= 1.0, (section, case, "y", r_y)
    assert same_y, "y is updated exactly as by v2a_cfg_euler on the stored out"
    assert not torch.equal(y_new, c["y"])
    live = updates_y(rps, row_off, T)
    v = pl.reshape(2, B, rps, st.ld)
    assert bool((v[:, :, ~live] == SENT).all()), "register rows and trailing rows of the planes"
    assert _same_bits(pl, want), "frame rows of both halves are split_planes(y_new); the columns between and behind the planes are untouched"
    return y_new


def _run_and_check(L, section, c, strength=2.0, step0=0, bias=True, ssq=False, note="", **geom):
    st = State(c, step0, **geom)
    seam_launch(L, c, st, strength, bias=bias, ssq=ssq)
    case = "%s N=%d K=%d s=%g step=%d%s" % (c["key"][0], c["N"], c["K"], strength, step0, note)
    return check_launch(L, section, case, c, st, step0, strength, bias=bias, ssq=ssq)


# ------------------------------------------------------------------------------------------------------------- 1. row map and bands
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=str)
def test_row_map_and_bands(L, shape):
    """One full band in one workgroup (the arriving workgroup is the last); mh = 9 < 32 (most tile rows are clamped loads); a 13-row last band;
    mh = 69 with sequence ends and register rows inside bands and four trailing rows per sequence, whose out rows are written and whose y and
    plane rows are not; no registers."""
    _run_and_check(L, "1 rows", seam_case(shape), step0=1)


# ------------------------------------------------------------------------------------------------------------- 2. columns and grid size
@pytest.mark.parametrize("N", SEAM_N)
def test_column_tiles(L, N):
    """2, 3 and 5 column tiles x 3 row bands through fill_tile_map."""
    _run_and_check(L, "2 columns", seam_case(RAGGED, N=N))


def test_more_workgroups_than_cus(L):
    """270 workgroups: the arrival counter across more than one wave of workgroups."""
    _run_and_check(L, "2 columns", seam_case(BIG, N=BIG_N, ks=(BIG_K,), nbuf=3), step0=3)


# ------------------------------------------------------------------------------------------------------------- 3. K loop
@pytest.mark.parametrize("K", SEAM_K)
def test_k_loop(L, K):
    """1, 3, 4 and 7 stages of 64: fewer than the ring issues ahead, exactly the ring, residues 1, 0, 1 modulo 3."""
    _run_and_check(L, "3 K loop", seam_case(TAIL13, ks=(K,)))


# ------------------------------------------------------------------------------------------------------------- 4. segments
@pytest.mark.parametrize("ks", SEG_KS, ids=str)
@pytest.mark.parametrize("shape", [RAGGED, TAIL13], ids=str)
def test_segments(L, shape, ks):
    """Two and three K segments with their own row strides and hi -> lo distances: everything the launch writes equals the one-segment call's
    bit for bit, which is checked in full."""
    c = seam_case(shape, ks=ks)
    lay = segment_layouts(c)
    ref = State(c)
    seam_launch(L, c, ref, 2.0, segs=lay["cat"])
    check_launch(L, "4 segments", "%s ks=%s cat" % (shape, ks), c, ref, 0, 2.0)
    for name in ("strided", "wide"):
        st = State(c)
        seam_launch(L, c, st, 2.0, segs=lay[name])
        torch.cuda.synchronize()
        for k, v in st.tensors().items():
            assert _same_bits(v, ref.tensors()[k]), (name, k)
        print("step-seam %-12s %-52s equal to the one-segment call bit for bit" % ("4 segments", "%s ks=%s %s" % (shape, ks, name)))


# ------------------------------------------------------------------------------------------------------------- 5. epilogue operands
def test_no_bias(L):
    _run_and_check(L, "5 epilogue", seam_case(RAGGED), bias=False, note=" no bias")


@pytest.mark.parametrize("shape", [TAIL13, RAGGED], ids=str)
def test_row_ssq(L, shape):
    """The folded final norm: a distinct scale per row, fetched through the seam's row map (rows of both halves, clamped rows in the last band)."""
    _run_and_check(L, "5 row_ssq", seam_case(shape), ssq=True, step0=4, note=" row_ssq")


def test_row_ssq_without_bias(L):
    _run_and_check(L, "5 row_ssq", seam_case(RAGGED), ssq=True, bias=False, note=" row_ssq no bias")


def test_padded_out_rows(L):
    c = seam_case(RAGGED)
    _run_and_check(L, "5 epilogue", c, ldo=c["N"] + 8, note=" ldo=N+8")


def test_wide_planes(L):
    c = seam_case(RAGGED)
    _run_and_check(L, "5 epilogue", c, lo=c["N"] + 8, ld=2 * c["N"] + 20, note=" lo=N+8 ld=lo+N+12")


def test_padded_out_rows_and_wide_planes_two_column_tiles(L):
    c = seam_case(RAGGED, N=128)
    _run_and_check(L, "5 epilogue", c, ssq=True, ldo=c["N"] + 8, lo=c["N"] + 8, ld=2 * c["N"] + 20, note=" ldo, lo, ld, row_ssq")


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("shape", [RAGGED, TINY], ids=str)
def test_cfg_strength(L, shape, strength):
    _run_and_check(L, "5 epilogue", seam_case(shape), strength=strength, step0=2)


# ------------------------------------------------------------------------------------------------------------- 6. the step counter over a sequence
@pytest.mark.parametrize("shape,N,K", [(BIG, BIG_N, BIG_K), (ONE_BAND, 64, 128)], ids=["270wg", "1wg"])
def test_three_launches_without_host_sync(L, shape, N, K):
    """From step = 2: three launches back to back, fresh a operands, the same out and planes.  step == 5, arrive == 0; y against the float64
    sequence over dt[2], dt[3], dt[4] and bit for bit the three-launch sequence."""
    c = seam_case(shape, N=N, ks=(K,), nbuf=3)
    B, T, rps, row_off, s = c["B"], c["T"], c["rps"], c["row_off"], 2.0
    _dev(c)                                                   # the three operands are on the device before the first launch
    torch.cuda.synchronize()
    st = State(c, 2)
    for k in range(3):
        seam_launch(L, c, st, s, buf=k)
    old = State(c, 2)
    outs = []
    for k in range(3):
        three_launches(L, c, old, s, buf=k)
        outs.append(old.out.clone())
    torch.cuda.synchronize()
    y_new = st.y.cpu()[:st.n].reshape(c["y"].shape)
    preds = [pred_halves(o.cpu(), B, rps, row_off, T) for o in outs]
    ref, tol = sequence_ref(c["y"], preds, [float(c["dt"][2 + k]) for k in range(3)], s)
    case = "%s N=%d K=%d steps 2..4" % (shape, N, K)
    r = _report_tol("6 sequence", case, "y-seq", y_new, ref, tol)
    # the stored predictions of the three-launch sequence, on which the float64 sequence stands, are what float64 says they are
    r_out = [_report("6 sequence", case + " launch %d" % k, "out", float((outs[k].cpu().double() - (c["acc"][k] + c["bias"].double())).abs().max()),
                     3e-5 * max(float(c["acc"][k].abs().max()), 1.0)) for k in range(3)]
    assert int(st.step.item()) == 5 and int(st.arrive.item()) == 0
    assert int(old.step.item()) == 5
    assert bool((st.y.cpu()[st.n:] == SENT).all())
    assert all(x < 1.0 for x in r_out), r_out
    assert r <= 1.0, r
    for name in ("y", "out", "planes", "step", "arrive"):
        assert _same_bits(st.tensors()[name], old.tensors()[name]), name
    assert _same_bits(st.planes.cpu(), expected_planes(y_new, c["M"], st.ld, st.lo, rps, row_off, 2))
    # one float64 step from the start separates the sequence from any single step: dt[2] alone is not within the bar
    one, _ = sequence_ref(c["y"], preds[:1], [float(c["dt"][2])], s)
    assert float(((one - ref).abs() / tol).max()) > 1.0


# ------------------------------------------------------------------------------------------------------------- 7. graph replay
def test_graph_replay_equals_eager(L):
    """The single launch captured on one stream (no parallel branches), replayed three times, against three eager launches."""
    c = seam_case(RAGGED, N=128)
    warm = State(c)
    seam_launch(L, c, warm, 2.0)                              # first-launch attribute calls must not happen under capture
    torch.cuda.synchronize()
    gs, es = State(c, 1), State(c, 1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        seam_launch(L, c, gs, 2.0)
    torch.cuda.synchronize()
    assert int(gs.step.item()) == 1 and bool(torch.isnan(gs.out[:, :c["N"]]).all()), "capture launches nothing"
    for _ in range(3):
        g.replay()
    for _ in range(3):
        seam_launch(L, c, es, 2.0)
    torch.cuda.synchronize()
    assert int(gs.step.item()) == 4 and int(gs.arrive.item()) == 0
    for name, v in gs.tensors().items():
        assert _same_bits(v, es.tensors()[name]), name
    assert not torch.equal(gs.y[:gs.n].cpu().reshape(c["y"].shape), c["y"])
    print("step-seam %-12s %-52s y, planes, out, step, arrive equal bit for bit" % ("7 graph", "%s N=128 three replays" % (RAGGED,)))


# ------------------------------------------------------------------------------------------------------------- 8. refusals
class _Null:
    def data_ptr(self):
        return 0


def _refusals():
    """name -> (c, st, L) -> dict(gemm_over=, seam_over=, segs=)."""
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)                                    # noqa: E731
    planes = lambda st, **kw: dict(planes=dict(dict(out=st.planes, ld=st.ld, lo_offset=st.lo), **kw))    # noqa: E731

    def offset_tables(c, st, L):
        t, ld, k = _dev(c)["segs"][0][0]
        return dict(segs=[(t, ld, k, k)], gemm_over=dict(a_row_offset=(torch.arange(c["M"], dtype=torch.int32) * ld).to(DEV),
                                                         a_ktile_offset=(torch.arange(k // 64, dtype=torch.int32) * 64).to(DEV)))

    def plain_bf16(c, st, L):
        t, ld, k = _dev(c)["segs"][0][0]
        return dict(segs=[(t, ld, k)], gemm_over=dict(a_split=False))

    return {
        "N=96": lambda c, st, L: dict(gemm_over=dict(N=96)),
        "M!=2*B*rps": lambda c, st, L: dict(gemm_over=dict(M=c["M"] - 2)),
        "B+1": lambda c, st, L: dict(seam_over=dict(B=c["B"] + 1)),
        "rps<row_off+T": lambda c, st, L: dict(seam_over=dict(T=c["rps"] - c["row_off"] + 1)),
        "lo_offset<N": lambda c, st, L: dict(seam_over=planes(st, lo_offset=c["N"] - 4)),
        "ld<lo_offset+N": lambda c, st, L: dict(seam_over=planes(st, ld=2 * c["N"] - 4)),
        "lo_offset%4": lambda c, st, L: dict(seam_over=planes(st, lo_offset=c["N"] + 2, ld=2 * c["N"] + 8)),
        "ld%4": lambda c, st, L: dict(seam_over=planes(st, ld=2 * c["N"] + 18)),
        "y+1float": lambda c, st, L: dict(seam_over=dict(y=st.y[1:])),
        "null step": lambda c, st, L: dict(seam_over=dict(step=_Null())),
        "null arrive": lambda c, st, L: dict(seam_over=dict(arrive=_Null())),
        "null planes": lambda c, st, L: dict(seam_over=planes(st, out=_Null())),
        "plain bf16": plain_bf16,
        "epilogue GELU": lambda c, st, L: dict(gemm_over=dict(epilogue=L.EPI_GELU)),
        "out_bf16": lambda c, st, L: dict(gemm_over=dict(out_bf16=torch.zeros(c["M"], c["N"], dtype=torch.bfloat16, device=DEV), ld_out_bf16=c["N"])),
        "rope_table": lambda c, st, L: dict(gemm_over=dict(rope_table=torch.zeros(c["rps"], 32, 2, device=DEV), rope_cols=64, rows_per_batch=c["rps"])),
        "relu": lambda c, st, L: dict(gemm_over=dict(relu=True)),
        "a offset tables": offset_tables,
        "out_row_offset": lambda c, st, L: dict(gemm_over=dict(out_row_offset=i32(c["M"]))),
        "ldo<N": lambda c, st, L: dict(gemm_over=dict(ldo=c["N"] - 4)),
    }


@pytest.mark.parametrize("name", list(_refusals()))
def test_refusals(L, name):
    """The argument error names v2a_gemm_cfg_euler; out, y, planes, step and arrive are as they were."""
    c = seam_case(RAGGED, N=128)
    st = State(c, 2, lo=c["N"] + 8, ld=2 * c["N"] + 16)
    before = st.snapshot()
    over = _refusals()[name](c, st, L)
    with pytest.raises(L.V2AError, match="v2a_gemm_cfg_euler") as e:
        seam_launch(L, c, st, 2.0, **over)
    assert "(-1)" in str(e.value), "V2A_ERR_ARG"
    torch.cuda.synchronize()
    for k, v in st.tensors().items():
        assert _same_bits(v, before[k]), (name, k)
    print("step-seam %-12s %-52s refused, nothing written" % ("8 refusals", name))


def test_the_refusal_state_is_launchable(L):
    """The state the refusals start from is accepted as it is: each refusal is due to the one argument it changes."""
    c = seam_case(RAGGED, N=128)
    st = State(c, 2, lo=c["N"] + 8, ld=2 * c["N"] + 16)
    seam_launch(L, c, st, 2.0)
    check_launch(L, "8 refusals", "%s N=128 the unchanged call" % (RAGGED,), c, st, 2, 2.0)


# ------------------------------------------------------------------------------------------------------------- 9. v2a_cfg_euler_planes
KEEP = 0.3
PRED_ROW_OFF = 4
#               copies trail  plane_row_off wide   C    T   B  pad step apg    strength
PLANES_CASES = [(1,    0,     4,            False, 4,   1,  1, 0,  0,   False, 2.0),
                (1,    0,     6,            True,  68,  37, 3, 16, 3,   True,  2.0),
                (1,    3,     4,            True,  260, 37, 1, 16, 3,   False, -0.5),
                (1,    3,     6,            False, 68,  1,  3, 0,  0,   True,  2.0),
                (2,    0,     4,            True,  68,  37, 3, 0,  3,   False, 0.0),
                (2,    0,     6,            False, 260, 1,  1, 16, 0,   True,  2.0),
                (2,    3,     4,            False, 4,   37, 3, 16, 3,   True,  -0.5),
                (2,    3,     6,            True,  260, 37, 3, 16, 1,   True,  2.0)]


def planes_case(copies, trail, prow, wide, C, T, B, pad, step, apg_on, strength):
    """pred (2 B, 4 + T, C) inside a flat buffer whose batch stride carries `pad` floats; y, dt; the geometry of the plane buffer."""
    key = ("planes", copies, trail, prow, wide, C, T, B, pad, step, apg_on, strength)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7919 * C + 31 * T + 5 * B + pad + step + 2 * copies + trail + prow)
        R = PRED_ROW_OFF
        pbs = (R + T) * C + pad
        flat = torch.randn(2 * B * pbs, generator=g)
        pred = flat.view(2 * B, pbs)[:, :(R + T) * C].unflatten(1, (R + T, C))
        lo = C + 8 if wide else C
        _CASES[key] = dict(B=B, T=T, C=C, pbs=pbs, flat=flat, pc=pred[:B, R:].clone(), pn=pred[B:, R:].clone(), y=torch.randn(B, T, C, generator=g),
                           dt=0.05 + 0.2 * torch.rand(NDT, generator=g), lo=lo, ld=lo + C + 4 if wide else 2 * C, rps=prow + T + trail, prow=prow,
                           copies=copies, step=step, apg_on=apg_on, strength=strength)
    return _CASES[key]


@pytest.mark.parametrize("case", PLANES_CASES, ids=lambda t: "-".join(str(v) for v in t))
def test_cfg_euler_planes(L, case):
    c = planes_case(*case)
    B, T, C, rps, prow, copies, s, step = (c[k] for k in ("B", "T", "C", "rps", "prow", "copies", "strength", "step"))
    pred, dt = c["flat"].to(DEV), c["dt"].to(DEV)
    kw = dict(B=B, T=T, C_=C, pred_batch_stride=c["pbs"], row_off=PRED_ROW_OFF)
    n = c["y"].numel()
    y = torch.full((n + GUARD,), SENT, device=DEV)
    y[:n] = c["y"].reshape(-1).to(DEV)
    plain = c["y"].to(DEV).clone()
    apg = None
    if c["apg_on"]:
        apg = torch.tensor([1e300, -7.0] * B, dtype=torch.float64, device=DEV)      # garbage: the call itself zeroes it
        L.apg_reduce(pred, apg, **kw)
    st = torch.tensor([step], dtype=torch.int32, device=DEV)
    rows = 2 * B * rps                                        # room for two copies whatever `copies` is
    buf = torch.full((rows, c["ld"]), SENT, dtype=torch.bfloat16, device=DEV)
    L.cfg_euler(y, pred, cfg_strength=s, dt=dt, step=st, apg=apg, keep=KEEP,
                planes=dict(out=buf, ld=c["ld"], lo_offset=c["lo"], row_off=prow, rows_per_seq=rps, copies=copies), **kw)
    L.cfg_euler(plain, pred, cfg_strength=s, dt=dt, step=st, apg=apg, keep=KEEP, **kw)
    torch.cuda.synchronize()
    yf = y.cpu()
    y_new = yf[:n].reshape(B, T, C)
    h = float(c["dt"][step])
    ref, par = _euler_ref(c["y"], c["pc"], c["pn"], h, s, _apg_sums_ref(c["pc"], c["pn"], None) if c["apg_on"] else None, KEEP)
    r = _report_tol("9 planes", "-".join(str(v) for v in case), "y", y_new, ref, tol_euler(c["y"], c["pc"], c["pn"], par, h, s))
    assert r <= 1.0, r
    assert int(st.item()) == step, "the step counter is not this launch's to advance"
    assert bool((yf[n:] == SENT).all()), "the guard tail behind y"
    assert _same_bits(y_new, plain.cpu()), "y is updated exactly as by v2a_cfg_euler"
    assert not torch.equal(y_new, c["y"])
    assert _same_bits(buf.cpu(), expected_planes(y_new, rows, c["ld"], c["lo"], rps, prow, copies))
