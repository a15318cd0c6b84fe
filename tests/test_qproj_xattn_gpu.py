"""v2a_qproj_xattn (csrc/qproj_xattn.hip: q-projection, folded RMSNorm row scale, bias, RoPE, one-tile cross-attention and head gate
in one launch) against a float64 restatement of the whole operation, on the K loops, strides, epilogue options and tile edges that
tests/test_kernels_gpu.py::test_qproj_xattn_* (bit equality with v2a_gemm + v2a_attention on tightly packed operands) do not launch.

The dispatch (v2a_qproj_xattn; csrc/attn_core.h, attn_clamp_mode) picks

  S3       qproj_xattn_kernel<C, false> on bf16 operands (bf16 A, W, K, V, bf16 output rows), <C, true> on V2A_BF16_SPLIT ones
           (hi | lo planes of A and W, fp32 K and V, output rows as hi | lo planes, the lo plane H*64 columns after the hi one)
  CLAMP    0 without a clamp; 2 (bounded weights, no maximum) while clamp * log2 e + log2 Nk <= 90; else 1 -- the mode v2a_attention
           would pick for these keys.  Clamp 50 -> 2, 80 -> 1, 0 -> 0 at every Nk <= 64
  grid     ceil(Nq / 64) * B * H workgroups of 64 tokens x one head, 4 waves of 16 tokens; nk = K / 64 trips of a 3-stage ring
           unrolled by three; dynamic LDS = the ring + the head's gate row of W (K, split 2 K, bf16) + 64 row scales

The reference (qx_qgate64, qx_ref64; checked on the CPU by tests/test_qproj_xattn_refs.py) works from the operands as stored -- bf16
values, or hi + lo summed in float64: z = A W^T over the H*64 q rows and the H gate rows of W; x sqrt(row_norm_dim) / sqrt(sum of the
row's row_ssq parts); + bias; interleaved RoPE of the q columns below rope_cols at position rope_pos_offset + m mod Nq; bf16 mode
rounds q and the gate logit to bf16 (the [q | gate] buffer of the two-launch path), split mode rounds neither; then attn_ref64 of
tests/test_attention_paths_gpu.py.  Split outputs are compared as hi + lo, and the planes are held to hi = bf16(o), lo = bf16(o - hi)
as far as they show it: |lo| <= ulp_bf16(hi) / 2, lo == 0 where hi == 0.

Every launch writes into rows of 8 pad columns and batch entries of 2 pad rows prefilled with SENTINEL: the pad must keep it, every
live column must have lost it and be finite, rows >= q_len and every row of a clip without keys must be == 0.0.  Operand pad (the
"engine" layouts) is NaN, the row_ssq columns behind `parts` hold 1e30: a read outside the operand shows.

Inputs follow tests/test_attention_paths_gpu.py, with q and k at 1.5 instead of 2: a ~ N(0, 1), q rows of W ~ N(0, 2.25 / K), gate rows
~ N(0, 1 / K), bias ~ N(0, 0.09), k ~ N(0, 2.25), v ~ N(0, 1): logits of spread 2.25 before the clamp, |v| < 6.  At spread 4 the bf16
rounding of q alone moves the float64 result by up to 1.8 times half the bf16 bar, at 2.25 by 0.78 of it
(tests/test_qproj_xattn_refs.py::test_inputs_leave_room_under_the_bf16_bar): the scale was lowered, not the bar.  Tolerances are the
ones the project holds these kernels to (atol = rtol): 2e-2 bf16, 2e-4 split (TOL of test_attention_paths_gpu.py); saturated case
2e-2 / 1e-4 absolute (test_mode2_at_rule_limit).

What each test reaches, and the largest error it measured on an MI355X (max |got - ref| / max |ref| over its cases):

  test_k_ring      B=2 H=3 Nq=70 Nk=40 (12 workgroups: XCD remap with a remainder; second tile of 6 live rows), K = 512 .. 4096:
                   nk = 8, 16, 24, 32, 48, 64, nk mod 3 = 2, 1, 0, 2, 0, 1 -- the loop ends on tile<1>, tile<0>, tile<2>; K = 4096
                   asks for all of smem_max, first in the process ("k4096_first", when the module runs alone) and after smaller
                   requests ("k4096_last"); K = 1536 and 4096 also equal the two launches bit for bit
                   bf16 6.2e-03, split 1.5e-05
  test_engine_strides  B=3 H=3 Nq=130 Nk=64 K=1024, folded + bias + RoPE, the layouts of dit.py::_audio_cross_attention: A and W rows
                   of K + 24 (split 2 K + 24) inside NaN buffers, N = H*64 + 16, k and v slices of one buffer of row stride
                   4*H*64 + 8 ("engine") or two buffers of row strides H*64 + 8 and 2*H*64 + 16 ("engine2"), batch strides beyond
                   Nk rows; clamp 50, 80, 0; every case also equals the two launches bit for bit
                   bf16 5.8e-03, split 1.1e-05
  test_epilogue_options  the same shape, packed operands: folded alone and RoPE alone, rope_cols = 64 of 192 at offsets 0 and 7,
                   no bias, kv_len or q_len absent; folded at K = 512 and 1024 (16 and 32 row_ssq parts in rows of 40)
                   bf16 6.4e-03 (rope_cols64-off0), split 1.8e-05 (folded_only-K512)
  test_tile_edges  K=512: Nq = 65 (three of four waves of the last tile leave early), 1, 64; Nk = 1, 5, 64 with kv_len 31 / 32 /
                   33 / 64; a clip with q_len 0; split H = 16 (32 workgroups: no remainder in the XCD remap)
                   bf16 4.9e-03 (nk1), split 1.6e-05 (q_len0)
  test_clamp_rule_limit_saturated  Nk = 1 and 64 at clamp 62 / 58 (the last integers with CLAMP = 2) and 63 / 59 (CLAMP = 1), every
                   logit at +-2304: the output is sigmoid(gate) x the mean of v over the live keys
                   absolute: bf16 1.56e-02 = 4 * 2^-8 (Nk 1, clamp 62, sign +; Nk 64: 4.2e-03), split 4.6e-05 (the same case;
                   Nk 64: 8.1e-06)

The whole file: 65 tests, 85 fused launches, in 1.3 s on the MI355X."""
import functools
import math

import pytest
import torch

from test_attention_paths_gpu import SCALE, SENTINEL, TOL, _clamp_mode, attn_ref64
from test_gemm_split_ring_gpu import _rope_ref, _rope_table, _split_planes

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SSQ_SENTINEL = 1e30
OUT_PAD_COLS, OUT_PAD_ROWS = 8, 2
DTS = ["bf16", "split"]
QK_STD = 1.5            # 2.0 (test_attention_paths_gpu.py) fails test_inputs_leave_room_under_the_bf16_bar: 1.8 half-bars; 1.5: 0.78

K_RING = [512, 1024, 1536, 2048, 3072, 4096]
K_ORDERS = {"k4096_first": [4096, 512, 1024, 1536, 2048, 3072], "k4096_last": [512, 1024, 1536, 2048, 3072, 4096]}
K_TWO_LAUNCH = [1536, 4096]


def _case(B, H, Nq, Nk, kv_len, q_len, K, clamp=50.0, folded=False, rope=False, rope_cols=None, rope_off=0, bias=True, layout="tight",
          dts=("bf16", "split")):
    return dict(B=B, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len, q_len=q_len, K=K, clamp=clamp, folded=folded, rope=rope,
                rope_cols=(H * 64 if rope_cols is None else rope_cols) if rope else 0, rope_off=rope_off if rope else 0, bias=bias,
                layout=layout, dts=dts)


_RING_SHAPE = (2, 3, 70, 40, (40, 17), (70, 5))
_BASE_SHAPE = (3, 3, 130, 64, (64, 33, 0), (130, 64, 1))
RING_CASES = {"K%d" % K: _case(*_RING_SHAPE, K, clamp=50.0) for K in K_RING}
ENGINE_CASES = {"%s-clamp%g" % (lay, c): _case(*_BASE_SHAPE, 1024, clamp=c, folded=True, rope=True, rope_off=0, layout=lay)
                for lay in ("engine", "engine2") for c in (50.0, 80.0, 0.0)}
EPILOGUE_CASES = {
    "folded_only-K512": _case(*_BASE_SHAPE, 512, folded=True),
    "folded_only-K1024": _case(*_BASE_SHAPE, 1024, folded=True),
    "rope_only": _case(*_BASE_SHAPE, 1024, rope=True, rope_off=3),
    "rope_cols64-off0": _case(*_BASE_SHAPE, 512, rope=True, rope_cols=64, rope_off=0),
    "rope_cols64-off7": _case(*_BASE_SHAPE, 512, rope=True, rope_cols=64, rope_off=7),
    "no_bias-K512": _case(*_BASE_SHAPE, 512, folded=True, rope=True, rope_off=2, bias=False),
    "no_bias-K1024": _case(*_BASE_SHAPE, 1024, folded=True, rope=True, rope_off=2, bias=False),
    "no_kv_len": _case(3, 3, 130, 64, None, (130, 64, 1), 512, folded=True, rope=True, rope_off=2),
    "no_q_len": _case(3, 3, 130, 64, (64, 33, 0), None, 512, folded=True, rope=True, rope_off=2),
}
_EDGE = dict(folded=True, rope=True, rope_off=2)
EDGE_CASES = {
    "nq65": _case(2, 3, 65, 40, (40, 17), (65, 64), 512, **_EDGE),
    "nq1": _case(3, 3, 1, 40, (40, 1, 0), (1, 1, 1), 512, **_EDGE),
    "nq64": _case(2, 3, 64, 40, (40, 17), (64, 63), 512, **_EDGE),
    "nk1": _case(2, 3, 70, 1, (1, 0), (70, 5), 512, **_EDGE),
    "nk64-fragment-edge": _case(4, 3, 70, 64, (31, 32, 33, 64), (70, 70, 69, 1), 512, **_EDGE),
    "nk5": _case(2, 3, 70, 5, (5, 3), (70, 10), 512, **_EDGE),
    "q_len0": _case(3, 3, 70, 40, (40, 40, 17), (70, 0, 64), 512, **_EDGE),
    "h16": _case(1, 16, 70, 40, (33,), (70,), 512, dts=("split",), **_EDGE),
}
CASE_LISTS = {"ring": RING_CASES, "engine": ENGINE_CASES, "epilogue": EPILOGUE_CASES, "edges": EDGE_CASES}


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------------------- the float64 reference
# (checked against torch and against its own definitions on the CPU by tests/test_qproj_xattn_refs.py)
def qx_qgate64(a, w, *, H, Nq, bias=None, row_ssq=None, row_norm_dim=0, rope_table=None, rope_cols=0, rope_pos_offset=0, round_bf16=False):
    """float64 (M, H*64 + H) = [q | gate logits] of the stored a (M, K) and w (>= H*65, K) at the point where attention reads them."""
    n = H * 64 + H
    z = a.double() @ w.double()[:n].t()
    if row_ssq is not None:
        parts = row_norm_dim // 32
        z = z * (math.sqrt(row_norm_dim) / row_ssq.double()[:, :parts].sum(1).sqrt().clamp_min(1e-12))[:, None]
    if bias is not None:
        z = z + bias.double()[:n]
    if rope_table is not None:
        z = _rope_ref(z, rope_table, rope_cols, Nq, rope_pos_offset)
    if round_bf16:
        z = z.float().bfloat16().double()
    return z


def qx_ref64(a, w, k, v, *, B, H, Nq, kv_len=None, q_len=None, scale=SCALE, clamp=0.0, **qkw):
    """float64 (B, Nq, H*64) of the whole operation: qx_qgate64, then attn_ref64 over k, v (B, Nk, H*64) as stored."""
    z = qx_qgate64(a, w, H=H, Nq=Nq, **qkw)
    Nk = k.shape[1]
    heads = lambda t, n: t.double().reshape(B, n, H, 64).permute(0, 2, 1, 3)
    gate = z[:, H * 64:].reshape(B, Nq, H).permute(0, 2, 1)
    o = attn_ref64(heads(z[:, :H * 64], Nq), heads(k, Nk), heads(v, Nk), gate, list(kv_len) if kv_len is not None else [Nk] * B,
                   list(q_len) if q_len is not None else [Nq] * B, scale, clamp)
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * 64).contiguous()


def _planes64(p, k):
    """[hi k | lo k] bf16 rows -> their float64 sum."""
    return p[..., :k].double() + p[..., k:2 * k].double()


def _ulp_bf16(x):
    """Spacing of bf16 at the (normal, non-zero) float64 values x: 2^(floor(log2 |x|) - 7)."""
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 8)


# ------------------------------------------------------------------------------------------------------------- operands, made once per case
@functools.lru_cache(maxsize=None)
def _raw(B, H, Nq, Nk, K, folded):
    """fp32 operands on the CPU from a generator seeded by the shape (shared by every case of that shape, never written to)."""
    g = torch.Generator().manual_seed(100003 * K + 1009 * Nq + 31 * Nk + 7 * H + B)
    M, inner, N = B * Nq, H * 64, H * 64 + 16
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    w[:inner] *= QK_STD                                # q, k ~ N(0, QK_STD^2): logits 0.125 q.k of spread QK_STD^2
    bias = 0.3 * torch.randn(N, generator=g)
    k = torch.randn(B, Nk, inner, generator=g) * QK_STD
    v = torch.randn(B, Nk, inner, generator=g)
    ssq = None
    if folded:                                         # the sums of squares of 32 columns, off by a factor per row: scales of 0.8 .. 1.3 / rms
        parts = K // 32
        ssq = torch.full((M, 40), SSQ_SENTINEL)
        ssq[:, :parts] = a.reshape(M, parts, 32).square().sum(-1) * (torch.rand(M, 1, generator=g) + 0.6)
    return a, w, bias, k, v, ssq


def operands(case, dt):
    """The operands of a case as stored for dt, on the CPU: a, w (bf16; split: [hi | lo] planes), k, v (bf16; split: fp32), bias, ssq, rope
    table (fp32 or None), and the float64 values a64, w64, k64, v64 the stored ones stand for."""
    a, w, bias, k, v, ssq = _raw(case["B"], case["H"], case["Nq"], case["Nk"], case["K"], case["folded"])
    K = case["K"]
    o = dict(bias=bias if case["bias"] else None, ssq=ssq, tab=_rope_table(case["rope_off"] + case["Nq"]) if case["rope"] else None)
    if dt == "split":
        o.update(a=_split_planes(a), w=_split_planes(w), k=k, v=v)
        o.update(a64=_planes64(o["a"], K), w64=_planes64(o["w"], K))
    else:
        o.update(a=a.bfloat16(), w=w.bfloat16(), k=k.bfloat16(), v=v.bfloat16())
        o.update(a64=o["a"].double(), w64=o["w"].double())
    o.update(k64=o["k"].double(), v64=o["v"].double())
    return o


def reference(case, dt, round_bf16=None):
    """qx_ref64 of a case's stored operands; q and gate rounded to bf16 in bf16 mode unless round_bf16 says otherwise."""
    o = operands(case, dt)
    return qx_ref64(o["a64"], o["w64"], o["k64"], o["v64"], B=case["B"], H=case["H"], Nq=case["Nq"], kv_len=case["kv_len"], q_len=case["q_len"],
                    clamp=case["clamp"], bias=o["bias"], row_ssq=o["ssq"], row_norm_dim=case["K"] if case["folded"] else 0, rope_table=o["tab"],
                    rope_cols=case["rope_cols"], rope_pos_offset=case["rope_off"], round_bf16=(dt == "bf16") if round_bf16 is None else round_bf16)


_REFS = {}


def _ref(lst, name, dt):
    """The reference of CASE_LISTS[lst][name], computed once (the layout does not enter it) and never written to."""
    case = CASE_LISTS[lst][name]
    key = (tuple(sorted((k, v) for k, v in case.items() if k not in ("layout", "dts"))), dt)
    if key not in _REFS:
        _REFS[key] = reference(case, dt)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------------------- launches
def _padded(t, ld, col0):
    """The (rows, cols) tensor t as a view at column col0 of a NaN buffer of row stride ld, on the device."""
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf.to(DEV)[:, col0:col0 + t.shape[1]]


def _device(case, dt):
    """Device copies of a case's operands in its layout, and the arguments both paths share.
    tight    packed A and W rows, [k | v] rows of 2*H*64
    engine   A at column 8 and W at column 16 of NaN buffers of row stride K + 24 (split: 2 K + 24); k at column H*64 + 8 and v at column
             3*H*64 of one NaN buffer of row stride 4*H*64 + 8 and Nk + 2 rows per clip
    engine2  A and W as in engine; k in a buffer of row stride H*64 + 8 and Nk + 1 rows per clip, v in one of 2*H*64 + 16 and Nk + 3"""
    o = operands(case, dt)
    B, H, Nq, Nk, K = (case[x] for x in ("B", "H", "Nq", "Nk", "K"))
    inner, pl = H * 64, 2 if dt == "split" else 1
    d = dict(keep=[])
    if case["layout"] == "tight":
        d["a"], d["w"] = o["a"].to(DEV), o["w"].to(DEV)
        kv = torch.cat([o["k"], o["v"]], -1).to(DEV)
        es = kv.element_size()
        d["k"], d["v"] = kv.data_ptr(), kv.data_ptr() + inner * es
        d["kv_strides"] = (2 * inner, 2 * inner, Nk * 2 * inner, Nk * 2 * inner)
        d["keep"].append(kv)
    else:
        ld = pl * K + 24
        d["a"], d["w"] = _padded(o["a"], ld, 8), _padded(o["w"], ld, 16)
        if case["layout"] == "engine":
            rs, rows = 4 * inner + 8, Nk + 2
            kv = torch.full((B, rows, rs), NAN, dtype=o["k"].dtype)
            kv[:, :Nk, inner + 8:2 * inner + 8] = o["k"]
            kv[:, :Nk, 3 * inner:4 * inner] = o["v"]
            kv = kv.to(DEV)
            es = kv.element_size()
            d["k"], d["v"] = kv.data_ptr() + (inner + 8) * es, kv.data_ptr() + 3 * inner * es
            d["kv_strides"] = (rs, rs, rows * rs, rows * rs)
            d["keep"].append(kv)
        else:
            krs, vrs, krows, vrows = inner + 8, 2 * inner + 16, Nk + 1, Nk + 3
            kb = torch.full((B, krows, krs), NAN, dtype=o["k"].dtype)
            vb = torch.full((B, vrows, vrs), NAN, dtype=o["v"].dtype)
            kb[:, :Nk, :inner] = o["k"]
            vb[:, :Nk, 16:16 + inner] = o["v"]
            kb, vb = kb.to(DEV), vb.to(DEV)
            d["k"], d["v"] = kb.data_ptr(), vb.data_ptr() + 16 * vb.element_size()
            d["kv_strides"] = (krs, vrs, krows * krs, vrows * vrs)
            d["keep"] += [kb, vb]
        assert d["a"].stride(0) == ld and d["w"].stride(0) == ld and d["kv_strides"][2] > Nk * d["kv_strides"][0]
    d["bias"] = o["bias"].to(DEV) if o["bias"] is not None else None
    d["kvl"] = torch.tensor(case["kv_len"], dtype=torch.int32, device=DEV) if case["kv_len"] is not None else None
    d["ql"] = torch.tensor(case["q_len"], dtype=torch.int32, device=DEV) if case["q_len"] is not None else None
    d["epi"] = {}
    if case["rope"]:
        d["epi"].update(rope_table=o["tab"].to(DEV), rope_cols=case["rope_cols"], rope_pos_offset=case["rope_off"])
    if case["folded"]:
        d["epi"].update(row_ssq=o["ssq"].to(DEV), row_norm_dim=K)
    return d


def _out(case, dt):
    """(B, Nq + 2, width + 8) bf16 of SENTINEL: width = H*64 (split: 2*H*64), the written region is [:, :Nq, :width]."""
    width = case["H"] * 64 * (2 if dt == "split" else 1)
    return torch.full((case["B"], case["Nq"] + OUT_PAD_ROWS, width + OUT_PAD_COLS), SENTINEL, dtype=torch.bfloat16, device=DEV)


def _fused(L, case, dt, d):
    """One v2a_qproj_xattn launch; the whole output buffer, on the CPU."""
    B, H, Nq, Nk, K = (case[x] for x in ("B", "H", "Nq", "Nk", "K"))
    out = _out(case, dt)
    L.qproj_xattn(d["a"], d["a"].stride(0), K, d["w"], bias=d["bias"], M=B * Nq, N=H * 64 + 16, rows_per_batch=Nq, k=d["k"], v=d["v"],
                  out=out.data_ptr(), kv_strides=d["kv_strides"], out_strides=(out.stride(1), out.stride(0)), B=B, H=H, Nk=Nk, kv_len=d["kvl"],
                  q_len=d["ql"], scale=SCALE, softclamp=case["clamp"], split=dt == "split", **d["epi"])
    torch.cuda.synchronize()
    return out.cpu()


def _two_launches(L, case, dt, d):
    """The same operands through v2a_gemm (tile_hint 4; split: tile_hint 1, a_split) into a [q | gate] buffer, then v2a_attention, as
    tests/test_kernels_gpu.py::test_qproj_xattn_equals_two_launches and ..._split_equals_two_launches build it."""
    B, H, Nq, Nk, K = (case[x] for x in ("B", "H", "Nq", "Nk", "K"))
    M, inner, N = B * Nq, H * 64, H * 64 + 16
    split = dt == "split"
    qb = torch.zeros(M, N, dtype=torch.float32 if split else torch.bfloat16, device=DEV)
    L.gemm([(d["a"], d["a"].stride(0), K)], d["w"], qb, M=M, N=N, compute=L.BF16, bias=d["bias"], rows_per_batch=Nq,
           **(dict(a_split=True, tile_hint=1) if split else dict(tile_hint=4)), **d["epi"])
    out = _out(case, dt)
    krs, vrs, kbs, vbs = d["kv_strides"]
    L.attention(qb.data_ptr(), d["k"], d["v"], qb.data_ptr() + inner * qb.element_size(), out.data_ptr(),
                strides=(N, krs, vrs, N, out.stride(1), Nq * N, kbs, vbs, Nq * N, out.stride(0)), B=B, H=H, Nq=Nq, Nk=Nk, kv_len=d["kvl"],
                q_len=d["ql"], scale=SCALE, softclamp=case["clamp"], dtype=L.BF16_SPLIT if split else L.BF16, out_split=split)
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------------------- checks
def _written(out, case, dt):
    """The pad keeps the prefill, every live column was written and is finite; the output as float64 (B, Nq, H*64), split: hi + lo after
    the planes passed |lo| <= ulp_bf16(hi) / 2 and lo == 0 where hi == 0."""
    Nq, inner = case["Nq"], case["H"] * 64
    width = inner * (2 if dt == "split" else 1)
    assert bool((out[:, :Nq, width:] == SENTINEL).all()), "a pad column beside the rows was written"
    assert bool((out[:, Nq:] == SENTINEL).all()), "a pad row behind a clip was written"
    got = out[:, :Nq, :width].float()
    assert bool((got != SENTINEL).all()), "%d output elements were never written" % int((got == SENTINEL).sum())
    assert bool(torch.isfinite(got).all()), "%d non-finite outputs, clips %s" % (
        int((~torch.isfinite(got)).sum()), sorted(set((~torch.isfinite(got)).nonzero()[:, 0].tolist())))
    got = got.double()
    if dt != "split":
        return got
    hi, lo = got[..., :inner], got[..., inner:]
    nz = hi != 0
    assert bool((lo[~nz] == 0).all()), "a lo plane element under hi == 0 is not zero"
    assert bool((lo[nz].abs() <= _ulp_bf16(hi[nz]) / 2).all()), "|lo| > ulp_bf16(hi) / 2: lo is not bf16(o - hi) of any o with hi = bf16(o)"
    return hi + lo


_WORST = {}


def _check(out, ref, case, dt, label, test):
    got = _written(out, case, dt)
    kv_len = case["kv_len"] if case["kv_len"] is not None else [case["Nk"]] * case["B"]
    q_len = case["q_len"] if case["q_len"] is not None else [case["Nq"]] * case["B"]
    for b in range(case["B"]):      # exact zeros, not zeros within the tolerance
        dead = got[b] if kv_len[b] == 0 else got[b, q_len[b]:]
        assert not dead.numel() or float(dead.abs().max()) == 0.0, "clip %d: a row without keys or past q_len is not zero" % b
    err = float((got - ref).abs().max() / ref.abs().max())
    _WORST[(test, dt)] = max(_WORST.get((test, dt), 0.0), err)
    print(f"qproj_xattn {label} {dt}: {err:.2e} of max |ref| (bar {TOL[dt]:.0e}); largest of {test} {dt} so far {_WORST[(test, dt)]:.2e}")
    torch.testing.assert_close(got, ref, atol=TOL[dt], rtol=TOL[dt])


def _run(L, lst, name, dt, test, two_launches=False):
    case = CASE_LISTS[lst][name]
    d = _device(case, dt)
    out = _fused(L, case, dt, d)
    _check(out, _ref(lst, name, dt), case, dt, f"{lst} {name}", test)
    if two_launches:
        two = _two_launches(L, case, dt, d)
        assert torch.equal(out, two), "fused != v2a_gemm + v2a_attention: max |delta| %g" % float((out.float() - two.float()).abs().max())


def _of(lst):
    return [(n, dt) for n, c in CASE_LISTS[lst].items() for dt in DTS if dt in c["dts"]]


# ------------------------------------------------------------------------------------------------------------- the K ring (first in the file: K = 4096 opens the module)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("order", list(K_ORDERS))
def test_k_ring(L, order, dt):
    """nk = K / 64 = 8, 16, 24, 32, 48, 64 trips: the unrolled loop ends on tile<1>, tile<0>, tile<2>, tile<1>, tile<2>, tile<0>, each with its own
    counted waits in the last two trips.  K = 4096 requests exactly smem_max of dynamic LDS (61.8 KB bf16, 122.6 KB split): as the first launch of
    qproj_xattn_kernel<2, S3> in the process when this module runs alone, and after smaller requests.  K = 1536 and 4096 are also held to bit
    equality with v2a_gemm + v2a_attention, which the tests of test_kernels_gpu.py stop short of."""
    for K in K_ORDERS[order]:
        _run(L, "ring", "K%d" % K, dt, "test_k_ring", two_launches=K in K_TWO_LAUNCH)


# ------------------------------------------------------------------------------------------------------------- the engine's strides
@pytest.mark.parametrize("name,dt", _of("engine"))
def test_engine_strides(L, name, dt):
    """lda, ldw, the lo plane K (not lda / 2) elements into a row, k and v row and batch strides that differ from the width and (engine2) from each
    other, out row and batch strides: a wrong multiply reads NaN pad or misses the reference; the pad of the output keeps its prefill.  Three
    query tiles per clip, the last with two live rows; a clip without keys; CLAMP = 2, 1, 0.  Each case also equals the two launches bit for bit."""
    _run(L, "engine", name, dt, "test_engine_strides", two_launches=True)


# ------------------------------------------------------------------------------------------------------------- epilogue options, one at a time
@pytest.mark.parametrize("name,dt", _of("epilogue"))
def test_epilogue_options(L, name, dt):
    """The row scale without RoPE and RoPE without the row scale; rope_cols = 64 leaves heads 1 and 2 unrotated (the n < rope_cols branch) at position
    offsets 0 and 7; no bias (q and gate); kv_len absent (all Nk keys live) and q_len absent (no dead rows).  The row_ssq rows hold 16 or 32
    parts and 1e30 behind them: a read past `parts` collapses the scale."""
    _run(L, "epilogue", name, dt, "test_epilogue_options")


# ------------------------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("name,dt", _of("edges"))
def test_tile_edges(L, name, dt):
    """Nq = 65: a tile with one live row (waves 1 .. 3 return before the store, rows clamped to the clip's last); Nq = 1: every row of every tile
    clamped; Nq = 64: no partial tile; Nk = 1 and 5: key rows clamped to the last; Nk = 64 with kv_len on both sides of the 32-key fragment edge;
    a clip with q_len 0; split at H = 16: 32 workgroups, the XCD remap without a remainder (H = 3 leaves one everywhere else)."""
    _run(L, "edges", name, dt, "test_tile_edges")


# ------------------------------------------------------------------------------------------------------------- clamp rule limit, saturated logits
SAT_GATES = (20.0, 0.5, -1.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("Nk", [1, 64])
def test_clamp_rule_limit_saturated(L, Nk, mode, sign, dt):
    """The largest integer clamp with CLAMP = 2 at this Nk (62 at 1 key, 58 at 64: c log2 e + log2 Nk <= 90) and the next one (CLAMP = 1), every logit
    far beyond +-clamp as in test_attention_saturated_logits: a = 1, q rows of W = 12 / K, k = +-24, so q = 12 and 0.125 q.k = +-2304 exactly; gate
    rows 20 / K, 0.5 / K, -1 / K.  All live keys weigh the same: the output is sigmoid(gate) x the mean of v over them (kv_len Nk and (Nk + 1) / 2),
    finite.  |v| <= 4: with one live key the output is v p' / p with p' the weight as the PV product reads it (bf16: within 2^-9 of p; hi + lo:
    2^-17) and is then stored (bf16: 2^-9 again; hi | lo: 2^-17), so the formats alone cost |v| 2^-8 = 1.6e-2 of the 2e-2 at |v| = 4 and
    |v| 2^-16 = 6.1e-5 of the 1e-4.  At |v| <= 8 (test_mode2_at_rule_limit, whose 200 keys average it away) this test measured exactly that: one bf16
    step of 2^-5 in bf16 mode, 9.2e-5 in split mode, both at Nk = 1, clamp 62, sign +.  The two launches must give the same bits here too."""
    c2 = max(i for i in range(1, 200) if _clamp_mode(float(i), Nk) == 2)
    assert c2 == {1: 62, 64: 58}[Nk] and _clamp_mode(float(c2 + 1), Nk) == 1
    clamp = float(c2 if mode == 2 else c2 + 1)
    B, H, Nq, K = 2, 3, 70, 512
    inner, N, split = H * 64, H * 64 + 16, dt == "split"
    kv_len = [Nk, (Nk + 1) // 2]
    case = _case(B, H, Nq, Nk, kv_len, None, K, clamp=clamp)
    a = torch.ones(B * Nq, K)
    w = torch.zeros(N, K)
    w[:inner] = 12.0 / K                                                          # exact in bf16, as every partial sum of the product
    for h, gv in enumerate(SAT_GATES):
        w[inner + h] = gv / K
    k = torch.full((B, Nk, inner), sign * 24.0)
    v = (torch.rand(B, Nk, inner, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 4.0
    if split:
        ad, wd, kv = _split_planes(a).to(DEV), _split_planes(w).to(DEV), torch.cat([k, v], -1).to(DEV)
    else:
        ad, wd, kv = a.bfloat16().to(DEV), w.bfloat16().to(DEV), torch.cat([k, v], -1).bfloat16().to(DEV)
    d = dict(a=ad, w=wd, k=kv.data_ptr(), v=kv.data_ptr() + inner * kv.element_size(), kv_strides=(2 * inner, 2 * inner, Nk * 2 * inner, Nk * 2 * inner),
             bias=None, kvl=torch.tensor(kv_len, dtype=torch.int32, device=DEV), ql=None, epi={})
    out = _fused(L, case, dt, d)
    got = _written(out, case, dt)
    assert torch.equal(out, _two_launches(L, case, dt, d))
    v64 = kv[..., inner:].cpu().double()
    mean = torch.stack([v64[b, :kv_len[b]].mean(0) for b in range(B)])                      # (B, inner)
    gate = torch.sigmoid(torch.tensor(SAT_GATES, dtype=torch.float64)).repeat_interleave(64)
    ref = (mean * gate)[:, None, :].expand(B, Nq, inner)
    err = float((got - ref).abs().max())
    key = ("test_clamp_rule_limit_saturated", dt)
    _WORST[key] = max(_WORST.get(key, 0.0), err)
    print(f"qproj_xattn saturated Nk {Nk} clamp {clamp:g} (mode {mode}) sign {sign:+g} {dt}: {err:.2e} absolute; largest so far {_WORST[key]:.2e}")
    torch.testing.assert_close(got, ref, atol=1e-4 if split else 2e-2, rtol=0)
