"""v2a_attention against a float64 restatement on the dispatch paths that tests/test_kernels_gpu.py::test_attention and
tests/test_dinov2_gpu.py do not reach.  The dispatch (csrc/attention.hip, v2a_attention; csrc/attn_core.h, attn_clamp_mode) picks

  kernel   attn_rowlane_kernel<float | bf16_t> when a q / k / v / out address or stride misses the vector alignment, else
           attn_mfma_f32_kernel (fp32), attn_mfma_kernel (bf16), attn_mfma_split_kernel (BF16_SPLIT)
  NG       key groups per workgroup, nwg = ceil(Nq / 64) * H * B: fp32 2 when Nk > 128; bf16 2 when Nk > 128 and
           nwg < attn_one_group_from (1536); split 2 when Nk > 128 and nwg < 200 (or < the override), else NG = 1 with QG = 2
           (128 queries per workgroup) when Nq > 64 and Nk > 128, else NG = 1, QG = 1; set_tuning(reserved=256): QG = 1
  CLAMP    0 without a clamp; 2 (bounded weights, no running maximum) while clamp * log2 e + log2 Nk <= 90; else 1

Base shape B=8 H=3 Nq=130 Nk=200 (72 workgroups; three 64-query blocks, the last with two live rows; four key tiles, the last
with 8 keys), kv_len 0 / 1 / 63 / 64 / 65 / 128 / 129 / 200: no key, one key, both sides of the first two tile edges, key
group 1 wholly empty (kv_len <= 64) or with one tile (129); q_len 130 / 1 / 0 / 64 / 65 / 129 / 130 / 100.  Clamp 50 -> mode
2, 80 -> mode 1, 0 -> mode 0 at every Nk used here.  Buffers are packed as the engine packs them ([q | gate] rows, [k | v]
rows), the output rows carry 8 pad columns that must keep their prefill.  Every check also holds rows >= q_len and every row of
a batch entry without keys to exact zeros, and the whole output to isfinite before any comparison.

Tolerances are the ones test_attention holds these kernels to (atol = rtol): 2e-5 fp32, 2e-4 split, 2e-2 bf16.

What each test reaches, and the largest error it measured on an MI355X (max |got - ref| / max |ref| over its cases; taken on
the library as it was before the merge guard for key-less groups, over the cases that were finite there):

  test_base_shape  form "default":  attn_mfma_f32_kernel<2, C>, attn_mfma_kernel<2, C>, attn_mfma_split_kernel<2, C, 1>
                   form "one_group" (attn_one_group_from=1):  attn_mfma_kernel<1, C>, attn_mfma_split_kernel<1, C, 2>
                   form "one_group_q64" (and reserved=256):  attn_mfma_split_kernel<1, C, 1>;  C = 2, 1, 0; gate dense and None
                   fp32 1.9e-06, split 1.4e-05, bf16 5.5e-03
  test_second_shapes  Nq=100 Nk=129: default NG = 2 (all three kernels); one_group: bf16 NG = 1, split <1, C, 2> whose second
                   query group holds 36 of 64 rows.  Nq=64 Nk=200: default NG = 2; one_group: bf16 NG = 1, split <1, C, 1> by
                   the Nq <= 64 rule.  Nq=70 Nk=40: one key tile, NG = 1, QG = 1 in all three kernels.  C = 2, 1.
                   (In the default dispatch the split kernel takes NG = 2 at these workgroup counts, so the two QG rules are
                   reached under attn_one_group_from=1.)
                   fp32 3.3e-06, split 2.3e-05, bf16 4.6e-03
  test_two_forms_agree  bf16 <2, C> against <1, C>; split <2, C, 1> against <1, C, 2> and <1, C, 1>: bf16 8.7e-04, split 3.2e-07
  test_out_split_planes_exact  the three split forms with out_split: hi == bf16(o), lo == bf16(o - hi) of the fp32 output, bit for bit
  test_unaligned_fallback  attn_rowlane_kernel<float> (fp32 and BF16_SPLIT tensors) and attn_rowlane_kernel<bf16_t>, reached by
                   (a) a q / gate row stride of H*64+17, (b) k / v one element past an aligned address, (c) an output row
                   stride of H*64+2:  fp32 8.4e-07, split 8.4e-07, bf16 2.8e-03
  test_unaligned_out_split_raises  no kernel: V2AError
  test_mode2_at_rule_limit  CLAMP = 2, NG = 2 of all three kernels at clamp 57, the last integer the rule admits at Nk = 200:
                   fp32 2.2e-07, split 5.4e-06, bf16 4.4e-03 (absolute, against the mean of v)
"""
import contextlib
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -4096.0          # exact in bf16, far outside any output (|o| <= max |v| < 6)
SCALE = 0.125

#         name         B  H  Nq   Nk   kv_len                                q_len
SHAPES = {"base":     (8, 3, 130, 200, [0, 1, 63, 64, 65, 128, 129, 200], [130, 1, 0, 64, 65, 129, 130, 100]),
          "q100k129": (1, 1, 100, 129, [129], [100]),
          "q64k200":  (2, 2, 64, 200, [200, 70], [64, 33]),
          "q70k40":   (2, 2, 70, 40, [40, 17], [70, 5])}
TOL = {"fp32": 2e-5, "split": 2e-4, "bf16": 2e-2}            # tests/test_kernels_gpu.py::test_attention
FORMS = {"default": {}, "one_group": dict(attn_one_group_from=1), "one_group_q64": dict(attn_one_group_from=1, reserved=256)}
FORMS_OF = {"fp32": ["default"], "bf16": ["default", "one_group"], "split": ["default", "one_group", "one_group_q64"]}


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


@contextlib.contextmanager
def _tuning(L, form):
    try:
        if FORMS[form]:
            L.set_tuning(**FORMS[form])
        yield
    finally:
        L.set_tuning()


def _storage(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def _data(name, tdt):
    """q, k, v (B, H, N, 64) and gate (B, H, Nq), fp32 on the CPU, rounded to the storage type tdt."""
    B, H, Nq, Nk, _, _ = SHAPES[name]
    g = torch.Generator().manual_seed(Nq + Nk)
    q = torch.randn(B, H, Nq, 64, generator=g) * 2.0          # |logits| large enough that the tanh clamp bends them
    k = torch.randn(B, H, Nk, 64, generator=g) * 2.0
    v = torch.randn(B, H, Nk, 64, generator=g)
    gate = torch.randn(B, H, Nq, generator=g)
    return tuple(t.to(tdt).float() for t in (q, k, v, gate))


def attn_ref64(q, k, v, gate, kv_len, q_len, scale, clamp):
    """float64 attention of (B, H, N, 64) operands: soft clamp only when clamp > 0, keys >= kv_len[b] masked, sigmoid(gate) or 1,
    rows >= q_len[b] and every row of a batch entry without keys zero."""
    q, k, v = q.double(), k.double(), v.double()
    s = scale * torch.einsum("bhid,bhjd->bhij", q, k)
    if clamp > 0:
        s = clamp * torch.tanh(s / clamp)
    kvl, ql = torch.tensor(kv_len), torch.tensor(q_len)
    km = torch.arange(k.shape[2])[None, :] < kvl[:, None]
    s = s.masked_fill(~km[:, None, None, :], -math.inf)
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))       # a row without keys: all zeros, not NaN
    den = p.sum(-1, keepdim=True)
    o = (p / torch.where(den > 0, den, torch.ones_like(den))) @ v
    if gate is not None:
        o = o * torch.sigmoid(gate.double())[..., None]
    qm = torch.arange(q.shape[2])[None, :] < ql[:, None]
    return o * qm[:, None, :, None] * (kvl > 0)[:, None, None, None]


@functools.lru_cache(maxsize=None)
def _ref(name, tdt, clamp, gated):
    """The float64 reference in the layout of the output buffer, (B, Nq, H * 64).  Shared between tests: never written to."""
    B, H, Nq, _, kv_len, q_len = SHAPES[name]
    q, k, v, gate = _data(name, tdt)
    o = attn_ref64(q, k, v, gate if gated else None, kv_len, q_len, SCALE, clamp)
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * 64).contiguous()


def _launch(L, name, dt, clamp, gated, *, out_split=False, how=None):
    """One v2a_attention launch on buffers packed as the engine packs them: [q | gate | pad] rows of stride H*64+16, [k | v] rows
    of stride 2*H*64, output rows of stride H*64+8 prefilled with SENTINEL (out_split: bf16 rows of 2*H*64).  how: "a" q / gate row
    stride H*64+17, "b" k / v one element past the start of their buffer, "c" output row stride H*64+2.  Returns the output buffer."""
    B, H, Nq, Nk, kv_len, q_len = SHAPES[name]
    tdt = _storage(dt)
    q, k, v, gate = _data(name, tdt)
    inner = H * 64
    qrs = inner + (17 if how == "a" else 16)
    qb = torch.zeros(B, Nq, qrs)
    qb[..., :inner] = q.permute(0, 2, 1, 3).reshape(B, Nq, inner)
    qb[..., inner:inner + H] = gate.permute(0, 2, 1)
    kvb = torch.cat([k.permute(0, 2, 1, 3).reshape(B, Nk, inner), v.permute(0, 2, 1, 3).reshape(B, Nk, inner)], -1)
    off = 1 if how == "b" else 0
    kvflat = torch.zeros(kvb.numel() + 8)
    kvflat[off:off + kvb.numel()] = kvb.reshape(-1)
    qd, kvd = qb.to(DEV, tdt), kvflat.to(DEV, tdt)
    es = qd.element_size()
    ors = 2 * inner if out_split else inner + (2 if how == "c" else 8)
    out = torch.full((B, Nq, ors), SENTINEL, dtype=torch.bfloat16 if out_split else tdt, device=DEV)
    kp = kvd.data_ptr() + off * es
    L.attention(qd.data_ptr(), kp, kp + inner * es, qd.data_ptr() + inner * es if gated else None, out.data_ptr(),
                strides=(qrs, 2 * inner, 2 * inner, qrs if gated else 0, ors,
                         Nq * qrs, Nk * 2 * inner, Nk * 2 * inner, Nq * qrs if gated else 0, Nq * ors),
                B=B, H=H, Nq=Nq, Nk=Nk, kv_len=torch.tensor(kv_len, dtype=torch.int32, device=DEV),
                q_len=torch.tensor(q_len, dtype=torch.int32, device=DEV), scale=SCALE, softclamp=clamp,
                dtype=L.BF16_SPLIT if dt == "split" else L.dt_code(tdt), out_split=out_split)
    torch.cuda.synchronize()
    return out.cpu()


def _written(out, name, width):
    """Pad columns keep the prefill, every column below `width` of every row was written, and all of it is finite."""
    B, H, Nq, _, kv_len, q_len = SHAPES[name]
    assert bool((out[..., width:] == SENTINEL).all()), "a pad column was written"
    got = out[..., :width].float()
    assert bool((got != SENTINEL).all()), "%d output elements were never written" % int((got == SENTINEL).sum())
    assert bool(torch.isfinite(got).all()), "%d non-finite outputs, batch entries %s (kv_len %s)" % (
        int((~torch.isfinite(got)).sum()), sorted(set((~torch.isfinite(got)).nonzero()[:, 0].tolist())), kv_len)
    return got


def _check(out, name, dt, clamp, gated, tol, label):
    B, H, Nq, _, kv_len, q_len = SHAPES[name]
    got = _written(out, name, H * 64).double()
    for b in range(B):      # exact zeros, not zeros within the tolerance
        dead = got[b] if kv_len[b] == 0 else got[b, q_len[b]:]
        assert not dead.numel() or float(dead.abs().max()) == 0.0, "batch entry %d: a row without keys or past q_len is not zero" % b
    ref = _ref(name, _storage(dt), clamp, gated)
    print(f"{label}: {float((got - ref).abs().max() / ref.abs().max()):.2e} of max |ref| (bar {tol:.0e})")
    torch.testing.assert_close(got, ref, atol=tol, rtol=tol)
    return got


# ------------------------------------------------------------------------ the MFMA kernels
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("clamp", [50.0, 80.0, 0.0])
@pytest.mark.parametrize("dt,form", [(dt, f) for dt in ("fp32", "bf16", "split") for f in FORMS_OF[dt]])
def test_base_shape(L, dt, form, clamp, gated):
    """Base shape.  default: attn_mfma_f32_kernel<2, C> / attn_mfma_kernel<2, C> / attn_mfma_split_kernel<2, C, 1> (72 workgroups:
    below 1536 and below 200), with key group 1 empty (kv_len <= 64), holding one tile (129) or a partial last tile (200), and a
    batch entry without keys.  one_group: attn_mfma_kernel<1, C> / attn_mfma_split_kernel<1, C, 2> (three 64-query blocks: the last
    workgroup's second query group is empty).  one_group_q64: attn_mfma_split_kernel<1, C, 1>.  C = 2 (clamp 50), 1 (80), 0 (0)."""
    with _tuning(L, form):
        out = _launch(L, "base", dt, clamp, gated)
    _check(out, "base", dt, clamp, gated, TOL[dt], f"base {dt} {form} clamp {clamp:g} gate {gated}")


@pytest.mark.parametrize("clamp", [50.0, 80.0])
@pytest.mark.parametrize("name,dt,form", [(n, dt, f) for n in ("q100k129", "q64k200", "q70k40") for dt in ("fp32", "bf16", "split")
                                          for f in (FORMS_OF[dt][:2] if n != "q70k40" else ["default"])])
def test_second_shapes(L, name, dt, form, clamp):
    """q100k129 (2 workgroups, key tiles 64 | 64 | 1): default NG = 2 in all three kernels, one_group attn_mfma_kernel<1, C> and
    attn_mfma_split_kernel<1, C, 2> with 36 live rows in the second query group.  q64k200: default NG = 2, one_group
    attn_mfma_kernel<1, C> and attn_mfma_split_kernel<1, C, 1> (Nq <= 64).  q70k40: NG = 1, QG = 1 whatever the tuning (Nk <= 128),
    one partial key tile.  C = 2 (clamp 50), 1 (80).  The split kernel's default at these workgroup counts is NG = 2, so its two
    query-group rules are reached under attn_one_group_from=1."""
    with _tuning(L, form):
        out = _launch(L, name, dt, clamp, True)
    _check(out, name, dt, clamp, True, TOL[dt], f"{name} {dt} {form} clamp {clamp:g}")


@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("clamp", [50.0, 80.0, 0.0])
@pytest.mark.parametrize("dt", ["bf16", "split"])
def test_two_forms_agree(L, dt, clamp, gated):
    """Base shape, one kernel in its forms against each other: attn_mfma_kernel<2, C> against <1, C> under the bf16 bar,
    attn_mfma_split_kernel<2, C, 1> against <1, C, 2> and <1, C, 1> under the split bar (the merge reorders sums: not bitwise)."""
    H = SHAPES["base"][1]
    got = {}
    for form in FORMS_OF[dt]:
        with _tuning(L, form):
            got[form] = _written(_launch(L, "base", dt, clamp, gated), "base", H * 64)
    for form in FORMS_OF[dt][1:]:
        err = float((got[form] - got["default"]).abs().max() / got["default"].abs().max())
        print(f"forms {dt} clamp {clamp:g} gate {gated}: default vs {form} {err:.2e} of max |o| (bar {TOL[dt]:.0e})")
        torch.testing.assert_close(got[form], got["default"], atol=TOL[dt], rtol=TOL[dt])


@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("clamp", [50.0, 80.0, 0.0])
@pytest.mark.parametrize("form", FORMS_OF["split"])
def test_out_split_planes_exact(L, form, clamp, gated):
    """attn_mfma_split_kernel<2, C, 1>, <1, C, 2>, <1, C, 1> with out_split (bf16 rows of 2*H*64: hi | lo planes): the dispatch does
    not look at out_split, so the planes are hi = bf16(o), lo = bf16(o - hi) of the same instantiation's fp32 output, bit for bit."""
    inner = SHAPES["base"][1] * 64
    with _tuning(L, form):
        o = _written(_launch(L, "base", "split", clamp, gated), "base", inner)
        planes = _written(_launch(L, "base", "split", clamp, gated, out_split=True), "base", 2 * inner)
    hi, lo = planes[..., :inner].bfloat16(), planes[..., inner:].bfloat16()
    assert torch.equal(hi, o.bfloat16())
    assert torch.equal(lo, (o - hi.float()).bfloat16())


# ------------------------------------------------------------------- the unaligned fallback
@pytest.mark.parametrize("how", ["a", "b", "c"])
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("clamp", [50.0, 0.0])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "split"])
@pytest.mark.parametrize("name", ["base", "q70k40"])
def test_unaligned_fallback(L, name, dt, clamp, gated, how):
    """attn_rowlane_kernel<float> (fp32; BF16_SPLIT tensors are fp32 and take it too) and attn_rowlane_kernel<bf16_t>: exact-fp32
    arithmetic in another order, held to the fp32 and bf16 bars.  how: (a) q / gate row stride H*64+17, (b) k / v one element
    past an aligned address, (c) output row stride H*64+2 (not a multiple of 4).  Key tiles of 32: 200 keys end inside the
    seventh, 40 inside the second; kv_len 0 never enters the key loop."""
    out = _launch(L, name, dt, clamp, gated, how=how)
    _check(out, name, dt, clamp, gated, TOL["bf16" if dt == "bf16" else "fp32"], f"rowlane {name} {dt} ({how}) clamp {clamp:g} gate {gated}")


@pytest.mark.parametrize("how", ["a", "b"])
def test_unaligned_out_split_raises(L, how):
    """The fallback cannot write hi | lo planes: out_split with unaligned operands is an error, not a launch."""
    with pytest.raises(L.V2AError, match="out_split needs"):
        _launch(L, "q70k40", "split", 50.0, True, out_split=True, how=how)


# ----------------------------------------------------------- mode 2 at the edge of its rule
def _clamp_mode(clamp, Nk):
    """attn_clamp_mode of csrc/attn_core.h."""
    if not clamp > 0:
        return 0
    return 2 if clamp * math.log2(math.e) + math.log2(max(Nk, 1)) <= 90.0 else 1


@pytest.mark.parametrize("dt", ["fp32", "bf16", "split"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_mode2_at_rule_limit(L, dt, sign):
    """CLAMP = 2, NG = 2 of all three kernels (8 workgroups) at the largest integer clamp the rule admits for 200 keys, 57
    (57 log2 e + log2 200 = 89.9): every logit at +-clamp as in test_attention_saturated_logits, |v| <= 8, so the fp32 sums hold
    200 * 8 * 2^(+-82.2).  All weights are equal: the output is the mean of v, finite."""
    B, H, N = 1, 2, 200
    c = max(i for i in range(1, 200) if _clamp_mode(float(i), N) == 2)
    assert c == 57 and _clamp_mode(float(c + 1), N) == 1
    tdt = _storage(dt)
    inner = H * 64
    q = torch.full((B, N, inner + 16), 12.0)
    q[..., inner:] = 20.0                                   # gate: sigmoid(20) == 1 in fp32
    kv = torch.full((B, N, 2 * inner), sign * 24.0)         # 64 * 12 * 24 * 0.125 = 2304 >> 57
    kv[..., inner:] = (torch.rand(B, N, inner, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 8.0
    qd, kvd = q.to(DEV, tdt), kv.to(DEV, tdt)
    out = torch.full((B, N, inner), float("nan"), dtype=tdt, device=DEV)
    es = qd.element_size()
    L.attention(qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + inner * es, qd.data_ptr() + inner * es, out.data_ptr(),
                strides=(inner + 16, 2 * inner, 2 * inner, inner + 16, inner, N * (inner + 16), N * 2 * inner, N * 2 * inner,
                         N * (inner + 16), N * inner),
                B=B, H=H, Nq=N, Nk=N, scale=SCALE, softclamp=float(c), dtype=L.BF16_SPLIT if dt == "split" else L.dt_code(tdt))
    got = out.float().cpu().double()
    ref = kvd[..., inner:].cpu().double().mean(1, keepdim=True).expand(B, N, inner)
    assert bool(torch.isfinite(got).all())
    print(f"mode 2 at clamp {c} {dt} sign {sign:+g}: {float((got - ref).abs().max()):.2e} (absolute)")
    torch.testing.assert_close(got, ref, atol=2e-2 if dt == "bf16" else 1e-4, rtol=0)
