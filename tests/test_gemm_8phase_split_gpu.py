"""GPU: the 256x256 8-phase kernel on split (hi | lo plane) operands -- stages of 32 logical k, each LDS row [32 k hi | 32 k lo], three MFMA
products per stage from one set of fragments (csrc/gemm_8phase.hip, SPLIT) -- on what tests/test_kernels_gpu.py::test_gemm_split_native
does not reach: the shortest K loops the host admits (logical K = 64 = two stages: one trip with nothing left to prefetch; 192 and 320 = 6 and 10
stages), three segments whose hi -> lo plane distances differ, row tiles with skipped padding bands (M = 1564, M = 28), a 16-column last tile
(N = 3088), the one-clip production shapes of the sampler, and a split shadow written at a plane offset by this kernel.

Bars: those of test_gemm_split_native -- 3e-5 (GEGLU: 4e-5) of the largest reference value against the fp64 product (three bf16 MFMA products
per fp32 product leave ~1e-5 relative) -- and bit equality where two launches must sum in the same order."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HINT_8PHASE = 5


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


def _split_planes(x):
    """fp32 (rows, k) -> bf16 (rows, 2k) = [hi | lo] (the V2A_BF16_SPLIT layout)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, lo], -1).contiguous()


def _rope_table(n):
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(n).float()[:, None] * inv[None, :]
    return torch.stack((ang.cos(), ang.sin()), -1).contiguous()


def _rope_ref(z, tab, rope_cols, rows_per_batch):
    """fp64: interleaved pairs (2i, 2i + 1) of every 64-column head of the first rope_cols columns rotated by the table row of the position."""
    M = z.shape[0]
    pos = torch.arange(M) % rows_per_batch
    cos, sin = tab[pos, :, 0].double(), tab[pos, :, 1].double()              # (M, 32)
    x = z[:, :rope_cols].reshape(M, rope_cols // 64, 32, 2)
    even = x[..., 0] * cos[:, None] - x[..., 1] * sin[:, None]
    odd = x[..., 1] * cos[:, None] + x[..., 0] * sin[:, None]
    out = z.clone()
    out[:, :rope_cols] = torch.stack((even, odd), -1).reshape(M, rope_cols)
    return out


def _operands(M, N, ks, seed):
    g = _g(seed)
    a = [torch.randn(M, k, generator=g) for k in ks]
    K = sum(ks)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = 0.1 * torch.randn(N, generator=g)
    acc = torch.cat(a, 1).double() @ w.double().t()
    return g, a, w, bias, acc


@pytest.mark.parametrize("epi", ["store", "resid_shadow"])
@pytest.mark.parametrize("M,N,K", [(28, 512, 64), (1564, 512, 64), (300, 3088, 64), (1564, 3088, 192), (28, 1024, 192), (1564, 1024, 320),
                                   (300, 272, 320)])
def test_short_k_loops_and_edge_tiles(L, epi, M, N, K):
    """Logical K = 64 / 192 / 320 = 2 / 6 / 10 stages (prologue + one trip; odd and even numbers of buffer pairs), M = 28 and 1564 (row bands
    behind the last row are not multiplied), N = 3088 and 272 (16-column last tile).  Against fp64."""
    g, a, w, bias, acc = _operands(M, N, (K,), 7 * M + N + K)
    segs = [(_split_planes(a[0]).to(DEV), 2 * K, K)]
    wd = _split_planes(w).to(DEV)
    kw = dict(M=M, N=N, compute=L.BF16, a_split=True, tile_hint=HINT_8PHASE)
    scale = max(float(acc.abs().max()), 1.0)
    if epi == "store":
        out = torch.empty(M, N, device=DEV)
        L.gemm(segs, wd, out, bias=bias.to(DEV), **kw)
        err = float((out.cpu().double() - (acc + bias.double())).abs().max())
        print("K=%d M=%d N=%d store: err %.3g (bar %.3g)" % (K, M, N, err, 3e-5 * scale))
        assert err < 3e-5 * scale, err
    else:
        res = torch.randn(M, N, generator=g)
        out, sh = torch.empty(M, N, device=DEV), torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
        L.gemm(segs, wd, out, epilogue=L.EPI_RESID, resid=res.to(DEV), out_bf16=sh, ld_out_bf16=2 * N, out_bf16_split=True, **kw)
        err = float((out.cpu().double() - (res.double() + acc)).abs().max())
        print("K=%d M=%d N=%d resid: err %.3g (bar %.3g)" % (K, M, N, err, 3e-5 * scale))
        assert err < 3e-5 * scale, err
        assert torch.equal(sh.cpu(), _split_planes(out.cpu()))


@pytest.mark.parametrize("M", [1564, 28])
def test_three_segments_with_different_plane_distances(L, M):
    """Three logical segments whose lo planes lie at different distances behind their hi planes: the two halves of one [x_hi | s_hi | x_lo | s_lo]
    buffer (K = d each, lo plane 2d further) and a standard segment (K = 3d / 2, lo plane 3d / 2 further), with different row strides.  Against
    fp64, and bit-equal to the same product on three separately laid out standard segments (stages follow k order across segment ends)."""
    d, N = 128, 1024
    ks = (d, d, 3 * d // 2)
    g, a, w, bias, acc = _operands(M, N, ks, 900 + M)
    xs, ss, ts = (_split_planes(x) for x in a)
    wide = torch.cat([xs[:, :d], ss[:, :d], xs[:, d:], ss[:, d:]], 1).contiguous().to(DEV)
    wd = _split_planes(w).to(DEV)
    kw = dict(M=M, N=N, compute=L.BF16, a_split=True, tile_hint=HINT_8PHASE, bias=bias.to(DEV))
    got, ref = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    L.gemm([(wide, 4 * d, d, 2 * d), (wide[:, d:], 4 * d, d, 2 * d), (ts.to(DEV), 2 * ks[2], ks[2])], wd, got, **kw)
    L.gemm([(xs.to(DEV), 2 * d, d), (ss.to(DEV), 2 * d, d), (ts.to(DEV), 2 * ks[2], ks[2])], wd, ref, **kw)
    scale = max(float(acc.abs().max()), 1.0)
    err = float((got.cpu().double() - (acc + bias.double())).abs().max())
    print("M=%d three segments: err %.3g (bar %.3g)" % (M, err, 3e-5 * scale))
    assert err < 3e-5 * scale, err
    assert torch.equal(got, ref)


def test_production_geglu_one_clip(L):
    """Audio feed-forward-in at one clip: 1564 x 8192 x 1024, GEGLU with split (hi | lo) output.  Against fp64 (erf GELU)."""
    M, N, K = 1564, 8192, 1024
    g, a, w, bias, acc = _operands(M, N, (K,), 31)
    half = N // 2
    perm = torch.cat([torch.cat([torch.arange(j * 16, j * 16 + 16), half + torch.arange(j * 16, j * 16 + 16)]) for j in range(half // 16)])
    wp, bp = w[perm], bias[perm]                   # W rows regrouped [16 value | 16 gate]
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm([(_split_planes(a[0]).to(DEV), 2 * K, K)], _split_planes(wp).to(DEV), out, M=M, N=N, compute=L.BF16, a_split=True,
           tile_hint=HINT_8PHASE, epilogue=L.EPI_GEGLU, bias=bp.to(DEV), ldo=N, out_split=True)
    z = acc + bias.double()
    ref = z[:, :half] * torch.nn.functional.gelu(z[:, half:])
    got = out[:, :half].float().cpu().double() + out[:, half:].float().cpu().double()
    err, bar = float((got - ref).abs().max()), 4e-5 * max(float(ref.abs().max()), 1.0)
    print("GEGLU 1564x8192x1024: err %.3g (bar %.3g)" % (err, bar))
    assert err < bar, err


@pytest.mark.parametrize("hint", [HINT_8PHASE, 0])
def test_production_qkv_rope_one_clip(L, hint):
    """Audio QKV + gate projection at one clip: 1564 x 3088 x 1024, fp32 STORE with RoPE fused over the q and k heads (2048 columns), two
    sequences of 782 rows.  Against the fp64 product rotated in fp64 by the same table."""
    M, N, K, rpb, rope_cols = 1564, 3088, 1024, 782, 2048
    g, a, w, bias, acc = _operands(M, N, (K,), 32)
    tab = _rope_table(rpb)
    out = torch.empty(M, N, device=DEV)
    L.gemm([(_split_planes(a[0]).to(DEV), 2 * K, K)], _split_planes(w).to(DEV), out, M=M, N=N, compute=L.BF16, a_split=True, tile_hint=hint,
           bias=bias.to(DEV), rope_table=tab.to(DEV), rope_cols=rope_cols, rope_pos_offset=0, rows_per_batch=rpb)
    ref = _rope_ref(acc + bias.double(), tab, rope_cols, rpb)
    err, bar = float((out.cpu().double() - ref).abs().max()), 3e-5 * max(float(acc.abs().max()), 1.0)
    print("QKV + RoPE 1564x3088x1024 hint %d: err %.3g (bar %.3g)" % (hint, err, bar))
    assert err < bar, err


@pytest.mark.parametrize("epi", ["resid", "gate_norm"])
@pytest.mark.parametrize("M,N", [(1564, 512), (1600, 1024)])
def test_split_shadow_at_plane_offset(L, M, N, epi):
    """A split shadow written by the 8-phase kernel (tile_hint 5) into one half of a [. | s_hi | . | s_lo] buffer through
    out_bf16_lo_offset: equal plane by plane to the standard [hi | lo] shadow of the same launch, the other half untouched.  With the residual
    epilogue, and with the gated residual as a folded-norm producer (shadow = planes of out * gamma)."""
    K = 256
    g, a, w, bias, acc = _operands(M, N, (K,), 40 + N)
    seg = [(_split_planes(a[0]).to(DEV), 2 * K, K)]
    wd = _split_planes(w).to(DEV)
    res = torch.randn(M, N, generator=g)
    sh = torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    wide = torch.zeros(M, 4 * N, dtype=torch.bfloat16, device=DEV)
    kw = dict(M=M, N=N, compute=L.BF16, a_split=True, out_bf16_split=True, tile_hint=HINT_8PHASE)
    if epi == "resid":
        o1, o2 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        kw.update(epilogue=L.EPI_RESID, resid=res.to(DEV))
        L.gemm(seg, wd, o1, out_bf16=sh, ld_out_bf16=2 * N, **kw)
        L.gemm(seg, wd, o2, out_bf16=wide[:, N:], ld_out_bf16=4 * N, out_bf16_lo_offset=2 * N, **kw)
        ref, shadow_of = res.double() + acc, o1.cpu()
    else:
        gate, gam = torch.rand(N, generator=g), 1 + 0.2 * torch.randn(N, generator=g)
        o1, o2 = res.clone().to(DEV), res.clone().to(DEV)
        ssq1, ssq2 = torch.zeros(M, N // 32, device=DEV), torch.zeros(M, N // 32, device=DEV)
        kw.update(epilogue=L.EPI_GATE_RESID, gate=gate.to(DEV), bias=bias.to(DEV), norm_gamma=gam.to(DEV))
        L.gemm(seg, wd, o1, resid=o1, out_bf16=sh, ld_out_bf16=2 * N, norm_ssq=ssq1, **kw)
        L.gemm(seg, wd, o2, resid=o2, out_bf16=wide[:, N:], ld_out_bf16=4 * N, out_bf16_lo_offset=2 * N, norm_ssq=ssq2, **kw)
        ref, shadow_of = res.double() + gate.double() * (acc + bias.double()), o1.cpu() * gam
        assert torch.equal(ssq1, ssq2)
    scale = max(float(acc.abs().max()), 1.0)
    assert float((o1.cpu().double() - ref).abs().max()) < 3e-5 * scale
    assert torch.equal(o1, o2)
    assert torch.equal(sh.cpu(), _split_planes(shadow_of))
    assert torch.equal(wide[:, N:2 * N], sh[:, :N]) and torch.equal(wide[:, 3 * N:], sh[:, N:])
    assert float(wide[:, :N].abs().max()) == 0 and float(wide[:, 2 * N:3 * N].abs().max()) == 0
