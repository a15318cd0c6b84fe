"""GPU parity, kernel by kernel, through the C ABI (v2a_amd._lib -> libv2a_cfm.so), against the
CPU oracle on seeded inputs and against tests/golden/blocks_small.npz.
Tolerances: fp32 kernels 1e-5 abs on O(1) values (fp32 summation-order noise only);
bf16 kernels are checked against the oracle run on bf16-rounded operands (tolerance in each test)."""
import math

import numpy as np
import pytest
import torch

from oracle import e2_cfm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("d", [64, 192, 512, 1024, 1280])
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
def test_rmsnorm_plain(L, d, odt):
    rows = 37
    x = torch.randn(rows, d, generator=_g(d))
    g = 1 + 0.1 * torch.randn(d, generator=_g(d + 1))
    ref = O.rmsnorm(x, g)
    y = torch.empty(rows, d, dtype=odt, device=DEV)
    L.rmsnorm(x.to(DEV), y, rows=rows, d=d, gamma=g.to(DEV))
    tol = 1e-5 if odt == torch.float32 else 2e-2
    torch.testing.assert_close(y.float().cpu(), ref, atol=tol, rtol=tol)


def test_rmsnorm_zero_row_and_step_vector(L):
    """eps path of F.normalize (all-zero row -> 0) and the step/batch-indexed gamma table."""
    B, N, d, S = 2, 5, 128, 3
    x = torch.randn(B * N, d, generator=_g(3))
    x[4] = 0
    tab = torch.randn(S, B, d, generator=_g(4))
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    y = torch.empty(B * N, d, device=DEV)
    L.rmsnorm(x.to(DEV), y, rows=B * N, d=d, gamma=tab.to(DEV), step=step, gamma_step_stride=B * d,
              gamma_batch_stride=d, rows_per_batch=N)
    ref = torch.cat([O.rmsnorm(x[b * N:(b + 1) * N], tab[2, b]) for b in range(B)])
    torch.testing.assert_close(y.cpu(), ref, atol=1e-5, rtol=1e-5)
    assert float(y[4].abs().max()) == 0.0


def test_adaptive_rmsnorm_golden(L, small, golden):
    b = golden["blocks_small"]
    P = small["P"]
    x, c = torch.from_numpy(b["x"]), torch.from_numpy(b["c"])
    gamma = torch.nn.functional.linear(c, P["transformer.layers.0.0.2.to_gamma.weight"]) + 1.0     # (2, 128)
    y = torch.empty(2 * 44, 128, device=DEV)
    L.rmsnorm(x.reshape(-1, 128).to(DEV), y, rows=88, d=128, gamma=gamma.to(DEV), gamma_batch_stride=128, rows_per_batch=44)
    np.testing.assert_allclose(y.cpu().numpy().reshape(2, 44, 128), b["ada_rmsnorm"], atol=1e-5)


# -------------------------------------------------------------------------------- dwconv
@pytest.mark.parametrize("tn", [4, 6])
@pytest.mark.parametrize("N,d,lens", [(44, 128, [44, 30]), (782, 512, None), (7, 64, [7, 3]), (100, 1280, [100, 33]), (782, 1024, [782, 1])])
def test_dwconv(L, N, d, lens, tn):
    """All position-tile sizes of the kernel (4 / 6 outputs per wave pass); edge tiles, masked tails, a 1-frame clip."""
    B = 2
    x = torch.randn(B, N, d, generator=_g(N))
    w = torch.randn(d, 1, 31, generator=_g(N + 1)) / math.sqrt(31)
    bias = 0.1 * torch.randn(d, generator=_g(N + 2))
    mask = None if lens is None else O.lens_to_mask(torch.tensor(lens), N)
    ref = O.depthwise_conv(x, w, bias, mask) + x
    out = torch.empty(B, N, d, device=DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    L.set_tuning(dwconv_rows_per_wave=tn)
    try:
        L.dwconv(x.to(DEV), out, w[:, 0, :].t().contiguous().to(DEV), bias.to(DEV), B=B, N=N, d=d, ksize=31, lens=ld)
    finally:
        L.set_tuning()
    torch.testing.assert_close(out.cpu(), ref, atol=2e-5, rtol=1e-5)


def test_dwconv_golden(L, small, golden):
    b, P = golden["blocks_small"], small["P"]
    x = torch.from_numpy(b["x"])
    w, bias = P["transformer.layers.0.0.1.dw_conv1d.0.weight"], P["transformer.layers.0.0.1.dw_conv1d.0.bias"]
    out = torch.empty(2, 44, 128, device=DEV)
    L.dwconv(x.to(DEV), out, w[:, 0, :].t().contiguous().to(DEV), bias.to(DEV), B=2, N=44, d=128, ksize=31,
             lens=torch.tensor([44, 30], dtype=torch.int32, device=DEV))
    np.testing.assert_allclose((out.cpu() - x).numpy(), b["dwconv"], atol=2e-5)


# ---------------------------------------------------------------------------------- rope
def _rope_table(n):
    inv = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(n).float()[:, None] * inv[None, :]
    return torch.stack((ang.cos(), ang.sin()), -1).contiguous()


@pytest.mark.parametrize("layout", ["interleaved", "half"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rope(L, golden, layout, dt):
    b = golden["blocks_small"]
    q = torch.from_numpy(b["rope_in"])                        # (1, 2, 44, 64)
    rows = q.permute(0, 2, 1, 3).reshape(44, 128).contiguous()
    pad = torch.zeros(44, 144)
    pad[:, :128] = rows
    buf = pad.to(DEV, dt)
    L.rope(buf, rows=44, row_stride=144, nheads=2, rows_per_batch=44, pos_offset=0, table=_rope_table(44).to(DEV),
           layout={"interleaved": 0, "half": 1}[layout])
    got = buf.float().cpu()[:, :128].reshape(1, 44, 2, 64).permute(0, 2, 1, 3)
    if dt == torch.float32:
        np.testing.assert_allclose(got.numpy(), b[f"rope_{layout}"], atol=1e-5)
    else:
        ref = O.apply_rope(q.bfloat16().float(), O.rotary_freqs(44, 64, layout), layout)
        torch.testing.assert_close(got, ref, atol=3e-2, rtol=2e-2)
    assert float(buf[:, 128:].abs().max()) == 0.0              # columns beyond the heads untouched


def test_rope_last_rows_offset(L, golden):
    """A7: cross-attention keys take the LAST nc rows of the table."""
    b = golden["blocks_small"]
    q = torch.from_numpy(b["rope_in"])[:, :, :5]               # 5 keys
    rows = q.permute(0, 2, 1, 3).reshape(5, 128).contiguous().to(DEV)
    L.rope(rows, rows=5, row_stride=128, nheads=2, rows_per_batch=5, pos_offset=44 - 5, table=_rope_table(44).to(DEV), layout=0)
    got = rows.cpu().reshape(1, 5, 2, 64).permute(0, 2, 1, 3)
    np.testing.assert_allclose(got.numpy(), b["rope_last5_interleaved"], atol=1e-5)


# ---------------------------------------------------------------------------------- gemm
def _gemm_ref(a, w, bias):
    out = a.double() @ w.double().t()
    if bias is not None:
        out = out + bias.double()
    return out


@pytest.mark.parametrize("M,N,K", [(200, 144, 64), (1564, 272, 128), (31, 1024, 192), (130, 16, 1024)])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gemm_store(L, M, N, K, mode):
    a = torch.randn(M, K, generator=_g(M))
    w = torch.randn(N, K, generator=_g(N)) / math.sqrt(K)
    bias = torch.randn(N, generator=_g(K))
    if mode == "fp32":
        out = torch.empty(M, N, device=DEV)
        L.gemm([(a.to(DEV), K, K)], w.to(DEV), out, M=M, N=N, compute=L.F32, bias=bias.to(DEV))
        torch.testing.assert_close(out.cpu().double(), _gemm_ref(a, w, bias), atol=2e-5, rtol=1e-5)
    else:
        ab, wb = a.bfloat16(), w.bfloat16()
        ref = _gemm_ref(ab.float(), wb.float(), bias)
        for odt in (torch.float32, torch.bfloat16):
            out = torch.empty(M, N, dtype=odt, device=DEV)
            L.gemm([(ab.to(DEV), K, K)], wb.to(DEV), out, M=M, N=N, compute=L.BF16, bias=bias.to(DEV))
            tol = 1e-4 if odt == torch.float32 else 2e-2       # fp32 accumulate of exact bf16 products
            torch.testing.assert_close(out.cpu().double(), ref, atol=tol, rtol=tol)
        # fp32 A converted on load must equal pre-rounded bf16 A
        out2 = torch.empty(M, N, device=DEV)
        L.gemm([(a.to(DEV), K, K)], wb.to(DEV), out2, M=M, N=N, compute=L.BF16, bias=bias.to(DEV))
        torch.testing.assert_close(out2.cpu().double(), ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("M,N,K,epi", [(1564, 2048, 192, "store"), (1564, 10240, 192, "geglu"), (4200, 1024, 320, "resid"),
                                       (1564, 5120, 128, "gate_resid"), (3300, 2304, 64, "store"),
                                       (8200, 4096, 192, "store"), (8200, 4096, 128, "geglu"), (8300, 4096, 64, "gate_resid")])
def test_gemm_big_tile_persistent_configs(L, M, N, K, epi):
    """Shapes that select the 256x256 (2-deep ring), 128x256 (8-wave) and 128x128 tiles of the LDS-DMA kernel, including
    partial edge tiles, single- and multi-tile K loops and every fused epilogue."""
    g = _g(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    bias = 0.1 * torch.randn(N, generator=g)
    acc = a.float().double() @ w.float().double().t()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    if epi == "store":
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        L.gemm([(ad, K, K)], wd, out, M=M, N=N, compute=L.BF16, bias=bd)
        torch.testing.assert_close(out.float().cpu().double(), acc + bias.double(), atol=2e-2, rtol=2e-2)
    elif epi == "geglu":
        # value / gate rows are taken in the packed [16 | 16] order
        h = (acc + bias.double()).reshape(M, N // 32, 2, 16)
        ref = (h[:, :, 0] * torch.nn.functional.gelu(h[:, :, 1])).reshape(M, N // 2)
        out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV)
        L.gemm([(ad, K, K)], wd, out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_GEGLU, bias=bd, ldo=N // 2)
        torch.testing.assert_close(out.float().cpu().double(), ref, atol=2e-2, rtol=2e-2)
    elif epi == "resid":
        # two K segments (192 + 128) as in the U-Net skip GEMM, fp32 out + bf16 shadow
        a2 = torch.randn(M, 128, generator=g).bfloat16()
        w2 = (torch.randn(N, 128, generator=g) / math.sqrt(K)).bfloat16()
        wcat = torch.cat([w, w2], 1).contiguous()
        resid = torch.randn(M, N, generator=g)
        ref = resid.double() + acc + a2.float().double() @ w2.float().double().t() + bias.double()
        out = torch.empty(M, N, device=DEV)
        sh = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        L.gemm([(ad, K, K), (a2.to(DEV), 128, 128)], wcat.to(DEV), out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID,
               bias=bd, resid=resid.to(DEV), out_bf16=sh)
        torch.testing.assert_close(out.cpu().double(), ref, atol=2e-4, rtol=1e-4)
        assert torch.equal(sh.cpu(), out.cpu().bfloat16())
    else:
        resid = torch.randn(M, N, generator=g)
        gate = torch.rand(2, N, generator=g)
        step = torch.tensor([1], dtype=torch.int32, device=DEV)
        ref = resid.double() + gate[1].double() * (acc + bias.double())
        out = resid.to(DEV)
        L.gemm([(ad, K, K)], wd, out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_GATE_RESID, bias=bd, resid=out,
               gate=gate.to(DEV), step=step, gate_step_stride=N, rows_per_batch=782)
        torch.testing.assert_close(out.cpu().double(), ref, atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("M,N,ks,epi", [(1564, 3088, (1024,), "store_rope"), (1564, 8192, (1024,), "geglu"), (300, 512, (64,), "store"),
                                        (1564, 1024, (1024, 1280, 512), "resid"), (782, 1280, (128, 64), "gate_resid"),
                                        (2600, 768, (192,), "store_f32"), (257, 272, (320,), "resid")])
def test_gemm_8phase_kernel(L, M, N, ks, epi, stagger):
    """The 256x256 phase-interleaved kernel (gemm_8phase.hip) forced for every shape: partial edge tiles in M and N, K loops
    of 1, 2, 3 and many tiles, K-concatenated segments with different row strides, every fused epilogue, both wave-row
    schedules (staggered / lock-step).  Checked against fp64 products of the bf16-rounded operands."""
    K = sum(ks)
    g = _g(M + N + K)
    segs = [torch.randn(M, k, generator=g).bfloat16() for k in ks]
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    bias = 0.1 * torch.randn(N, generator=g)
    acc = torch.cat(segs, 1).float().double() @ w.float().double().t() + bias.double()
    sd = [(t.to(DEV), t.shape[1], t.shape[1]) for t in segs]
    wd, bd = w.to(DEV), bias.to(DEV)
    L.set_tuning(force_tile=6, eight_phase=stagger)
    try:
        if epi == "store":
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, bias=bd)
            torch.testing.assert_close(out.float().cpu().double(), acc, atol=2e-2, rtol=2e-2)
        elif epi == "store_f32":
            out = torch.empty(M, N, device=DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, bias=bd)
            torch.testing.assert_close(out.cpu().double(), acc, atol=1e-4, rtol=1e-4)
        elif epi == "store_rope":
            rpb = 782
            tab = _rope_table(rpb).to(DEV)
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, bias=bd, rope_table=tab, rope_cols=2048, rope_pos_offset=0, rows_per_batch=rpb)
            q = acc[:, :2048].float().reshape(M // rpb, rpb, 32, 64).permute(0, 2, 1, 3)
            fr = O.rotary_freqs(rpb, 64, "interleaved")
            ref = acc.clone().float()
            ref[:, :2048] = O.apply_rope(q, fr, "interleaved").permute(0, 2, 1, 3).reshape(M, 2048)
            torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=2e-2)
        elif epi == "geglu":
            h = acc.reshape(M, N // 32, 2, 16)
            ref = (h[:, :, 0] * torch.nn.functional.gelu(h[:, :, 1])).reshape(M, N // 2)
            out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_GEGLU, bias=bd, ldo=N // 2)
            torch.testing.assert_close(out.float().cpu().double(), ref, atol=2e-2, rtol=2e-2)
        elif epi == "resid":
            resid = torch.randn(M, N, generator=g)
            out = torch.empty(M, N, device=DEV)
            sh = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID, bias=bd, resid=resid.to(DEV), out_bf16=sh)
            torch.testing.assert_close(out.cpu().double(), resid.double() + acc, atol=2e-4, rtol=1e-4)
            assert torch.equal(sh.cpu(), out.cpu().bfloat16())
        else:
            resid = torch.randn(M, N, generator=g)
            gate = torch.rand(2, N, generator=g)
            step = torch.tensor([1], dtype=torch.int32, device=DEV)
            out = resid.to(DEV)
            L.gemm(sd, wd, out, M=M, N=N, compute=L.BF16, epilogue=L.EPI_GATE_RESID, bias=bd, resid=out, gate=gate.to(DEV),
                   step=step, gate_step_stride=N, rows_per_batch=391)
            torch.testing.assert_close(out.cpu().double(), resid.double() + gate[1].double() * acc, atol=2e-4, rtol=1e-4)
    finally:
        L.set_tuning()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gemm_three_segments_resid(L, mode):
    """concat-free TextAudioCrossCondition: W [N][Ka+Kb+Kc] against three fp32 row-major streams."""
    M, N, ks = 150, 128, (128, 192, 64)
    segs = [torch.randn(M, k, generator=_g(k)) for k in ks]
    w = torch.randn(N, sum(ks), generator=_g(5)) / math.sqrt(sum(ks))
    resid = torch.randn(M, N, generator=_g(6))
    cat = torch.cat(segs, -1)
    cd, comp, tol = (torch.float32, L.F32, 2e-5) if mode == "fp32" else (torch.bfloat16, L.BF16, 1e-4)
    if mode == "bf16":
        cat, w = cat.bfloat16().float(), w.bfloat16().float()
    ref = resid.double() + cat.double() @ w.double().t()
    out = torch.empty(M, N, device=DEV)
    L.gemm([(s.to(DEV), s.shape[1], s.shape[1]) for s in segs], w.to(DEV, cd), out, M=M, N=N, compute=comp,
           epilogue=L.EPI_RESID, resid=resid.to(DEV))
    torch.testing.assert_close(out.cpu().double(), ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gemm_geglu(L, mode):
    """A8 with the [16 value | 16 gate] row packing of dit._FF."""
    from v2a_amd.dit import _FF
    M, d = 100, 128
    sd = {"ff.ff.0.proj.weight": torch.randn(8 * d, d, generator=_g(1)) / math.sqrt(d), "ff.ff.0.proj.bias": 0.1 * torch.randn(8 * d, generator=_g(2)),
          "ff.ff.2.weight": torch.randn(d, 4 * d, generator=_g(3)) / math.sqrt(4 * d), "ff.ff.2.bias": 0.1 * torch.randn(d, generator=_g(4))}
    cd, comp = (torch.float32, L.F32) if mode == "fp32" else (torch.bfloat16, L.BF16)
    F = _FF(sd, "ff", d, cd, DEV)
    x = torch.randn(M, d, generator=_g(5))
    xq = x.to(cd).float()
    w1 = sd["ff.ff.0.proj.weight"].to(cd).float()
    h = torch.nn.functional.linear(xq, w1, sd["ff.ff.0.proj.bias"])
    a, g = h.chunk(2, -1)
    ref = a * torch.nn.functional.gelu(g)
    out = torch.empty(M, 4 * d, dtype=cd, device=DEV)
    L.gemm([(x.to(DEV, cd), d, d)], F.w1, out, M=M, N=8 * d, compute=comp, epilogue=L.EPI_GEGLU, bias=F.b1, ldo=4 * d)
    tol = 2e-5 if mode == "fp32" else 2e-2
    torch.testing.assert_close(out.float().cpu(), ref, atol=tol, rtol=tol)


def test_gemm_gate_resid_and_sigmoid(L):
    """AdaLNZero: table = sigmoid(W c + b) (SIGMOID epilogue), then x + gate * (acc + bias) indexed by a device step."""
    S, d, M, N, K, rpb = 3, 128, 90, 128, 64, 45
    c = torch.randn(S, d, generator=_g(1))
    wg, bg = torch.randn(N, d, generator=_g(2)) / math.sqrt(d), torch.randn(N, generator=_g(3))
    tab = torch.empty(S, N, device=DEV)
    L.gemm([(c.to(DEV), d, d)], wg.to(DEV), tab, M=S, N=N, compute=L.F32, epilogue=L.EPI_SIGMOID, bias=bg.to(DEV))
    tab_ref = torch.sigmoid(torch.nn.functional.linear(c, wg, bg))
    torch.testing.assert_close(tab.cpu(), tab_ref, atol=1e-5, rtol=1e-5)
    a, w = torch.randn(M, K, generator=_g(4)), torch.randn(N, K, generator=_g(5)) / math.sqrt(K)
    bias, x = torch.randn(N, generator=_g(6)), torch.randn(M, N, generator=_g(7))
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    L.gemm([(a.to(DEV), K, K)], w.to(DEV), xd, M=M, N=N, compute=L.F32, epilogue=L.EPI_GATE_RESID, bias=bias.to(DEV),
           resid=xd, gate=tab, step=step, gate_step_stride=N, rows_per_batch=rpb)
    ref = x + tab_ref[1] * torch.nn.functional.linear(a, w, bias)
    torch.testing.assert_close(xd.cpu(), ref, atol=2e-5, rtol=1e-5)


def test_gemm_rejects_bad_args(L):
    a = torch.zeros(4, 40, device=DEV)
    w = torch.zeros(16, 40, device=DEV)
    out = torch.zeros(4, 16, device=DEV)
    with pytest.raises(L.V2AError, match="not a multiple"):
        L.gemm([(a, 40, 40)], w, out, M=4, N=16, compute=L.F32)


@pytest.mark.parametrize("B,N,d,ragged", [(16, 782, 1024, False), (16, 782, 1280, True), (16, 782, 512, True), (12, 300, 1024, True), (40, 1500, 96, True)])
@pytest.mark.parametrize("norm", [None, "bf16", "split"])
def test_dwconv_streaming_kernel_equals_small_launch_kernel(L, B, N, d, ragged, norm):
    """Chip-filling launches take the streaming kernel (rows through an LDS ring once per block, taps in registers, deferred stores);
    it adds the taps in the same order as the per-wave kernel, so the two agree bit for bit -- fp32 rows, the gamma-scaled bf16 (or
    hi | lo) copy and the sums of squares -- through ragged lengths, partial channel blocks (d = 96) and segment boundaries."""
    g = _g(B + N + d)
    x = torch.randn(B, N, d, generator=g).to(DEV)
    w = (torch.randn(31, d, generator=g) / math.sqrt(31)).to(DEV)
    bias = (0.1 * torch.randn(d, generator=g)).to(DEV)
    ld = None
    if ragged:
        ld = torch.randint(1, N + 1, (B,), generator=g).to(torch.int32)
        ld[0], ld[-1] = N, 1
        ld = ld.to(DEV)
    res = []
    for stream in (False, True):
        L.set_tuning(dwconv_rows_per_wave=0 if stream else -1)
        out = torch.full((B, N, d), float("nan"), device=DEV)
        kw = {}
        if norm:
            w2 = 2 if norm == "split" else 1
            hn = torch.zeros(B * N, w2 * d, dtype=torch.bfloat16, device=DEV)
            ssq = torch.zeros(B * N, (d // 32 + 3) // 4 * 4, device=DEV)
            gam = (1.0 + 0.3 * torch.randn(B, d, generator=_g(7))).to(DEV)
            kw = dict(norm=dict(out_bf16=hn, ld_out_bf16=w2 * d, gamma=gam[0], batch_stride=d, ssq=ssq, split=norm == "split"))
        L.dwconv(x, out, w, bias, B=B, N=N, d=d, ksize=31, lens=ld, **kw)
        torch.cuda.synchronize()
        res.append((out, kw["norm"]["out_bf16"], kw["norm"]["ssq"]) if norm else (out,))
    L.set_tuning()
    for a, b_ in zip(res[0], res[1]):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, b_)
    # and against the definition (x3:495-528 + the residual), fp32
    lens = ld.cpu() if ld is not None else torch.full((B,), N)
    m = (torch.arange(N)[None, :] < lens[:, None]).float()[..., None]
    xm = (x.cpu() * m).transpose(1, 2)
    conv = torch.nn.functional.conv1d(xm, w.cpu().t()[:, None, :], bias.cpu(), padding=15, groups=d).transpose(1, 2)
    ref = x.cpu() + m * torch.nn.functional.silu(conv)
    torch.testing.assert_close(res[1][0].cpu(), ref, atol=2e-5, rtol=1e-5)


def test_dwconv_rejects_bad_args(L):
    """The depthwise-conv launch path answers V2A_ERR_ARG for what its kernels are not built for -- before anything reaches the
    runtime (a process abort past the argument checks is what round 2's discarded one-channel-per-lane variant produced)."""
    B, N, d = 2, 44, 96                                        # d % 32 == 0 but not a whole 256-channel block
    x, out = torch.randn(B, N, d, device=DEV), torch.empty(B, N, d, device=DEV)
    w, bias = torch.randn(31, d, device=DEV), torch.zeros(d, device=DEV)
    hn, gam = torch.zeros(B * N, d, dtype=torch.bfloat16, device=DEV), torch.ones(d, device=DEV)
    ssq = torch.zeros(B * N, d // 32, device=DEV)
    L.dwconv(x, out, w, bias, B=B, N=N, d=d, ksize=31, norm=dict(out_bf16=hn, gamma=gam, ssq=ssq))        # supported
    with pytest.raises(L.V2AError, match="kernel_size"):
        L.dwconv(x, out, w[:7], bias, B=B, N=N, d=d, ksize=7)
    with pytest.raises(L.V2AError, match="alias"):
        L.dwconv(x, x, w, bias, B=B, N=N, d=d, ksize=31)
    with pytest.raises(L.V2AError, match="folded norm"):                                                 # sums of squares narrower than d / 32
        L.dwconv(x, out, w, bias, B=B, N=N, d=d, ksize=31, norm=dict(out_bf16=hn, gamma=gam, ssq=torch.zeros(B * N, 2, device=DEV)))
    with pytest.raises(L.V2AError, match="folded norm"):                                                 # shadow rows narrower than d
        L.dwconv(x, out, w, bias, B=B, N=N, d=d, ksize=31, norm=dict(out_bf16=hn, gamma=gam, ssq=ssq, ld_out_bf16=64))
    x2 = torch.randn(B, N, 72, device=DEV)                                                                # d % 32 != 0
    with pytest.raises(L.V2AError, match="folded norm"):
        L.dwconv(x2, torch.empty_like(x2), w[:, :72].contiguous(), bias[:72], B=B, N=N, d=72, ksize=31,
                 norm=dict(out_bf16=hn, gamma=gam, ssq=ssq))
    with pytest.raises(L.V2AError, match="B=0"):
        L.dwconv(x, out, w, bias, B=0, N=N, d=d, ksize=31)


# ----------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, gate, kv_len, q_len, clamp=50.0):
    """q (B,H,Nq,64) etc. fp32 CPU."""
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * 0.125
    sim = torch.tanh(sim / clamp) * clamp
    Nk = k.shape[2]
    km = torch.arange(Nk)[None, :] < torch.tensor(kv_len)[:, None]
    sim = sim.masked_fill(~km[:, None, None, :], -torch.finfo(torch.float32).max)
    out = sim.softmax(-1) @ v
    out = out * torch.sigmoid(gate)[..., None]
    qm = torch.arange(q.shape[2])[None, :] < torch.tensor(q_len)[:, None]
    return out * qm[:, None, :, None]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, "split"])
@pytest.mark.parametrize("B,H,Nq,Nk,kv_len,q_len", [(2, 2, 44, 44, [44, 30], [44, 30]), (1, 16, 782, 782, [782], [782]),
                                                  (2, 3, 100, 5, [5, 3], [100, 70]), (1, 1, 65, 129, [129], [65]),
                                                  (24, 16, 260, 200, [200, 130, 65, 1] * 6, [260, 200, 64, 259] * 6)])
@pytest.mark.parametrize("clamp", [50.0, 80.0])
def test_attention(L, dt, B, H, Nq, Nk, kv_len, q_len, clamp):
    """clamp 50 (the reference's value): the bf16 kernel runs without a running maximum (bounded weights); clamp 80: with
    the online maximum (2^(80 log2 e) is too close to fp32's range to skip it).  dt "split": fp32 tensors, products as
    three bf16 MFMA passes over hi | lo planes (the bf16x3 mode's kernel), held to 2e-4.  The last shape has 1920 workgroups:
    the bf16 kernel then runs one wave group per workgroup over all key tiles."""
    code = None
    if dt == "split":
        dt, code = torch.float32, L.BF16_SPLIT
    g = _g(Nq + Nk)
    q = torch.randn(B, H, Nq, 64, generator=g) * 2.0          # |logits| large enough that the tanh clamp bends them
    k = torch.randn(B, H, Nk, 64, generator=g) * 2.0
    v = torch.randn(B, H, Nk, 64, generator=g)
    gate = torch.randn(B, H, Nq, generator=g)
    q, k, v, gate = (t.to(dt).float() for t in (q, k, v, gate))
    ref = _attn_ref(q, k, v, gate, kv_len, q_len, clamp=clamp)
    # pack as the engine does: rows = tokens, [q | k | v | gate] columns (self) -- here separate buffers with paddings
    inner = H * 64
    qb = torch.zeros(B, Nq, inner + 16)
    qb[..., :inner] = q.permute(0, 2, 1, 3).reshape(B, Nq, inner)
    qb[..., inner:inner + H] = gate.permute(0, 2, 1)
    kvb = torch.cat([k.permute(0, 2, 1, 3).reshape(B, Nk, inner), v.permute(0, 2, 1, 3).reshape(B, Nk, inner)], -1)
    qd, kvd = qb.to(DEV, dt).contiguous(), kvb.to(DEV, dt).contiguous()
    out = torch.full((B, Nq, inner), float("nan"), dtype=dt, device=DEV)
    es = qd.element_size()
    L.attention(qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + inner * es, qd.data_ptr() + inner * es, out.data_ptr(),
                strides=(inner + 16, 2 * inner, 2 * inner, inner + 16, inner,
                         Nq * (inner + 16), Nk * 2 * inner, Nk * 2 * inner, Nq * (inner + 16), Nq * inner),
                B=B, H=H, Nq=Nq, Nk=Nk, kv_len=torch.tensor(kv_len, dtype=torch.int32, device=DEV),
                q_len=torch.tensor(q_len, dtype=torch.int32, device=DEV), scale=0.125, softclamp=clamp,
                dtype=L.dt_code(dt) if code is None else code)
    got = out.float().cpu().reshape(B, Nq, H, 64).permute(0, 2, 1, 3)
    tol = (2e-5 if code is None else 2e-4) if dt == torch.float32 else 2e-2
    torch.testing.assert_close(got, ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, "split"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_attention_saturated_logits(L, dt, sign):
    """Every logit at +-clamp (q . k * scale = +-2300 >> 50) over the largest key count of the path (782) with |v| = 8: the
    bounded-weight kernels keep no running maximum, so their fp32 sums hold Nk * |v| * 2^(+-72) -- finite by the margin the
    selection rule states (clamp * log2 e + log2 Nk <= 90).  All weights are equal, so the result is the mean of v."""
    code = None
    if dt == "split":
        dt, code = torch.float32, L.BF16_SPLIT
    B, H, N = 1, 2, 782
    q = torch.full((B, N, H * 64 + 16), 12.0)
    q[..., H * 64:] = 20.0                                  # gate: sigmoid(20) == 1 in fp32
    kv = torch.full((B, N, 2 * H * 64), sign * 24.0)        # 64 * 12 * 24 * 0.125 = 2304
    g = _g(3)
    v = (torch.rand(B, N, H * 64, generator=g) * 2 - 1) * 8.0
    kv[..., H * 64:] = v
    qd, kvd = q.to(DEV, dt).contiguous(), kv.to(DEV, dt).contiguous()
    out = torch.full((B, N, H * 64), float("nan"), dtype=dt, device=DEV)
    es, inner = qd.element_size(), H * 64
    L.attention(qd.data_ptr(), kvd.data_ptr(), kvd.data_ptr() + inner * es, qd.data_ptr() + inner * es, out.data_ptr(),
                strides=(inner + 16, 2 * inner, 2 * inner, inner + 16, inner, N * (inner + 16), N * 2 * inner, N * 2 * inner,
                         N * (inner + 16), N * inner),
                B=B, H=H, Nq=N, Nk=N, scale=0.125, softclamp=50.0, dtype=L.dt_code(dt) if code is None else code)
    got = out.float().cpu()
    ref = kvd[..., inner:].float().cpu().mean(1, keepdim=True).expand(B, N, inner)
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got, ref, atol=2e-2 if dt == torch.bfloat16 else 1e-4, rtol=0)


def test_attention_golden_self_and_cross(L, small, golden):
    """Full Attention module (Linears via v2a_gemm, rope, core) against blocks_small.npz."""
    from v2a_amd.dit import _Attn
    b, P, cfg = golden["blocks_small"], small["P"], small["cfg"]
    x = torch.from_numpy(b["x"])
    N, d, H = 44, 128, 2
    lens = torch.tensor([44, 30], dtype=torch.int32, device=DEV)
    tab = _rope_table(N).to(DEV)
    for name, cross in (("self_attn", False), ("cross_attn", True), ("cross_attn_rope", True)):
        rope = name != "cross_attn"          # A7: the default reading applies no rotary embedding in cross-attention
        pre = "transformer.layers.0.0.6" if cross else "transformer.layers.0.0.3"
        A = _Attn(P, pre, d, H, 64, torch.float32, DEV, cross=cross)
        xd = x.reshape(-1, d).to(DEV)
        qkv = torch.empty(2 * N, A.n_pad, device=DEV)
        L.gemm([(xd, d, d)], A.w_in, qkv, M=2 * N, N=A.n_pad, compute=L.F32, bias=A.b_in)
        if rope:
            L.rope(qkv, rows=2 * N, row_stride=A.n_pad, nheads=(1 if cross else 2) * H, rows_per_batch=N, pos_offset=0, table=tab, layout=0)
        ao = torch.empty(2 * N, 128, device=DEV)
        if cross:
            ctx = torch.from_numpy(b["ctx"]).reshape(-1, d).to(DEV)
            wkv = torch.cat([P[f"{pre}.to_k.weight"], P[f"{pre}.to_v.weight"]], 0).to(DEV)
            kv = torch.empty(10, 256, device=DEV)
            L.gemm([(ctx, d, d)], wkv, kv, M=10, N=256, compute=L.F32)
            if rope:
                L.rope(kv, rows=10, row_stride=256, nheads=H, rows_per_batch=5, pos_offset=N - 5, table=tab, layout=0)
            L.attention(qkv.data_ptr(), kv.data_ptr(), kv.data_ptr() + 128 * 4, qkv.data_ptr() + A.gate_col * 4, ao.data_ptr(),
                        strides=(A.n_pad, 256, 256, A.n_pad, 128, N * A.n_pad, 5 * 256, 5 * 256, N * A.n_pad, N * 128),
                        B=2, H=H, Nq=N, Nk=5, kv_len=torch.tensor([5, 3], dtype=torch.int32, device=DEV), q_len=lens,
                        scale=0.125, softclamp=50.0, dtype=L.F32)
        else:
            base = qkv.data_ptr()
            L.attention(base, base + 128 * 4, base + 256 * 4, base + A.gate_col * 4, ao.data_ptr(),
                        strides=(A.n_pad,) * 4 + (128,) + (N * A.n_pad,) * 4 + (N * 128,),
                        B=2, H=H, Nq=N, Nk=N, kv_len=lens, q_len=lens, scale=0.125, softclamp=50.0, dtype=L.F32)
        out = torch.empty(2 * N, d, device=DEV)
        L.gemm([(ao, 128, 128)], A.w_out, out, M=2 * N, N=d, compute=L.F32)
        np.testing.assert_allclose(out.cpu().numpy().reshape(2, N, d), b[name], atol=3e-5)


# -------------------------------------------------------------------- small setup kernels
def test_time_cond_golden(L, small, golden):
    P, b = small["P"], golden["blocks_small"]
    t = torch.tensor([0.0, 0.37, 1.0], device=DEV)
    out = torch.empty(3, 128, device=DEV)
    L.time_cond(t, P["transformer.time_cond_mlp.0.weights"].to(DEV), P["transformer.time_cond_mlp.1.weight"].t().contiguous().to(DEV),
                P["transformer.time_cond_mlp.1.bias"].to(DEV), out, S=3, d=128)
    np.testing.assert_allclose(out.cpu().numpy(), b["time_cond"], atol=2e-5)


def test_linear_small_scatter_and_registers(L):
    B, T, K, d, R = 2, 9, 51, 64, 4
    a = torch.randn(B * T, K, generator=_g(1))
    w, bias, add = torch.randn(d, K, generator=_g(2)), torch.randn(d, generator=_g(3)), torch.randn(T, d, generator=_g(4))
    regs = torch.randn(R, d, generator=_g(5))
    ref = (torch.nn.functional.linear(a, w, bias).reshape(B, T, d) + add[None])
    # (a) separate register fill, no shadow (proj_frames form)
    out = torch.zeros(2 * B, R + T, d, device=DEV)
    L.fill_registers(out, regs.to(DEV), B=2 * B, R=R, d=d, out_batch_stride=(R + T) * d)
    L.linear_small(a.to(DEV), w.t().contiguous().to(DEV), bias.to(DEV), add.to(DEV), out, M=B * T, K=K, T=T,
                   out_batch_stride=(R + T) * d, row_off=R, d=d, dup=B)
    # (b) fused register rows + bf16 shadow (embed form)
    out_b = torch.zeros(2 * B, R + T, d, device=DEV)
    sh = torch.zeros(2 * B, R + T, d, dtype=torch.bfloat16, device=DEV)
    L.linear_small(a.to(DEV), w.t().contiguous().to(DEV), bias.to(DEV), add.to(DEV), out_b, M=B * T, K=K, T=T,
                   out_batch_stride=(R + T) * d, row_off=R, d=d, dup=B, regs=regs.to(DEV), out_bf16=sh)
    for o in (out.cpu(), out_b.cpu()):
        for half in (0, B):
            torch.testing.assert_close(o[half:half + B, R:], ref, atol=2e-5, rtol=1e-5)
            assert torch.equal(o[half:half + B, :R], regs[None].expand(B, -1, -1))
    assert torch.equal(sh.cpu(), out_b.cpu().bfloat16())


@pytest.mark.parametrize("N,rope_cols", [(3 * 128 + 16, 256), (128 + 16, 128)])
def test_gemm_fused_rope(L, N, rope_cols):
    """RoPE (interleaved, A6) fused in the bf16 STORE epilogue == GEMM then the stand-alone rope kernel."""
    rows_per_batch, Bt, K = 44, 2, 128
    M = Bt * rows_per_batch
    a = torch.randn(M, K, generator=_g(1)).bfloat16()
    w = (torch.randn(N, K, generator=_g(2)) / math.sqrt(K)).bfloat16()
    bias = torch.zeros(N)
    bias[-16:] = torch.randn(16, generator=_g(3))
    tab = _rope_table(rows_per_batch + 3).to(DEV)
    fused = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm([(a.to(DEV), K, K)], w.to(DEV), fused, M=M, N=N, compute=L.BF16, bias=bias.to(DEV), rope_table=tab, rope_cols=rope_cols,
           rope_pos_offset=3, rows_per_batch=rows_per_batch)
    acc = a.float() @ w.float().t() + bias                              # fp32 accumulate of bf16 products
    ref = acc.clone()
    q = acc[:, :rope_cols].reshape(Bt, rows_per_batch, rope_cols // 64, 64).permute(0, 2, 1, 3)
    fr = O.rotary_freqs(rows_per_batch + 3, 64, "interleaved")[3:]
    ref[:, :rope_cols] = O.apply_rope(q, fr, "interleaved").permute(0, 2, 1, 3).reshape(M, rope_cols)
    torch.testing.assert_close(fused.float().cpu(), ref, atol=2e-2, rtol=2e-2)
    # and the un-rotated columns are exactly the plain GEMM's
    plain = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm([(a.to(DEV), K, K)], w.to(DEV), plain, M=M, N=N, compute=L.BF16, bias=bias.to(DEV))
    assert torch.equal(plain[:, rope_cols:], fused[:, rope_cols:])


@pytest.mark.parametrize("apg", [False, True])
def test_cfg_euler(L, apg):
    B, T, C, R = 2, 11, 16, 4
    y = torch.randn(B, T, C, generator=_g(1))
    pred = torch.randn(2 * B, R + T, C, generator=_g(2))
    dt = torch.tensor([0.1, 0.25, 0.05])
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    pc, pn = pred[:B, R:], pred[B:, R:]
    upd = pc - pn
    if apg:
        par, orth = O.apg_project(upd, pc)
        upd = orth + par * 0.3
    ref = y + dt[1] * (pc + upd * 2.0)
    yd, pd = y.to(DEV), pred.to(DEV)
    kw = dict(B=B, T=T, C_=C, pred_batch_stride=(R + T) * C, row_off=R)
    buf = None
    if apg:
        buf = torch.zeros(2 * B, dtype=torch.float64, device=DEV)
        L.apg_reduce(pd, buf, **kw)
    L.cfg_euler(yd, pd, cfg_strength=2.0, dt=dt.to(DEV), step=step, apg=buf, keep=0.3, **kw)
    L.step_advance(step)
    torch.testing.assert_close(yd.cpu(), ref, atol=1e-5, rtol=1e-5)
    assert int(step.item()) == 2


# --------------------------------------------------- HIP rows against vectors produced by the reference's own code
@pytest.fixture(scope="module")
def intree():
    import os
    from conftest import GOLDEN
    d = dict(np.load(os.path.join(GOLDEN, "intree_blocks.npz"), allow_pickle=False))
    d.pop("meta")
    return {k: torch.from_numpy(v) for k, v in d.items()}


def test_cfg_euler_apg_vs_reference_project(L, intree):
    """a2: v2a_apg_reduce + v2a_cfg_euler with remove_parallel_component against `project` (x3:162-173) run from the
    reference file itself: y + dt * (pc + s * (orthogonal + keep * parallel)),  (parallel, orthogonal) = project(pc - pn, pc)."""
    r = intree
    pc = r["project_y"]                                     # project(update, pred): y is the conditional prediction
    upd, par, orth = r["project_x"], r["project_parallel"], r["project_orthogonal"]
    pn = pc - upd
    B, T, C = pc.shape
    R, s, keep, dt = 4, 2.0, 0.25, 0.125
    pred = torch.zeros(2 * B, R + T, C)
    pred[:B, R:], pred[B:, R:] = pc, pn
    y = torch.randn(B, T, C, generator=_g(3))
    want = y + dt * (pc + s * (orth + keep * par))
    yd, pd = y.to(DEV), pred.to(DEV)
    apg = torch.zeros(2 * B, dtype=torch.float64, device=DEV)
    kw = dict(B=B, T=T, C_=C, pred_batch_stride=(R + T) * C, row_off=R)
    L.apg_reduce(pd, apg, **kw)
    L.cfg_euler(yd, pd, cfg_strength=s, dt=torch.tensor([dt], device=DEV), step=None, apg=apg, keep=keep, **kw)
    torch.testing.assert_close(yd.cpu(), want, atol=2e-6, rtol=1e-6)


def test_adaln_zero_vs_reference_module(L, intree):
    """a12: gate table by the SIGMOID epilogue, applied by GATE_RESID (resid = 0, identity weight: out = gate * x) against
    `AdaLNZero.forward` (x3:546-551) run from the reference file itself."""
    r = intree
    x, cond, w, b = r["adaln_x"], r["adaln_cond"], r["adaln_w"], r["adaln_b"]
    Bt, N, d = x.shape
    tab = torch.empty(Bt, d, device=DEV)
    L.gemm([(cond.to(DEV), d, d)], w.to(DEV), tab, M=Bt, N=d, compute=L.F32, epilogue=L.EPI_SIGMOID, bias=b.to(DEV))
    out = torch.zeros(Bt * N, d, device=DEV)
    L.gemm([(x.reshape(-1, d).to(DEV), d, d)], torch.eye(d, device=DEV), out, M=Bt * N, N=d, compute=L.F32, epilogue=L.EPI_GATE_RESID,
           resid=out, gate=tab, gate_batch_stride=d, rows_per_batch=N)
    torch.testing.assert_close(out.cpu().reshape(Bt, N, d), r["adaln_out"], atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("flag", [1, 0])
def test_cross_condition_vs_reference_module(L, intree, flag):
    """a13: the three concat-free multi-segment GEMMs against `TextAudioCrossCondition.forward` (x3:686-702) run from
    the reference file itself (fp32 mode), all reading the pre-update streams."""
    r = intree
    a, t, f = r["cc_audio"], r["cc_text"], r["cc_frames"]
    Bt, N, da = a.shape
    dt, df = t.shape[-1], f.shape[-1]
    M = Bt * N
    ad, td, fd = (v.reshape(M, -1).to(DEV) for v in (a, t, f))
    oa = torch.empty(M, da, device=DEV)
    L.gemm([(ad, da, da), (td, dt, dt), (fd, df, df)], r[f"cc_{flag}_text_frames_to_audio_weight"].to(DEV), oa, M=M, N=da, compute=L.F32,
           epilogue=L.EPI_RESID, resid=ad)
    torch.testing.assert_close(oa.cpu().reshape(Bt, N, da), r[f"cc_{flag}_out_audio"], atol=2e-5, rtol=1e-5)
    if flag:
        ot, of = torch.empty(M, dt, device=DEV), torch.empty(M, df, device=DEV)
        L.gemm([(ad, da, da), (td, dt, dt)], r["cc_1_audio_to_text_weight"].to(DEV), ot, M=M, N=dt, compute=L.F32, epilogue=L.EPI_RESID, resid=td)
        L.gemm([(ad, da, da), (fd, df, df)], r["cc_1_audio_to_frames_weight"].to(DEV), of, M=M, N=df, compute=L.F32, epilogue=L.EPI_RESID, resid=fd)
        torch.testing.assert_close(ot.cpu().reshape(Bt, N, dt), r["cc_1_out_text"], atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(of.cpu().reshape(Bt, N, df), r["cc_1_out_frames"], atol=2e-5, rtol=1e-5)


# ------------------------------------------------------------------------ split-bf16 ("bf16x3") building blocks
def _split_planes(x):
    """fp32 (rows, k) -> bf16 (rows, 2k) = [hi | lo] (the V2A_BF16_SPLIT layout)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, lo], -1).contiguous()


@pytest.mark.parametrize("hint", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("epi", ["store", "resid_shadow", "gate_norm", "geglu"])
@pytest.mark.parametrize("M,N,ks", [(300, 192, (256,)), (1564, 1024, (1024, 1280, 512)), (782, 1280, (1024, 1280)), (130, 2048, (512,)),
                                    (1564, 4096, (512,))])
def test_gemm_split_native(L, hint, epi, M, N, ks):
    """v2a_gemm with a_dtype V2A_BF16_SPLIT: A segments as [hi | lo] rows, W as [W_hi | W_lo], acc = A_lo W_hi + A_hi W_lo + A_hi W_hi
    in ONE launch over up to three logical K segments (TextAudioCrossCondition's pack, x3:693-700; hint 5 = the phase-interleaved
    256x256 kernel on three passes over the logical K -- hi x hi, hi x lo, lo x hi -- each over all segments), every epilogue of the bf16x3 mode: fp32 store, residual + split (hi | lo) shadow, gated residual + folded-norm producer with a split shadow, GEGLU with
    split output.  Against the fp64 product: ~1e-5 relative (three bf16 MFMA products per fp32 product)."""
    g = _g(M + N + len(ks))
    K = sum(ks)
    a = [torch.randn(M, k, generator=g) for k in ks]
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    segs = [(_split_planes(x).to(DEV), 2 * k, k) for x, k in zip(a, ks)]
    wd = torch.cat([w.bfloat16(), (w - w.bfloat16().float()).bfloat16()], 1).contiguous().to(DEV)          # [W_hi | W_lo]
    bias = (0.1 * torch.randn(N, generator=g))
    acc = torch.cat(a, 1).double() @ w.double().t()
    kw = dict(M=M, N=N, compute=L.BF16, a_split=True, tile_hint=hint)
    scale = float(acc.abs().max())
    if epi == "store":
        out = torch.empty(M, N, device=DEV)
        L.gemm(segs, wd, out, bias=bias.to(DEV), **kw)
        err = float((out.cpu().double() - (acc + bias.double())).abs().max())
        assert err < 3e-5 * max(scale, 1.0), err
    elif epi == "resid_shadow":
        res = torch.randn(M, N, generator=g)
        out, sh = torch.empty(M, N, device=DEV), torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
        L.gemm(segs, wd, out, epilogue=L.EPI_RESID, resid=res.to(DEV), out_bf16=sh, ld_out_bf16=2 * N, out_bf16_split=True, **kw)
        ref = res.double() + acc
        assert float((out.cpu().double() - ref).abs().max()) < 3e-5 * max(scale, 1.0)
        assert torch.equal(sh.cpu(), _split_planes(out.cpu()))
    elif epi == "gate_norm":
        res = torch.randn(M, N, generator=g)
        gate, gam = torch.rand(N, generator=g), 1 + 0.2 * torch.randn(N, generator=g)
        out = res.clone().to(DEV)
        sh, ssq = torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV), torch.zeros(M, N // 32, device=DEV)
        L.gemm(segs, wd, out, epilogue=L.EPI_GATE_RESID, resid=out, gate=gate.to(DEV), bias=bias.to(DEV), out_bf16=sh, ld_out_bf16=2 * N,
               out_bf16_split=True, norm_gamma=gam.to(DEV), norm_ssq=ssq, **kw)
        ref = res.double() + gate.double() * (acc + bias.double())
        assert float((out.cpu().double() - ref).abs().max()) < 3e-5 * max(scale, 1.0)
        assert torch.equal(sh.cpu(), _split_planes(out.cpu() * gam))
        torch.testing.assert_close(ssq.cpu().double(), (out.cpu().double() ** 2).reshape(M, N // 32, 32).sum(-1), rtol=1e-5, atol=1e-6)
    else:
        # GEGLU: W rows regrouped [16 value | 16 gate]; output hi | lo planes of the N / 2 hidden values, erf GELU by gelu_fast_f (Abramowitz-Stegun erf, 1.5e-7 abs)
        half = N // 2
        perm = torch.cat([torch.cat([torch.arange(j * 16, j * 16 + 16), half + torch.arange(j * 16, j * 16 + 16)]) for j in range(half // 16)])
        wp, bp = w[perm], bias[perm]
        wpd = torch.cat([wp.bfloat16(), (wp - wp.bfloat16().float()).bfloat16()], 1).contiguous().to(DEV)
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        L.gemm(segs, wpd, out, epilogue=L.EPI_GEGLU, bias=bp.to(DEV), ldo=N, out_split=True, **kw)
        z = acc + bias.double()
        ref = z[:, :half] * torch.nn.functional.gelu(z[:, half:])
        got = out[:, :half].float().cpu().double() + out[:, half:].float().cpu().double()
        err = float((got - ref).abs().max())
        assert err < 4e-5 * max(float(ref.abs().max()), 1.0), err


@pytest.mark.parametrize("hint", [0, 4, 5, 6])
def test_gemm_split_plane_offsets(L, hint):
    """v2a_gemm_args.a_lo_offset / out_bf16_lo_offset: ONE buffer of rows [x_hi | s_hi | x_lo | s_lo] read as a K = 2d split segment (lo plane
    2d further: the default) and, half by half, as K = d segments whose lo plane lies 2d -- not d -- behind the hi plane; and a split
    shadow written into one half of such a buffer.  Equal bit for bit to the same GEMMs on separately laid out operands."""
    M, d, N = 1564 if hint == 5 else 300, 256, 1024
    g = _g(50 + hint)
    x, sk = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    w = torch.randn(N, 2 * d, generator=g) / math.sqrt(2 * d)
    xs, ss = _split_planes(x), _split_planes(sk)
    wide = torch.cat([xs[:, :d], ss[:, :d], xs[:, d:], ss[:, d:]], 1).contiguous().to(DEV)      # [x_hi | s_hi | x_lo | s_lo]
    wd = _split_planes(w).to(DEV)
    kw = dict(M=M, N=N, compute=L.BF16, a_split=True, tile_hint=hint)
    ref, got = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    L.gemm([(xs.to(DEV), 2 * d, d), (ss.to(DEV), 2 * d, d)], wd, ref, **kw)                           # two standard segments
    L.gemm([(wide, 4 * d, 2 * d)], wd, got, **kw)                                                       # the wide buffer as one K = 2d segment
    assert torch.equal(got, ref)
    got.zero_()
    L.gemm([(wide, 4 * d, d, 2 * d), (wide[:, d:], 4 * d, d, 2 * d)], wd, got, **kw)                    # its halves as K = d segments, lo plane 2d further
    assert torch.equal(got, ref)
    # a split shadow written into the skip half of a wide buffer == the standard shadow, plane by plane
    res = torch.randn(M, d, generator=g).to(DEV)
    w2 = _split_planes(torch.randn(d, d, generator=g) / 16).to(DEV)
    o1, o2 = torch.empty(M, d, device=DEV), torch.empty(M, d, device=DEV)
    sh = torch.zeros(M, 2 * d, dtype=torch.bfloat16, device=DEV)
    wide2 = torch.zeros(M, 4 * d, dtype=torch.bfloat16, device=DEV)
    ekw = dict(M=M, N=d, compute=L.BF16, a_split=True, epilogue=L.EPI_RESID, resid=res, out_bf16_split=True, tile_hint=0 if hint == 5 else hint)
    L.gemm([(xs.to(DEV), 2 * d, d)], w2, o1, out_bf16=sh, ld_out_bf16=2 * d, **ekw)
    L.gemm([(xs.to(DEV), 2 * d, d)], w2, o2, out_bf16=wide2[:, d:], ld_out_bf16=4 * d, out_bf16_lo_offset=2 * d, **ekw)
    assert torch.equal(o1, o2) and torch.equal(wide2[:, d:2 * d], sh[:, :d]) and torch.equal(wide2[:, 3 * d:], sh[:, d:])
    assert float(wide2[:, :d].abs().max()) == 0 and float(wide2[:, 2 * d:3 * d].abs().max()) == 0
    with pytest.raises(L.V2AError, match="a_lo_offset"):
        L.gemm([(wide, 4 * d, d, 2 * d + 4)], wd[:, :2 * d].contiguous(), got, M=M, N=N, compute=L.BF16, a_split=True)


def test_gemm_split_native_folded_norm_consumer(L):
    """... and as the CONSUMER of a folded RMSNorm: A = split(x * gamma), the accumulator row scaled by sqrt(d) / |x| before the bias."""
    M, K, N = 300, 512, 256
    g = _g(77)
    x = torch.randn(M, K, generator=g) * 3
    gam = 1 + 0.2 * torch.randn(K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = 0.1 * torch.randn(N, generator=g)
    ssq = (x.double() ** 2).reshape(M, K // 32, 32).sum(-1).float()
    wd = torch.cat([w.bfloat16(), (w - w.bfloat16().float()).bfloat16()], 1).contiguous().to(DEV)
    out = torch.empty(M, N, device=DEV)
    L.gemm([(_split_planes(x * gam).to(DEV), 2 * K, K)], wd, out, M=M, N=N, compute=L.BF16, a_split=True, bias=bias.to(DEV),
           row_ssq=ssq.to(DEV), row_norm_dim=K)
    xn = torch.nn.functional.normalize(x.double(), dim=-1) * math.sqrt(K) * gam.double()
    ref = xn @ w.double().t() + bias.double()
    assert float((out.cpu().double() - ref).abs().max()) < 5e-5 * float(ref.abs().max())


def test_split_bf16_planes_and_three_segment_gemm(L):
    """v2a_split_bf16 / rmsnorm(split) write hi | lo planes; the three-segment GEMM [A_hi | A_hi | A_lo] x [W_hi | W_lo | W_hi]^T
    reproduces the fp32 product to ~1e-5 relative (bf16 alone: ~1e-2)."""
    from v2a_amd.dit import pack_weight
    M, K, N = 300, 256, 192
    g = _g(11)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    ad = a.to(DEV)
    sp = torch.empty(M, 2 * K, dtype=torch.bfloat16, device=DEV)
    L.split_bf16(ad, sp, rows=M, d=K)
    hi, lo = sp[:, :K].float().cpu(), sp[:, K:].float().cpu()
    assert torch.equal(hi, a.bfloat16().float()) and torch.equal(lo, (a - a.bfloat16().float()).bfloat16().float())
    assert float((hi + lo - a).abs().max()) < 2e-5 * float(a.abs().max())
    W2 = pack_weight(w, DEV, torch.bfloat16, split=True)                    # [W_hi | W_lo]: the operand of the native split GEMM
    assert W2.shape == (N, 2 * K) and torch.equal(W2[:, :K].cpu(), w.bfloat16())
    W3 = torch.cat([W2[:, :K], W2[:, K:], W2[:, :K]], 1).contiguous()        # [W_hi | W_lo | W_hi] against [A_hi | A_hi | A_lo]
    out = torch.empty(M, N, device=DEV)
    L.gemm([(sp, 2 * K, K), (sp, 2 * K, K), (sp[:, K:], 2 * K, K)], W3, out, M=M, N=N, compute=L.BF16)
    nat = torch.empty(M, N, device=DEV)
    L.gemm([(sp, 2 * K, K)], W2, nat, M=M, N=N, compute=L.BF16, a_split=True)                       # same three products per K step, one launch
    assert float((nat - out).abs().max()) < 2e-5
    ref = a.double() @ w.double().t()
    err3 = float((out.cpu().double() - ref).abs().max())
    out1 = torch.empty(M, N, device=DEV)
    L.gemm([(a.bfloat16().to(DEV), K, K)], w.bfloat16().to(DEV), out1, M=M, N=N, compute=L.BF16)
    err1 = float((out1.cpu().double() - ref).abs().max())
    print(f"split-bf16 GEMM max err {err3:.2e} (plain bf16 {err1:.2e})")
    assert err3 < 3e-5 and err3 < err1 / 100
    # rmsnorm with split output == split of the fp32 rmsnorm
    gam = 1 + 0.1 * torch.randn(K, generator=g)
    y32 = torch.empty(M, K, device=DEV)
    L.rmsnorm(ad, y32, rows=M, d=K, gamma=gam.to(DEV))
    ys = torch.empty(M, 2 * K, dtype=torch.bfloat16, device=DEV)
    L.rmsnorm(ad, ys, rows=M, d=K, gamma=gam.to(DEV), split=True)
    L.split_bf16(y32, sp, rows=M, d=K)
    assert torch.equal(ys[:, :K].cpu(), sp[:, :K].cpu())                      # hi planes identical
    rec = ys[:, :K].float() + ys[:, K:].float()                              # lo may use a fused multiply-subtract: compare the sum
    assert float((rec - y32).abs().max()) < 2e-5 * float(y32.abs().max())


@pytest.mark.parametrize("hint", [1, 2, 3, 4, 7, 8, 9])
def test_gemm_tile_hint(L, hint):
    """tile_hint picks one tile shape for the call (1: 128x256 ... 4: 64x64, 7: the 256x256 phase-interleaved kernel, 8 / 9: 64x128 /
    64x64 with the 6-deep ring): the
    result equals the automatic choice bit for bit -- the K summation order of an output element does not depend on the tile."""
    M, N, K = 1564, 1552, 192
    g = _g(hint * 100)
    a = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    ref, got = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    L.gemm([(a, K, K)], w, ref, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID, bias=bias, resid=resid)
    L.gemm([(a, K, K)], w, got, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID, bias=bias, resid=resid, tile_hint=hint)
    assert torch.equal(got, ref)
    exact = resid.double().cpu() + a.float().double().cpu() @ w.float().double().cpu().t() + bias.double().cpu()
    torch.testing.assert_close(got.cpu().double(), exact, atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("hint", [8, 9])
@pytest.mark.parametrize("K", [64, 128, 320, 384, 448, 832, 1024])
def test_gemm_deep_ring_k_tails(L, hint, K):
    """6-deep ring (64x128 / 64x64 tiles): every length of the K loop's tail relative to the ring (1 .. 16 K tiles), three
    A segments, ragged M and N edges, the gated-residual epilogue -- bit for bit what the 3-deep 64x64 kernel gives."""
    M, N = 333, 456
    g = _g(K + hint)
    ks = [K] if K < 192 else [64, K - 128, 64]
    segs = [torch.randn(M, k, generator=g).bfloat16().to(DEV) for k in ks]
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    gate = torch.randn(1, N, generator=g).to(DEV)
    kw = dict(M=M, N=N, compute=L.BF16, epilogue=L.EPI_GATE_RESID, bias=bias, resid=resid, gate=gate, gate_step_stride=0,
              gate_batch_stride=0, rows_per_batch=M)
    ref, got = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    L.gemm([(a, k, k) for a, k in zip(segs, ks)], w, ref, tile_hint=4, **kw)
    L.gemm([(a, k, k) for a, k in zip(segs, ks)], w, got, tile_hint=hint, **kw)
    assert torch.equal(got, ref)
    acat = torch.cat([a.float().cpu() for a in segs], 1).double()
    exact = resid.double().cpu() + gate.double().cpu() * (acat @ w.float().double().cpu().t() + bias.double().cpu())
    torch.testing.assert_close(got.cpu().double(), exact, atol=5e-4, rtol=1e-4)


# -------------------------------------------------------------------------------- RMSNorm folded into its neighbours
@pytest.mark.parametrize("hint", [0, 1, 2, 3, 4, 7])
@pytest.mark.parametrize("epi", ["resid", "gate_resid"])
def test_gemm_folded_norm_producer(L, hint, epi):
    """RESID / GATE_RESID with norm_gamma + norm_ssq: the bf16 shadow is bf16(out * gamma) with the step-indexed gamma row
    (and the switched row for m >= norm_switch_row), the sums of squares of out per 32 columns land in norm_ssq -- for every
    tile shape, with ragged M / N edges."""
    M, N, K, rpb = 333, 416, 192, 111
    g = _g(hint * 7 + len(epi))
    a = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    gam = (1.0 + 0.3 * torch.randn(3, 2, N, generator=g)).to(DEV)          # [step][slot][N]
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    out = torch.empty(M, N, device=DEV)
    sh = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    ssq = torch.full((M, N // 32), -1.0, device=DEV)
    kw = dict(M=M, N=N, compute=L.BF16, bias=bias, resid=resid, step=step, rows_per_batch=rpb, tile_hint=hint, out_bf16=sh,
              norm_gamma=gam[0, 0], norm_step_stride=gam.stride(0), norm_switch_row=2 * rpb, norm_switch_offset=N, norm_ssq=ssq)
    if epi == "gate_resid":
        gate = torch.rand(3, N, generator=g).to(DEV)
        kw.update(epilogue=L.EPI_GATE_RESID, gate=gate, gate_step_stride=N)
    else:
        kw.update(epilogue=L.EPI_RESID)
    L.gemm([(a, K, K)], w, out, **kw)
    plain = torch.empty(M, N, device=DEV)
    kw2 = {k: v for k, v in kw.items() if not k.startswith("norm_") and k != "out_bf16"}
    L.gemm([(a, K, K)], w, plain, **kw2)
    assert torch.equal(out, plain)                                          # the fp32 result is untouched by the fold
    grow = torch.where((torch.arange(M, device=DEV) >= 2 * rpb)[:, None], gam[2, 1][None], gam[2, 0][None])
    assert torch.equal(sh, (out * grow).bfloat16())
    ref = (out.double() ** 2).reshape(M, N // 32, 32).sum(-1)
    torch.testing.assert_close(ssq.double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("hint", [0, 1, 4, 7])
@pytest.mark.parametrize("epi", ["store_bf16", "store_f32", "geglu", "store_rope"])
def test_gemm_folded_norm_consumer(L, hint, epi):
    """row_ssq: accumulator row m is scaled by sqrt(d) / max(sqrt(sum of its partial sums), 1e-12) before bias / GELU / RoPE."""
    M, N, K, d = 300, 512, 256, 192                                         # 6 partial sums: the row is padded to 8 with zeros
    g = _g(hint + 31 * len(epi))
    a = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    ssq = torch.zeros(M, 8)
    ssq[:, :d // 32] = torch.rand(M, d // 32, generator=g) * 40 + 1
    ssq = ssq.to(DEV)
    ssq[5] = 0.0                                                            # an all-zero row: eps clamp, 0 * huge = 0, no NaN
    a[5] = 0
    rstd = (math.sqrt(d) / ssq.double().sum(-1).sqrt().clamp_min(1e-12)).cpu()
    acc = a.float().double().cpu() @ w.float().double().cpu().t()
    kw = dict(M=M, N=N, compute=L.BF16, bias=bias, tile_hint=hint, row_ssq=ssq, row_norm_dim=d)
    if epi == "geglu":
        out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV)
        L.gemm([(a, K, K)], w, out, epilogue=L.EPI_GEGLU, ldo=N // 2, **kw)
        z = (acc * rstd[:, None] + bias.double().cpu()).reshape(M, N // 32, 2, 16)
        ref = (z[:, :, 0] * torch.nn.functional.gelu(z[:, :, 1])).reshape(M, N // 2)
        ref[5] = (bias.double().cpu().reshape(N // 32, 2, 16)[:, 0] * torch.nn.functional.gelu(bias.double().cpu().reshape(N // 32, 2, 16)[:, 1])).reshape(-1)
        torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-2, atol=2e-2)
        return
    if epi == "store_rope":
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        L.gemm([(a, K, K)], w, out, rope_table=_rope_table(M).to(DEV), rope_cols=128, rope_pos_offset=0, rows_per_batch=M, **kw)
        ref = (acc * rstd[:, None] + bias.double().cpu()).float()
        ref[5] = bias.cpu()
        q = ref[:, :128].reshape(1, M, 2, 64).permute(0, 2, 1, 3)
        ref[:, :128] = O.apply_rope(q, O.rotary_freqs(M, 64, "interleaved"), "interleaved").permute(0, 2, 1, 3).reshape(M, 128)
        torch.testing.assert_close(out.float().cpu(), ref, rtol=2e-2, atol=3e-2)
        return
    out = torch.empty(M, N, dtype=torch.bfloat16 if epi == "store_bf16" else torch.float32, device=DEV)
    L.gemm([(a, K, K)], w, out, **kw)
    ref = acc * rstd[:, None] + bias.double().cpu()
    ref[5] = bias.double().cpu()                                            # 0 * (sqrt(d) / 1e-12) = 0
    tol = dict(rtol=1e-2, atol=2e-2) if epi == "store_bf16" else dict(rtol=1e-4, atol=5e-4)
    torch.testing.assert_close(out.cpu().double(), ref, **tol)


@pytest.mark.parametrize("N,d,lens", [(44, 128, [44, 30]), (782, 512, None), (100, 1280, [100, 33]), (782, 1024, [782, 1])])
def test_dwconv_folded_norm(L, N, d, lens):
    """v2a_dwconv_silu_residual_norm: the fp32 result equals the plain kernel's bit for bit; the bf16 copy is bf16(out * gamma)
    with the step- and batch-indexed gamma row; the sums of squares per 32 channels match."""
    B = 2
    x = torch.randn(B, N, d, generator=_g(N)).to(DEV)
    w = (torch.randn(31, d, generator=_g(N + 1)) / math.sqrt(31)).to(DEV)
    bias = (0.1 * torch.randn(d, generator=_g(N + 2))).to(DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    gam = (1.0 + 0.3 * torch.randn(3, B, d, generator=_g(N + 3))).to(DEV)
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    plain, out = torch.empty(B, N, d, device=DEV), torch.empty(B, N, d, device=DEV)
    hn = torch.zeros(B * N, d, dtype=torch.bfloat16, device=DEV)
    ssq = torch.full((B * N, d // 32), -1.0, device=DEV)
    L.dwconv(x, plain, w, bias, B=B, N=N, d=d, ksize=31, lens=ld)
    L.dwconv(x, out, w, bias, B=B, N=N, d=d, ksize=31, lens=ld,
             norm=dict(out_bf16=hn, gamma=gam[0, 0], ssq=ssq, step=step, step_stride=gam.stride(0), batch_stride=gam.stride(1)))
    assert torch.equal(out, plain)
    assert torch.equal(hn.reshape(B, N, d), (out * gam[1][:, None, :]).bfloat16())
    ref = (out.double() ** 2).reshape(B * N, d // 32, 32).sum(-1)
    torch.testing.assert_close(ssq.double(), ref, rtol=1e-5, atol=1e-6)


def test_folded_norm_chain_equals_norm_then_linear(L):
    """conv -> RMSNorm -> Linear with the norm folded (gamma on the conv's bf16 copy, 1 / rms in the GEMM epilogue) against the
    three separate kernels: same result up to the bf16 rounding of the operand (the scale moves across the rounding)."""
    B, N, d, Nout = 2, 782, 1024, 384
    x = torch.randn(B, N, d, generator=_g(1)).to(DEV)
    w = (torch.randn(31, d, generator=_g(2)) / math.sqrt(31)).to(DEV)
    bias = (0.1 * torch.randn(d, generator=_g(3))).to(DEV)
    gam = (1.0 + 0.2 * torch.randn(d, generator=_g(4))).to(DEV)
    W = (torch.randn(Nout, d, generator=_g(5)) / math.sqrt(d)).bfloat16().to(DEV)
    b2 = (0.1 * torch.randn(Nout, generator=_g(6))).to(DEV)
    y = torch.empty(B, N, d, device=DEV)
    hn = torch.empty(B * N, d, dtype=torch.bfloat16, device=DEV)
    L.dwconv(x, y, w, bias, B=B, N=N, d=d, ksize=31)
    L.rmsnorm(y, hn, rows=B * N, d=d, gamma=gam)
    ref = torch.empty(B * N, Nout, device=DEV)
    L.gemm([(hn, d, d)], W, ref, M=B * N, N=Nout, compute=L.BF16, bias=b2)
    hn2 = torch.empty(B * N, d, dtype=torch.bfloat16, device=DEV)
    ssq = torch.empty(B * N, d // 32, device=DEV)
    L.dwconv(x, y, w, bias, B=B, N=N, d=d, ksize=31, norm=dict(out_bf16=hn2, gamma=gam, ssq=ssq))
    got = torch.empty(B * N, Nout, device=DEV)
    L.gemm([(hn2, d, d)], W, got, M=B * N, N=Nout, compute=L.BF16, bias=b2, row_ssq=ssq, row_norm_dim=d)
    exact = torch.nn.functional.linear(torch.nn.functional.normalize(y.reshape(B * N, d), dim=-1) * math.sqrt(d) * gam, W.float(), b2)
    e_ref, e_got = float((ref - exact).abs().max()), float((got - exact).abs().max())
    print(f"norm -> linear vs fp32: separate kernels {e_ref:.3e}, folded {e_got:.3e}")
    assert e_got < 1.5 * e_ref + 1e-3


@pytest.mark.parametrize("hint", [1, 2, 7])
@pytest.mark.parametrize("ks", [(512, 512, 512), (1024, 1280, 512), (64, 128, 64)])
def test_gemm_tile_hint_three_segments_bitwise(L, hint, ks):
    """Three K-concatenated segments (the cross-condition GEMMs; every bf16x3 GEMM): 128x256 / 128x128 ring tiles and the
    256x256 phase-interleaved kernel give bit for bit what 64x64 tiles give -- segment switches do not reorder the K sum."""
    M, N = 1564, 1552
    g = _g(hint + sum(ks))
    segs = [torch.randn(M, k, generator=g).bfloat16().to(DEV) for k in ks]
    K = sum(ks)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV)
    ref, got = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    a = [(t, k, k) for t, k in zip(segs, ks)]
    L.gemm(a, w, ref, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID, resid=resid, tile_hint=4)
    L.gemm(a, w, got, M=M, N=N, compute=L.BF16, epilogue=L.EPI_RESID, resid=resid, tile_hint=hint)
    assert torch.equal(got, ref)
    # the bf16x3 QKV call: [A_hi | A_hi | A_lo] planes of ONE buffer as the three segments (row stride 2k), fp32 STORE + bias
    k = ks[0]
    planes = torch.randn(M, 2 * k, generator=g).bfloat16().to(DEV)
    w3 = (torch.randn(N, 3 * k, generator=g) / math.sqrt(3 * k)).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    a3 = [(planes, 2 * k, k), (planes, 2 * k, k), (planes[:, k:], 2 * k, k)]
    L.gemm(a3, w3, ref, M=M, N=N, compute=L.BF16, bias=bias, tile_hint=4)
    L.gemm(a3, w3, got, M=M, N=N, compute=L.BF16, bias=bias, tile_hint=hint)
    assert torch.equal(got, ref)
    # ... with the rotary embedding fused into the epilogue (fp32 output): the rotation is written with explicit fused
    # multiply-adds so that every instantiation rounds it the same way
    tab = _rope_table(782).to(DEV)
    kw = dict(M=M, N=N, compute=L.BF16, bias=bias, rope_table=tab, rope_cols=1024, rope_pos_offset=0, rows_per_batch=782)
    L.gemm(a3, w3, ref, tile_hint=4, **kw)
    L.gemm(a3, w3, got, tile_hint=hint, **kw)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("B,Nq,Nk,kv_len,q_len", [(1, 782, 32, [20], [782]), (2, 782, 32, [32, 1], [782, 500]), (3, 100, 64, [64, 33, 0], [100, 64, 1]),
                                                  (2, 64, 5, [5, 3], [64, 10]), (1, 44, 16, None, None)])
@pytest.mark.parametrize("H,K", [(16, 1024), (3, 512)])
@pytest.mark.parametrize("clamp", [50.0, 80.0, 0.0])
@pytest.mark.parametrize("folded,rope", [(True, True), (False, False)])
def test_qproj_xattn_equals_two_launches(L, B, Nq, Nk, kv_len, q_len, H, K, clamp, folded, rope):
    """v2a_qproj_xattn (q-projection + RoPE + cross-attention + head gate in one launch) == v2a_gemm into a [q | gate] buffer followed
    by v2a_attention, bit for bit: sequences that end inside a 64-row tile, ragged query / key lengths (one clip without keys),
    every clamp mode, with and without the folded-RMSNorm row scale and the fused RoPE."""
    g = _g(B * Nq + Nk + H)
    M, inner, N = B * Nq, H * 64, H * 64 + 16
    a = (torch.randn(M, K, generator=g) * 0.7).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K) * 3.0).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    kv = (torch.randn(B, Nk, 2 * inner, generator=g) * 1.5).bfloat16().to(DEV)
    tab = _rope_table(Nq + 5).to(DEV) if rope else None
    ssq = None
    if folded:
        ssq = torch.zeros(M, 40, device=DEV)
        ssq[:, :K // 32] = (torch.rand(M, K // 32, generator=g) * 30 + 5).to(DEV)
    kvl = torch.tensor(kv_len, dtype=torch.int32, device=DEV) if kv_len is not None else None
    ql = torch.tensor(q_len, dtype=torch.int32, device=DEV) if q_len is not None else None
    rk = dict(rope_table=tab, rope_cols=inner, rope_pos_offset=2) if rope else {}
    nk = dict(row_ssq=ssq, row_norm_dim=K) if folded else {}
    # two launches
    qb = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    L.gemm([(a, K, K)], w, qb, M=M, N=N, compute=L.BF16, bias=bias, rows_per_batch=Nq, tile_hint=4, **rk, **nk)
    ref = torch.full((B, Nq, inner), 7.0, dtype=torch.bfloat16, device=DEV)
    L.attention(qb.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 2, qb.data_ptr() + inner * 2, ref.data_ptr(),
                strides=(N, 2 * inner, 2 * inner, N, inner, Nq * N, Nk * 2 * inner, Nk * 2 * inner, Nq * N, Nq * inner),
                B=B, H=H, Nq=Nq, Nk=Nk, kv_len=kvl, q_len=ql, scale=0.125, softclamp=clamp, dtype=L.BF16)
    # one launch
    got = torch.full((B, Nq, inner), 7.0, dtype=torch.bfloat16, device=DEV)
    L.qproj_xattn(a, K, K, w, bias=bias, M=M, N=N, rows_per_batch=Nq, k=kv.data_ptr(), v=kv.data_ptr() + inner * 2, out=got.data_ptr(),
                  kv_strides=(2 * inner, 2 * inner, Nk * 2 * inner, Nk * 2 * inner), out_strides=(inner, Nq * inner), B=B, H=H, Nk=Nk,
                  kv_len=kvl, q_len=ql, scale=0.125, softclamp=clamp, **rk, **nk)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all()
    assert ref.float().abs().max() > 0.05
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max()


@pytest.mark.parametrize("B,Nq,Nk,kv_len,q_len", [(1, 782, 16, [11], [782]), (2, 782, 32, [32, 1], [782, 500]), (3, 100, 64, [64, 33, 0], [100, 64, 1])])
@pytest.mark.parametrize("clamp", [50.0, 80.0, 0.0])
@pytest.mark.parametrize("folded,rope", [(True, True), (False, False)])
def test_qproj_xattn_split_equals_two_launches(L, B, Nq, Nk, kv_len, q_len, clamp, folded, rope, K=1024):
    """bf16x3 arithmetic: v2a_qproj_xattn on split operands == the split GEMM into an fp32 [q | gate] buffer followed by v2a_attention
    (dtype V2A_BF16_SPLIT, out_split), bit for bit -- and within 2e-4 of the fp32 reference."""
    H = 16
    g = _g(7 * B * Nq + Nk)
    M, inner, N = B * Nq, H * 64, H * 64 + 16
    a32 = torch.randn(M, K, generator=g) * 0.7
    w32 = torch.randn(N, K, generator=g) / math.sqrt(K) * 3.0
    a = _split_planes(a32).to(DEV)
    w = _split_planes(w32).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    kv = (torch.randn(B, Nk, 2 * inner, generator=g) * 1.5).to(DEV)
    tab = _rope_table(Nq + 5).to(DEV) if rope else None
    ssq = None
    if folded:
        ssq = torch.zeros(M, 40, device=DEV)
        ssq[:, :K // 32] = (torch.rand(M, K // 32, generator=g) * 30 + 5).to(DEV)
    kvl = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    ql = torch.tensor(q_len, dtype=torch.int32, device=DEV)
    rk = dict(rope_table=tab, rope_cols=inner, rope_pos_offset=2) if rope else {}
    nk = dict(row_ssq=ssq, row_norm_dim=K) if folded else {}
    qb = torch.zeros(M, N, device=DEV)
    L.gemm([(a, 2 * K, K)], w, qb, M=M, N=N, compute=L.BF16, bias=bias, rows_per_batch=Nq, a_split=True, tile_hint=1, **rk, **nk)
    ref = torch.full((B, Nq, 2 * inner), 7.0, dtype=torch.bfloat16, device=DEV)
    L.attention(qb.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, qb.data_ptr() + inner * 4, ref.data_ptr(),
                strides=(N, 2 * inner, 2 * inner, N, 2 * inner, Nq * N, Nk * 2 * inner, Nk * 2 * inner, Nq * N, Nq * 2 * inner),
                B=B, H=H, Nq=Nq, Nk=Nk, kv_len=kvl, q_len=ql, scale=0.125, softclamp=clamp, dtype=L.BF16_SPLIT, out_split=True)
    got = torch.full((B, Nq, 2 * inner), 7.0, dtype=torch.bfloat16, device=DEV)
    L.qproj_xattn(a, 2 * K, K, w, bias=bias, M=M, N=N, rows_per_batch=Nq, k=kv.data_ptr(), v=kv.data_ptr() + inner * 4, out=got.data_ptr(),
                  kv_strides=(2 * inner, 2 * inner, Nk * 2 * inner, Nk * 2 * inner), out_strides=(2 * inner, Nq * 2 * inner), B=B, H=H, Nk=Nk,
                  kv_len=kvl, q_len=ql, scale=0.125, softclamp=clamp, split=True, **rk, **nk)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0.05
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max()


def test_qproj_xattn_split_small_k_then_large_k(L):
    """The launch sizes its dynamic LDS by K (the preloaded gate row); the > 64 KB opt-in is set once per kernel for the largest K the
    entry point takes, so a model of another width later in the process (K = 512, then K = 2048) is not refused."""
    for K in (512, 2048):
        test_qproj_xattn_split_equals_two_launches(L, 2, 782, 32, [32, 1], [782, 500], 50.0, False, True, K=K)     # (a folded norm holds <= 40 sums: K <= 1280)


def test_qproj_xattn_rejects_bad_args(L):
    a = torch.zeros(64, 512, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(65, 512, dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros(1, 80, 128, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(1, 64, 64, dtype=torch.bfloat16, device=DEV)
    base = dict(bias=None, M=64, N=65, rows_per_batch=64, k=kv.data_ptr(), v=kv.data_ptr() + 128, out=out.data_ptr(), kv_strides=(128, 128, 80 * 128, 80 * 128),
                out_strides=(64, 64 * 64), B=1, H=1, Nk=16, scale=0.125, softclamp=50.0)
    L.qproj_xattn(a, 512, 512, w, **base)
    for bad in (dict(Nk=65), dict(N=64), dict(M=63), dict(rows_per_batch=32)):
        with pytest.raises(L.V2AError):
            L.qproj_xattn(a, 512, 512, w, **{**base, **bad})
    with pytest.raises(L.V2AError):
        L.qproj_xattn(a, 512, 320, w, **base)          # K not a multiple of 512
