"""CPU: the reference helpers of tests/test_gemm_fp32_gpu.py against loops, torch and the source -- a wrong helper would either fail every GPU
case or, worse, agree with a kernel that is wrong in the same way."""
import os
import re

import numpy as np
import torch

import test_gemm_fp32_gpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_glu_unpack_against_a_loop_and_torch_glu():
    M, N, K = 5, 96, 16
    a = torch.randn(M, K, generator=_g(1)).double()
    w = torch.randn(N, K, generator=_g(2)).double()                          # [N / 2 value rows | N / 2 gate rows]
    z = a @ w.t()
    # the packing of the kernel: group j of 32 rows = 16 value rows, then their 16 gate rows
    perm = torch.tensor([(N // 2) * half + 16 * j + i for j in range(N // 32) for half in (0, 1) for i in range(16)])
    assert sorted(perm.tolist()) == list(range(N))
    packed = a @ w[perm].t()
    v, gt = R.glu_unpack(packed)
    assert v.shape == (M, N // 2) and torch.equal(v, z[:, :N // 2]) and torch.equal(gt, z[:, N // 2:])
    for m in range(M):
        for c in range(N // 2):
            assert v[m, c] == packed[m, 32 * (c // 16) + c % 16] and gt[m, c] == packed[m, 32 * (c // 16) + 16 + c % 16]
    torch.testing.assert_close(v * torch.sigmoid(gt), torch.nn.functional.glu(z, -1), rtol=0, atol=1e-15)


def test_gate_rows_against_a_loop_and_the_strides():
    M, N, rpb, steps, step = 53, 8, 23, 5, 3
    B = (M + rpb - 1) // rpb
    buf = torch.full((steps, B, N + 4), float("nan"))
    table = buf[:, :, :N]
    table.copy_(torch.rand(steps, B, N, generator=_g(3)))
    rows = R.gate_rows(table, step, M, rpb)
    assert rows.shape == (M, N)
    flat = buf.reshape(-1)
    for m in range(M):
        assert torch.equal(rows[m], table[step, m // rpb])
        # as the kernel addresses it: base + step * step stride + (m / rows_per_batch) * batch stride, in elements
        at = step * table.stride(0) + (m // rpb) * table.stride(1)
        assert torch.equal(rows[m], flat[at:at + N])
    assert (M - 1) // rpb == B - 1 and M % rpb != 0 and rpb % 16 != 0         # a partial last batch element, a boundary inside a 16-row slab


def test_tie_inputs_separate_the_three_roundings():
    a = R.tie_inputs(65, 128, 7)
    even, up, trunc = (R.round_bf16_bits(a, rule) for rule in ("even", "half_up", "trunc"))
    lo, hi = torch.minimum(trunc, up), torch.maximum(trunc, up)
    # exactly half way between two neighbouring bf16 values, of both signs
    assert torch.equal(a.double() * 2, lo.double() + hi.double()) and bool((lo < hi).all())
    assert bool((a > 0).any()) and bool((a < 0).any())
    for t in (even, up, trunc):
        assert torch.equal(t.bfloat16().float(), t)                          # bf16 values
    # torch's rounding (the reference's) is nearest-even: the neighbour whose last mantissa bit is 0
    assert torch.equal(a.bfloat16().float(), even)
    assert int(((even.view(torch.int32) >> 16) & 1).sum()) == 0
    # ... which half-up misses where the lower neighbour is even, truncation where it is odd: both happen, often
    n = a.numel()
    assert n / 4 < int((even != up).sum()) < 3 * n / 4 and n / 4 < int((even != trunc).sum()) < 3 * n / 4
    assert bool(((even != up) ^ (even != trunc)).all())
    # half-up towards +infinity (not away from zero) differs as well
    up_signed = torch.where(a > 0, up, trunc)
    assert int((even != up_signed).sum()) > n / 4
    # the bit rule agrees with torch on ordinary values too
    x = torch.randn(1000, generator=_g(8))
    assert torch.equal(R.round_bf16_bits(x, "even"), x.bfloat16().float())


def test_tile_rule_is_the_one_in_the_source():
    src = open(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "gemm.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "int fp32_tile_by_shape(int M, int N) { return ntiles(M, N, 128, 128) < 224 && M > 64 ? 64 : 128; }" in flat
    assert ("return fp32_tile_by_shape(a->M, a->N) == 64 ? dispatch_epi<float, false, 64, 64>(a, p, to) : dispatch_epi<float, false, 128, 128>(a, p, to);"
            in flat)
    # ... and the one the library follows: the instantiation v2a_gemm would launch reports its tile and its workgroups (no GPU needed)
    from v2a_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    t = torch.zeros(1, 16)
    for M in (1, 63, 64, 65, 128, 129, 200, 1792, 1793, 1800, 3000):
        for N in (1, 3, 20, 128, 129, 144, 272, 1792, 1793, 1920, 4096):
            t128 = -(-M // 128) * -(-N // 128)
            assert R.tile_of(M, N) == (64 if (t128 < 224 and M > 64) else 128), (M, N)
            c = L.gemm_choice([(t, 16, 16)], t, t, M=M, N=N, compute=L.F32, ldo=N)
            assert (c.family, c.bm, c.bn, c.bk, c.tiles) == (L.GEMM_REGISTER_STAGED, R.tile_of(M, N), R.tile_of(M, N), 16, R.workgroups(M, N)), (M, N)
    # the shapes of the GPU file reach the tiles, workgroup counts and remainders they were chosen for
    for (M, N), (tile, wgs) in R.TILES.items():
        assert (R.tile_of(M, N), R.workgroups(M, N)) == (tile, wgs), (M, N)
    for M, N, _ in R.EPI_CASES + R.GLU_CASES:
        assert (M, N) in R.TILES
    assert {R.tile_of(M, N) for M, N, _ in R.EPI_CASES} == {64, 128} and {R.tile_of(M, N) for M, N, _ in R.GLU_CASES} == {64, 128}
    assert R.workgroups(*R.BIG) == 225 and R.workgroups(*R.BIG) % 8 == 1 and R.workgroups(273, 272) % 8 == 1 and R.BIG[0] % 128 == 8
    assert R.tile_of(R.BIG_ROWS, R.BIG[1]) == 64


def _chain_f32(a, w, order):
    """acc = fp32(acc + a_k w_k) over k in `order`: the product is exact in float64, the sum is rounded to fp32 once per step."""
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=np.float32)
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    for k in order:
        acc = (acc.astype(np.float64) + a64[:, k, None] * w64[None, :, k]).astype(np.float32)
    return acc


def test_dot_bound_holds_for_an_fp32_chain_and_sees_a_dropped_k_tile():
    M, N = 37, 29
    for K in (16, 80):
        g = _g(K)
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        bias, res, gate = 0.1 * torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.rand(M, N, generator=g)
        exact = a.double() @ w.double().t()
        absacc = a.double().abs() @ w.double().abs().t()
        orders = [list(range(K)), list(range(K))[::-1], [k for q in range(4) for k in range(q, K, 4)]]
        for order in orders:
            acc = _chain_f32(a.numpy(), w.numpy(), order)
            z = acc + bias.numpy()                                          # fp32 adds and multiplies, one rounding each
            for got, ref, bound in (
                    (acc, exact, R.dot_bound(K, absacc)),
                    (z, exact + bias.double(), R.dot_bound(K, absacc, bias.double().abs())),
                    (res.numpy() + z, res.double() + exact + bias.double(), R.dot_bound(K, absacc, bias.double().abs(), res.double().abs())),
                    (res.numpy() + gate.numpy() * z, res.double() + gate.double() * (exact + bias.double()),
                     R.dot_bound(K, absacc, bias.double().abs(), res.double().abs(), gate=gate.double()))):
                assert got.dtype == np.float32
                err = (torch.from_numpy(got).double() - ref).abs()
                assert bool((err <= bound).all()), (K, float((err / bound).max()))
        # a chain that leaves the last 16 products out is outside the bound almost everywhere
        short = _chain_f32(a.numpy(), w.numpy(), range(K - 16))
        miss = (torch.from_numpy(short).double() - exact).abs() > R.dot_bound(K, absacc)
        assert float(miss.double().mean()) > 0.99
