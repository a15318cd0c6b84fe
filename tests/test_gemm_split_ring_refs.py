"""CPU: the float64 reference helpers of tests/test_gemm_split_ring_gpu.py against torch and against each other -- a wrong helper would either
fail every GPU case or, worse, agree with a kernel that is wrong in the same way."""
import torch

import test_gemm_split_ring_gpu as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_split_planes_is_the_library_rule_and_keeps_16_bits():
    from v2a_amd import _lib
    x = torch.randn(37, 64, generator=_g(1)) * 3
    p = R._split_planes(x)
    assert p.dtype == torch.bfloat16 and p.shape == (37, 128)
    assert torch.equal(p, _lib.split_planes(x))
    assert torch.equal(p[:, :64], x.bfloat16())
    back = p[:, :64].double() + p[:, 64:].double()
    assert float(((back - x.double()).abs() / x.double().abs()).max()) <= 2.0 ** -16


def test_rope_ref_is_a_complex_rotation_by_the_table_row():
    M, N, rope_cols, rpb, off = 61, 208, 128, 23, 5
    z = torch.randn(M, N, generator=_g(2)).double()
    tab = R._rope_table(off + rpb)
    got = R._rope_ref(z, tab, rope_cols, rpb, off)
    assert torch.equal(got[:, rope_cols:], z[:, rope_cols:])                 # columns behind the heads pass through
    # the table is (cos, sin) of position * 10000^(-2i / 64)
    ang = torch.arange(off + rpb).double()[:, None] / 10000 ** (torch.arange(0, 64, 2).double() / 64)
    torch.testing.assert_close(tab.double(), torch.stack((ang.cos(), ang.sin()), -1), rtol=0, atol=2e-6)
    # element by element: pair i of head h of row m times (cos + i sin) of position m % rpb + off
    rot = torch.view_as_complex(tab.double())                                # (positions, 32)
    zc = torch.view_as_complex(z[:, :rope_cols].reshape(M, rope_cols // 64, 32, 2).contiguous())
    pos = torch.tensor([m % rpb + off for m in range(M)])
    want = torch.view_as_real(zc * rot[pos][:, None, :]).reshape(M, rope_cols)
    torch.testing.assert_close(got[:, :rope_cols], want, rtol=0, atol=1e-14)
    assert int(pos.max()) == off + rpb - 1 and int(pos[rpb]) == off           # the positions wrap, and reach the table's last row


def test_glu_unpack_inverts_the_row_permutation():
    M, N, K = 9, 96, 32
    a = torch.randn(M, K, generator=_g(3)).double()
    w = torch.randn(N, K, generator=_g(4)).double()                          # [N / 2 value rows | N / 2 gate rows]
    perm = R._glu_perm(N)
    assert sorted(perm.tolist()) == list(range(N))
    assert perm[:32].tolist() == list(range(16)) + list(range(48, 64))
    v, gt = R._glu_unpack(a @ w[perm].t())
    z = a @ w.t()
    assert torch.equal(v, z[:, :N // 2]) and torch.equal(gt, z[:, N // 2:])
    # ... which makes value * act(gate) torch's own GLU forms on the unpermuted halves
    torch.testing.assert_close(v * torch.sigmoid(gt), torch.nn.functional.glu(z, -1), rtol=0, atol=1e-15)


def test_gate_and_gamma_rows_against_loops():
    M, N, rpb, sw, steps, step = 53, 8, 23, 30, 4, 2
    B = (M + rpb - 1) // rpb
    gate = torch.randn(steps, B, N, generator=_g(5))
    gam = torch.randn(steps, B, 2, N, generator=_g(6))
    gr, gm = R._gate_rows(gate, step, M, rpb), R._gamma_rows(gam, step, M, rpb, sw)
    assert gr.shape == (M, N) and gm.shape == (M, N)
    for m in range(M):
        assert torch.equal(gr[m], gate[step, m // rpb])
        assert torch.equal(gm[m], gam[step, m // rpb, 1 if m >= sw else 0])
    # as the kernel addresses them: base + step * step stride + batch * batch stride (+ switch offset), in elements
    flat, m = gam.reshape(-1), 47
    at = step * gam.stride(0) + (m // rpb) * gam.stride(1) + gam.stride(2)
    assert torch.equal(gm[m], flat[at:at + N])


def test_planes_sum_and_shadow_check():
    x = torch.randn(11, 32, generator=_g(7))
    p = R._split_planes(x)
    assert torch.equal(R._planes_sum(torch.cat([p, p], 1), 32), p[:, :32].double() + p[:, 32:].double())
    R._assert_shadow(p, x)
