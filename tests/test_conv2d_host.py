"""CPU: the conv-as-GEMM host layer that video2roll.py and roll2midi.py share (conv2d.py): the offset tables of the implicit GEMM
stay inside their maps and gather a convolution's patch matrix -- for Roll2Midi's channel-slice geometry and for every geometry of
the Video2Roll network -- and the bordered map with its slices.  No GPU is touched."""
import pytest
import torch
import torch.nn.functional as F

from v2a_amd.conv2d import ConvMemory, Map, conv_tables, fold_batchnorm, gemm_weight, split_args


def slice_tables(n, H, W, sp, so, ci, dp, border=1):
    """Roll2Midi's geometry: 3x3 / stride 1 / pad 1 from a channel slice into a map of the same pixel grid and border."""
    return conv_tables(n, H, W, border, sp, so, ci, 3, 3, 1, 1, H, W, dp, border)


def test_slice_tables_stay_inside_the_map_and_are_a_convolution():
    n, H, W, sp, so, ci, dp = 2, 5, 3, 192, 64, 128, 384
    a_row, a_k, o_row = slice_tables(n, H, W, sp, so, ci, dp)
    Hp, Wp = H + 2, W + 2
    assert a_row.dtype == a_k.dtype == o_row.dtype == torch.int32
    assert a_row.shape == o_row.shape == (n * H * W,) and a_k.shape == (9 * ci // 64,)
    assert int(a_row.min()) >= 0 and so + int(a_row.max()) + int(a_k.max()) + 64 <= n * Hp * Wp * sp
    assert int(o_row.max()) + dp <= n * Hp * Wp * dp
    assert all(int(v) % 8 == 0 for t in (a_row, a_k, o_row) for v in t)
    # gathering through the tables is the convolution's patch matrix of the slice
    g = torch.Generator().manual_seed(1)
    m = torch.zeros(n, Hp, Wp, sp, dtype=torch.float64)
    m[:, 1:-1, 1:-1] = torch.randn(n, H, W, sp, generator=g, dtype=torch.float64)
    flat = m.view(-1)[so:]
    idx = a_row[:, None, None].long() + a_k[None, :, None].long() + torch.arange(64)[None, None, :]
    patch = flat[idx].reshape(n * H * W, 9 * ci)
    w = torch.randn(4, ci, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(m[:, 1:-1, 1:-1, so:so + ci].permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, 4)
    assert torch.allclose(patch @ w.permute(0, 2, 3, 1).reshape(4, -1).t(), ref, atol=1e-10)
    # output rows are the interior pixels of the destination map
    dst = torch.zeros(n, Hp, Wp, dp)
    dst.view(-1)[o_row.long()] = 1
    assert int(dst.sum()) == n * H * W and float(dst[:, 1:-1, 1:-1, 0].sum()) == n * H * W
    with pytest.raises(AssertionError):
        slice_tables(n, H, W, sp, 128, ci, dp)                      # the slice would leave the map's channels
    with pytest.raises(AssertionError):
        slice_tables(n, H, W, sp, so, ci, dp, border=0)             # the border must cover the padding


# (kh, stride, pad) of the Video2Roll network's NHWC convolutions: the 3x3 of the blocks and FTBs, the strided 3x3 and 1x1 downsample
# of a layer's first block, the toplayer's 1x1 and the FTB's 1x1 with padding 1 (output (H + 2) x (W + 2): the border is convolved too)
V2R_GEOMETRIES = {"3x3": (3, 1, 1), "3x3/s2": (3, 2, 1), "1x1/s2": (1, 2, 0), "1x1": (1, 1, 0), "1x1/pad1": (1, 1, 1)}


@pytest.mark.parametrize("dst_border", [0, 1])
@pytest.mark.parametrize("ci", [64, 128])
@pytest.mark.parametrize("geom", sorted(V2R_GEOMETRIES))
def test_video2roll_tables_stay_inside_the_map_and_are_a_convolution(geom, ci, dst_border):
    k, stride, pad = V2R_GEOMETRIES[geom]
    n, H, W, co, b = 2, 5, 4, 64, 1
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    a_row, a_k, o_row = conv_tables(n, H, W, b, ci, 0, ci, k, k, stride, pad, Ho, Wo, co, dst_border)
    Hp, Wp = H + 2 * b, W + 2 * b
    assert a_row.dtype == a_k.dtype == torch.int32
    assert a_row.shape == (n * Ho * Wo,) and a_k.shape == (k * k * ci // 64,)
    assert int(a_row.min()) >= 0 and int(a_row.max()) + int(a_k.max()) + 64 <= n * Hp * Wp * ci
    assert all(int(v) % 8 == 0 for t in (a_row, a_k) for v in t)
    # gathering through the tables is the convolution's patch matrix, in float64
    g = torch.Generator().manual_seed(2)
    m = torch.zeros(n, Hp, Wp, ci, dtype=torch.float64)
    m[:, b:-b, b:-b] = torch.randn(n, H, W, ci, generator=g, dtype=torch.float64)
    idx = a_row[:, None, None].long() + a_k[None, :, None].long() + torch.arange(64)[None, None, :]
    patch = m.view(-1)[idx].reshape(n * Ho * Wo, k * k * ci)
    w = torch.randn(4, ci, k, k, generator=g, dtype=torch.float64)
    ref = F.conv2d(m[:, b:-b, b:-b].permute(0, 3, 1, 2), w, stride=stride, padding=pad)
    assert ref.shape == (n, 4, Ho, Wo)
    assert torch.allclose(patch @ gemm_weight(w).t(), ref.permute(0, 2, 3, 1).reshape(-1, 4), atol=1e-10)
    if dst_border == 0:
        assert o_row is None                                        # dense output rows: the GEMM's own row pitch
        return
    # output rows are the interior pixels of the bordered destination map, in order
    assert o_row.dtype == torch.int32 and o_row.shape == (n * Ho * Wo,)
    dst = torch.zeros(n, Ho + 2, Wo + 2, co)
    assert int(o_row.max()) + co <= dst.numel()
    dst.view(-1)[o_row.long()] = torch.arange(1, n * Ho * Wo + 1, dtype=torch.float32)
    assert torch.equal(dst[:, 1:-1, 1:-1, 0].reshape(-1), torch.arange(1, n * Ho * Wo + 1, dtype=torch.float32))
    assert int((dst != 0).sum()) == n * Ho * Wo
    with pytest.raises(AssertionError):
        conv_tables(n, H, W, pad - 1, ci, 0, ci, k, k, stride, pad, Ho, Wo, co, dst_border)      # the border must cover the padding


def test_map_slices_share_memory_and_the_cache_keys_on_full_geometry():
    mem = ConvMemory(torch.device("cpu"), split=True)
    u = mem.map("u", 2, 5, 3, 192, border=1, shadow=True)
    assert mem.map("u", 2, 5, 3, 192, border=1, shadow=True) is u
    assert mem.map("u", 2, 5, 3, 192, border=0, shadow=True).f32.data_ptr() != u.f32.data_ptr()        # another geometry, other memory
    assert (u.n, u.H, u.W, u.C, u.pitch, u.off, u.border) == (2, 5, 3, 192, 192, 0, 1)
    assert u.sh.shape == (2, 2, 7, 5, 192) and u.plane == u.lo == 2 * 7 * 5 * 192
    d = u.slice(64, 128)
    assert (d.C, d.off, d.pitch, d.lo) == (128, 64, 192, u.lo) and d.f32 is u.f32 and d.sh is u.sh
    assert d.base().data_ptr() == u.f32.data_ptr() + 64 * 4 and d.shadow().data_ptr() == u.sh.data_ptr() + 64 * 2
    op = d.operand(9 * 128)
    assert op.t.data_ptr() == d.shadow().data_ptr() and op[1:] == (9 * 128, 9 * 128, u.lo)
    u.f32[:, 1:-1, 1:-1] = torch.arange(2 * 5 * 3 * 192, dtype=torch.float32).view(2, 5, 3, 192)
    assert torch.equal(d.nchw(), u.f32[:, 1:-1, 1:-1, 64:].permute(0, 3, 1, 2)) and d.interior(16).shape == (2, 5, 3, 16)
    assert split_args(True, d) == dict(a_split=True, out_bf16_split=True, out_bf16_lo_offset=u.lo)
    plain = Map(torch.zeros(2, 5, 3, 64), None, 5, 3)                # a wrapped buffer: no border, no shadow
    assert (plain.border, plain.lo, plain.shadow()) == (0, 0, None)
    assert split_args(True, plain) == split_args(True) == dict(a_split=True) and split_args(False, d) == {}
    with pytest.raises(AssertionError):
        u.slice(128, 128)                                            # the slice would leave the map's channels
    t = mem.tables(d, u.slice(0, 64), 3, 3, 1, 1)
    assert mem.tables(u.slice(64, 128), u.slice(0, 64), 3, 3, 1, 1) is t
    assert all(torch.equal(a, b) for a, b in zip(t, conv_tables(2, 5, 3, 1, 192, 64, 128, 3, 3, 1, 1, 5, 3, 192, 1)))
    c = mem.col(10, 32)
    assert c.shape == (10, 32) and mem.col(5, 32).data_ptr() == c.data_ptr() and mem.col(5, 32, 1).data_ptr() != c.data_ptr()


def test_fold_batchnorm_is_the_eval_mode_batchnorm_behind_the_convolution():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 6, 5, generator=g, dtype=torch.float64)
    w, bias = torch.randn(4, 3, 3, 3, generator=g), torch.randn(4, generator=g)
    gamma, beta, mean = (torch.randn(4, generator=g) for _ in range(3))
    var = torch.rand(4, generator=g) + 0.5
    for b0 in (None, bias):
        wf, bf = fold_batchnorm(w, b0, gamma, beta, mean, var, 0.8)
        assert wf.dtype == bf.dtype == torch.float32
        ref = F.batch_norm(F.conv2d(x, w.double(), None if b0 is None else b0.double(), padding=1), mean.double(), var.double(),
                           gamma.double(), beta.double(), False, 0.0, 0.8)
        # fp32 roundings of the scale, the scaled weight and the shift, 2^-24 relative each, over 27 taps with |x w s| < 10
        assert torch.allclose(F.conv2d(x, wf.double(), bf.double(), padding=1), ref, rtol=0, atol=1e-4)
