"""CPU: the bf16x3 mode of the Video2Roll encoder answers its argument checks before any HIP call -- the engine and E2TTS
refuse unknown modes, v2a_gemm refuses split operands with offset tables on the shapes that cannot take them and a split
shadow (out_bf16_split) on the launches whose scalar epilogue could not write its lo plane, the split
producers (v2a_frames_pack_split, v2a_pool2d_split) refuse null pointers and bad geometry, and the CLI's --frames-dtype
reaches E2TTS."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


def test_engine_rejects_unknown_compute(L):
    from v2a_amd.video2roll import Video2RollEngine
    with pytest.raises(ValueError, match="bf16x3"):
        Video2RollEngine({}, "cpu", compute="x")


def test_e2tts_rejects_unknown_frames_compute_dtype():
    import v2a_amd
    tk = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
              if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True)
    with pytest.raises(ValueError, match="frames_compute_dtype"):
        v2a_amd.E2TTS(transformer=tk, num_channels=16, frames_compute_dtype="x")
    m = v2a_amd.E2TTS(transformer=tk, num_channels=16, compute_dtype="bf16x3")
    assert m._frames_compute == "fp32"                       # no keyword: today's mapping
    assert v2a_amd.E2TTS(transformer=tk, num_channels=16, compute_dtype="bf16")._frames_compute == "bf16"
    assert v2a_amd.E2TTS(transformer=tk, num_channels=16, frames_compute_dtype="bf16x3")._frames_compute == "bf16x3"


def _split_conv_args(L, *, tile_hint=0, a_lo_offset=1 << 20):
    """A split-operand implicit-GEMM convolution whose pointers are never dereferenced (the call must fail on the host)."""
    g = L.GemmArgs()
    p = 1 << 16                                              # aligned dummy device address
    g.a[0], g.lda[0], g.ka[0], g.nseg = p, 576, 576, 1
    g.a_dtype, g.compute_dtype = L.BF16_SPLIT, L.BF16
    g.w, g.ldw = p, 2 * 576
    g.M, g.N = 4096, 128
    g.epilogue, g.out, g.ldo, g.out_dtype = L.EPI_STORE, p, 128, L.F32
    g.a_row_offset, g.a_ktile_offset = p, p
    g.a_lo_offset[0] = a_lo_offset
    g.tile_hint = tile_hint
    return g


@pytest.mark.parametrize("hint", [5, 6, 7])
def test_split_gemm_with_tables_refuses_other_tile_shapes(L, hint):
    g = _split_conv_args(L, tile_hint=hint)
    assert L.lib().v2a_gemm(ctypes.byref(g), None) == -1    # V2A_ERR_ARG
    msg = L.lib().v2a_last_error().decode()
    assert "tile_hint %d" % hint in msg and "offset tables" in msg, msg


def test_split_gemm_with_tables_needs_a_lo_offset(L):
    g = _split_conv_args(L, a_lo_offset=0)
    assert L.lib().v2a_gemm(ctypes.byref(g), None) == -1
    assert "a_lo_offset" in L.lib().v2a_last_error().decode()
    g = _split_conv_args(L, a_lo_offset=12)                  # not a multiple of 8
    assert L.lib().v2a_gemm(ctypes.byref(g), None) == -1
    assert "a_lo_offset" in L.lib().v2a_last_error().decode()


def test_split_shadow_with_out_row_offset_needs_lo_offset(L):
    g = _split_conv_args(L, tile_hint=5)                     # would be refused later anyway: the shadow check answers first
    g.out_bf16, g.ld_out_bf16, g.out_bf16_split = 1 << 16, 128, 1
    g.out_row_offset = 1 << 16
    assert L.lib().v2a_gemm(ctypes.byref(g), None) == -1
    assert "out_bf16_lo_offset" in L.lib().v2a_last_error().decode()


def _dense_shadow_args(L, *, compute, a_dtype, epilogue=None):
    """A dense GEMM with an out_bf16 shadow whose pointers are never dereferenced: every check but the one under test passes."""
    g = L.GemmArgs()
    p = 1 << 16
    g.a[0], g.lda[0], g.ka[0], g.nseg = p, 128, 128, 1
    g.a_dtype, g.compute_dtype = a_dtype, compute
    g.w, g.ldw = p, 128
    g.M, g.N = 256, 128
    g.epilogue = L.EPI_STORE if epilogue is None else epilogue
    g.out, g.ldo, g.out_dtype = p, 128, L.F32
    g.out_bf16, g.ld_out_bf16, g.out_bf16_split = p, 256, 1
    return g


@pytest.mark.parametrize("case", ["fp32 compute", "fp32 A on bf16 compute", "bf16 SIGMOID", "unaligned shadow rows"])
def test_split_shadow_refused_where_the_scalar_epilogue_runs(L, case):
    """out_bf16_split on a launch whose epilogue writes bf16(v) alone would leave the lo plane unwritten and report success: refused on the host."""
    g = {"fp32 compute": lambda: _dense_shadow_args(L, compute=L.F32, a_dtype=L.F32),
         "fp32 A on bf16 compute": lambda: _dense_shadow_args(L, compute=L.BF16, a_dtype=L.F32),
         "bf16 SIGMOID": lambda: _dense_shadow_args(L, compute=L.BF16, a_dtype=L.BF16, epilogue=L.EPI_SIGMOID),
         "unaligned shadow rows": lambda: _dense_shadow_args(L, compute=L.BF16, a_dtype=L.BF16)}[case]()
    if case == "unaligned shadow rows":
        g.out_bf16 = (1 << 16) + 2                           # not 8-byte aligned: the ring kernel would fall back to the scalar epilogue
    assert L.lib().v2a_gemm(ctypes.byref(g), None) == -1    # V2A_ERR_ARG
    msg = L.lib().v2a_last_error().decode()
    assert "out_bf16_split" in msg and "lo plane" in msg, msg


def test_frames_pack_split_refuses_bad_args(L):
    lib, p = L.lib(), 1 << 16
    T, H, W, kw, stride, pad = 6, 20, 37, 11, 2, 4
    Wo = (W + 2 * pad - kw) // stride + 1
    plane = (T + 4) * Wo * (H + 2 * pad) * 16
    assert lib.v2a_frames_pack_split(None, p, plane, T, H, W, kw, stride, pad, Wo, None) == -1
    assert "null" in lib.v2a_last_error().decode()
    assert lib.v2a_frames_pack_split(p, None, plane, T, H, W, kw, stride, pad, Wo, None) == -1
    assert "null" in lib.v2a_last_error().decode()
    assert lib.v2a_frames_pack_split(p, p, plane, T, H, W, kw, stride, pad, Wo + 1, None) == -1
    assert "Wo" in lib.v2a_last_error().decode()
    assert lib.v2a_frames_pack_split(p, p, plane, T, H, W, 17, stride, pad, Wo, None) == -1
    assert "geometry" in lib.v2a_last_error().decode()
    assert lib.v2a_frames_pack_split(p, p, plane - 8, T, H, W, kw, stride, pad, Wo, None) == -1      # lo plane overlaps hi
    assert "lo_offset" in lib.v2a_last_error().decode()
    assert lib.v2a_frames_pack_split(p, p + 2, plane, T, H, W, kw, stride, pad, Wo, None) == -1
    assert "alignment" in lib.v2a_last_error().decode()


def test_pool2d_split_refuses_bad_args(L):
    lib, p = L.lib(), 1 << 16
    B, H, W, C = 2, 9, 15, 64
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    plane = B * (Ho + 2) * (Wo + 2) * C
    ok = (B, H, W, C, 3, 2, 1, 0, Ho, Wo, 1, 1, None)
    assert lib.v2a_pool2d_split(p, p + 64, None, plane, *ok) == -1
    assert "null" in lib.v2a_last_error().decode()
    assert lib.v2a_pool2d_split(p, p, p, plane, *ok) == -1                   # aliased
    assert "aliased" in lib.v2a_last_error().decode()
    assert lib.v2a_pool2d_split(p, p + 64, p, plane - 4, *ok) == -1          # lo plane overlaps hi
    assert "lo_offset" in lib.v2a_last_error().decode()
    assert lib.v2a_pool2d_split(p, p + 64, p, plane, B, H, W, C, 3, 2, 1, 0, Ho + 1, Wo, 1, 1, None) == -1
    assert "Ho/Wo" in lib.v2a_last_error().decode()
    assert lib.v2a_pool2d_split(p, p + 64, p, plane, B, H, W, 6, 3, 2, 1, 0, Ho, Wo, 1, 1, None) == -1
    assert "geometry" in lib.v2a_last_error().decode()


def test_cli_frames_dtype_reaches_e2tts(monkeypatch, tmp_path):
    import v2a_amd
    from v2a_amd import cli
    seen = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(v2a_amd, "E2TTS", fake)
    args = [str(tmp_path / "ck.pt"), "0", str(tmp_path / "l.scp"), "0", "1", str(tmp_path / "o"), "--piano"]
    for extra, want in (([], None), (["--frames-dtype", "bf16x3"], "bf16x3"), (["--frames-dtype", "bf16"], "bf16")):
        with pytest.raises(Stop):
            cli.main(args + extra)
        assert seen[-1]["frames_compute_dtype"] == want
    with pytest.raises(SystemExit):
        cli.main(args + ["--frames-dtype", "fp16"])
