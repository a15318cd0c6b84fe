"""GPU: the bf16x3 mode of the Video2Roll frame encoder (split-bf16 operand planes + implicit GEMM for every convolution).

Recipe of test_video2roll_gpu.py: random_video2roll_state_dict(4321), the same synthetic_piano_frames seeds, and the vectors the
REFERENCE module produced (tests/golden/video2roll_{forward,encode}.npz).  Bars: kernels against fp64 torch within 1e-5 of the
output's magnitude, split planes bit-equal to the torch split of the fp32 result; the network at the fp32 mode's bars --
logits 2e-3 abs, probabilities 1e-4 abs, feature taps x1..x4 and x3_ 1e-4 rel / abs.  x2_, x4_ and x5 carry the split
products' error a little past that bar (the 1x1 `toplayer` conv sums 512 channels of magnitude ~1): they are held to
TAP_BAR x the fp32 bar, no looser than 4x the measured worst case of |d| / (1e-4 + 1e-4 |ref|) on an MI355X:
x5 2.53 (|d| 6.2e-4), x2_ 1.07, x4_ 0.83.  Measured beside them: logits 1.4e-4, probabilities 2.0e-5, x1 0.12, x2 0.37,
x3 0.30, x4 0.30, x3_ 0.52; split conv GEMMs 2.3e-6 .. 5.2e-6 of the output's magnitude."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import video2roll_oracle as VO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PARAM_SEED, INPUT_SEED = 4321, 77
TAP_BAR = {"x2_": 4.0, "x4_": 3.0, "x5": 8.0}


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def params():
    from v2a_amd.synth import random_video2roll_state_dict
    return random_video2roll_state_dict(PARAM_SEED)


@pytest.fixture(scope="module")
def eng(params):
    from v2a_amd.video2roll import Video2RollEngine
    return Video2RollEngine(params, DEV, compute="bf16x3", chunk=3)


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


def _split(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


# ------------------------------------------------------------------------------- split GEMM with offset tables
CASES = [(geom, epi, relu) for geom in ((3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0)) for epi in ("store", "resid") for relu in (False, True)]


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_split_gemm_offset_tables_are_a_convolution(L, idx):
    """v2a_gemm, a_dtype V2A_BF16_SPLIT, with a_row_offset / a_ktile_offset / out_row_offset on a zero-bordered split NHWC map ==
    fp64 conv2d of the fp32 map; the split shadow written through out_row_offset is the exact hi / lo split of the output and its
    border stays zero.  The cases cycle through tile_hint 0..4 (0 = by shape; 1..4 = the 64-wide K stage split ring shapes)."""
    (k, stride, pad), epi, relu = CASES[idx]
    hint = idx % 5
    cout = 64 if idx % 2 else 128
    n, H, W, C, b = 3, 9, 14, 64, 1
    g = _g(100 + idx)
    x = torch.randn(n, C, H, W, generator=g)
    w = torch.randn(cout, C, k, k, generator=g) / (C * k * k) ** 0.5
    bias = torch.randn(cout, generator=g)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(n, cout, Ho, Wo, generator=g)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride, pad)
    if epi == "resid":
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    Hp, Wp = H + 2 * b, W + 2 * b
    xp = torch.zeros(2, n, Hp, Wp, C, dtype=torch.bfloat16)
    xp[0, :, b:-b, b:-b], xp[1, :, b:-b, b:-b] = _split(x.permute(0, 2, 3, 1))
    ni, yo, xo = torch.arange(n)[:, None, None], torch.arange(Ho)[None, :, None], torch.arange(Wo)[None, None, :]
    a_row = (((ni * Hp + yo * stride - pad + b) * Wp + xo * stride - pad + b) * C).reshape(-1).int()
    k0 = torch.arange(0, k * k * C, 64)
    a_k = (((k0 // C) // k * Wp + (k0 // C) % k) * C + k0 % C).int()
    assert int(a_row.max()) + int(a_k.max()) + 64 <= xp[0].numel()              # hi-plane extent: the caller's guarantee
    ob = 1
    o_row = ((((ni * (Ho + 2 * ob) + yo + ob) * (Wo + 2 * ob) + xo + ob) * cout).reshape(-1)).int()
    rp = torch.zeros(n, Ho + 2, Wo + 2, cout)
    rp[:, 1:-1, 1:-1] = res.permute(0, 2, 3, 1)
    out = torch.full((n, Ho + 2, Wo + 2, cout), 5.0, device=DEV)
    sh = torch.zeros(2, n, Ho + 2, Wo + 2, cout, device=DEV, dtype=torch.bfloat16)
    wk = w.permute(0, 2, 3, 1).reshape(cout, -1)
    wsplit = torch.cat(_split(wk), 1).contiguous()                               # [W_hi | W_lo], ldw = 2K
    K = k * k * C
    L.gemm([(xp.to(DEV), K, K, xp[0].numel())], wsplit.to(DEV), out, M=n * Ho * Wo, N=cout, compute=L.BF16,
           epilogue=L.EPI_RESID if epi == "resid" else L.EPI_STORE, bias=bias.to(DEV), resid=rp.to(DEV) if epi == "resid" else None,
           relu=relu, ldo=cout, ldr=cout, out_bf16=sh, ld_out_bf16=cout, a_split=True, out_bf16_split=True,
           out_bf16_lo_offset=sh[0].numel(), a_row_offset=a_row.to(DEV), a_ktile_offset=a_k.to(DEV), out_row_offset=o_row.to(DEV),
           tile_hint=hint)
    got = out.cpu()
    inner = got[:, 1:-1, 1:-1]
    err = float((inner.permute(0, 3, 1, 2).double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"\nsplit conv k{k} s{stride} {epi} relu={relu} hint {hint}: max |d| = {err:.3e} ({err / scale:.2e} of max |out|)")
    assert err <= 1e-5 * scale
    assert torch.all(got[:, 0] == 5) and torch.all(got[:, :, 0] == 5) and torch.all(got[:, -1] == 5) and torch.all(got[:, :, -1] == 5)
    s = sh.cpu()
    hi, lo = _split(inner)
    assert torch.equal(s[0, :, 1:-1, 1:-1], hi) and torch.equal(s[1, :, 1:-1, 1:-1], lo)
    border = torch.ones(Ho + 2, Wo + 2, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert torch.all(s[:, :, border] == 0)


# ------------------------------------------------------------------------------- split producers
def test_frames_pack_split_planes(L):
    T, H, W, kh, stride, pad = 6, 20, 37, 11, 2, 4
    frames = torch.rand(T, H, W, generator=_g(21)) * 0.93 + 0.01         # fp32 intensities bf16 alone does not hold
    Wo, Hp = (W + 2 * pad - kh) // stride + 1, H + 2 * pad
    plane = (T + 4) * Wo * Hp * 16
    gap = 64
    buf = torch.full((2 * plane + gap,), 3.0, dtype=torch.bfloat16, device=DEV)
    L.frames_pack_split(frames.to(DEV), buf, lo_offset=plane + gap, T=T, H=H, W=W, kw=kh, stride=stride, pad=pad, Wo=Wo)
    got = buf.cpu()
    fp = F.pad(frames, (pad, pad + 16, pad, pad))                      # zero border (+ slack on the right)
    idx = (torch.arange(T + 4) - 2).clamp(0, T - 1)
    ref = torch.stack([fp[idx][:, :, stride * xo: stride * xo + 16] for xo in range(Wo)], 1).clone()   # (T+4, Wo, Hp, 16)
    ref[..., kh:] = 0
    hi, lo = _split(ref)
    assert torch.equal(got[:plane].view(T + 4, Wo, Hp, 16), hi)
    assert torch.equal(got[plane + gap:].view(T + 4, Wo, Hp, 16), lo)
    assert torch.all(got[plane:plane + gap] == 3)                       # nothing between the planes is written
    assert bool((lo != 0).any())
    plain = torch.empty(plane, dtype=torch.bfloat16, device=DEV)
    L.frames_pack(frames.to(DEV), plain, T=T, H=H, W=W, kw=kh, stride=stride, pad=pad, Wo=Wo)
    assert torch.equal(plain.cpu(), got[:plane])                          # hi plane == the bf16 mode's operand


@pytest.mark.parametrize("cfg", [(3, 2, 1, 0), (2, 2, 0, 1), (3, 1, 0, 1)])
def test_pool2d_split_planes(L, cfg):
    k, stride, pad, mode = cfg
    B, H, W, C = 2, 9, 15, 64
    x = torch.randn(B, C, H, W, generator=_g(9 + k))
    ref = F.max_pool2d(x, k, stride, pad) if mode == 0 else F.avg_pool2d(x, k, stride)
    Ho, Wo = ref.shape[2:]
    xp = torch.full((B, H + 2, W + 2, C), 99.0)                          # a non-zero input border must never be read
    xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    out = torch.zeros(B, Ho + 2, Wo + 2, C, device=DEV)
    sh = torch.zeros(2, B, Ho + 2, Wo + 2, C, device=DEV, dtype=torch.bfloat16)
    L.pool2d_split(xp.to(DEV), out, sh, lo_offset=sh[0].numel(), B=B, H=H, W=W, C_=C, k=k, stride=stride, pad=pad, mode=mode,
                   Ho=Ho, Wo=Wo, in_border=1, out_border=1)
    got = out.cpu()
    torch.testing.assert_close(got[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref, atol=1e-6, rtol=1e-6)
    plain = torch.zeros_like(out)
    L.pool2d(xp.to(DEV), plain, B=B, H=H, W=W, C_=C, k=k, stride=stride, pad=pad, mode=mode, Ho=Ho, Wo=Wo, in_border=1, out_border=1)
    assert torch.equal(plain.cpu(), got)                                 # the fp32 map is the plain kernel's, bit for bit
    s = sh.cpu()
    hi, lo = _split(got[:, 1:-1, 1:-1])
    assert torch.equal(s[0, :, 1:-1, 1:-1], hi) and torch.equal(s[1, :, 1:-1, 1:-1], lo)
    assert torch.all(s[:, :, 0] == 0) and torch.all(s[:, :, -1] == 0) and torch.all(s[:, :, :, 0] == 0) and torch.all(s[:, :, :, -1] == 0)
    assert torch.all(got[:, 0] == 0) and torch.all(got[:, :, -1] == 0)


# ------------------------------------------------------------------------------- whole network vs the reference vectors
def _windows_0_3_6():
    from v2a_amd.synth import synthetic_piano_frames
    return VO.frame_windows(synthetic_piano_frames(1, 7, seed=INPUT_SEED))[[0, 3, 6]]


def test_forward_bf16x3_matches_reference_vectors(eng):
    g = np.load(os.path.join(GOLD, "video2roll_forward.npz"))
    taps = {}
    logits = eng.forward_windows(_windows_0_3_6(), taps).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    print(f"\nvideo2roll bf16x3 vs reference logits: max |d| = {err:.3e} (|logit| max {np.abs(g['logits']).max():.1f})")
    assert err < 2e-3
    for k in ("x1", "x2", "x3", "x4", "x5", "x2_", "x3_", "x4_"):
        a = torch.cat(taps[k], 0).cpu().numpy()
        assert tuple(g[f"{k}_shape"]) == a.shape
        got, ref = a[tuple(g[f"{k}_idx"].T)], g[f"{k}_val"]
        ratio = float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max())
        print(f"  tap {k:4s}: max |d| = {np.abs(got - ref).max():.2e}, {ratio:.2f} x the fp32 bar")
        assert ratio <= TAP_BAR.get(k, 1.0), (k, ratio)
        assert np.abs(a).mean(dtype=np.float64) == pytest.approx(g[f"{k}_stats"][1], rel=1e-4 * TAP_BAR.get(k, 1.0))


@pytest.mark.parametrize("l", [10, 14])
def test_encode_frames_bf16x3_matches_reference_lines(eng, l):
    """The parity bar this mode exists for: probabilities within 1e-4 abs of the reference module's."""
    from v2a_amd.synth import synthetic_piano_frames
    g = np.load(os.path.join(GOLD, "video2roll_encode.npz"))
    x = synthetic_piano_frames(2, 4, seed=INPUT_SEED + 1)
    roll = eng.encode_frames(x, l)
    assert roll.shape == (2, l, 51) and roll.dtype == torch.float32 and roll.is_cuda
    err = float(np.abs(roll.cpu().numpy() - g[f"roll_l{l}"]).max())
    print(f"\nvideo2roll bf16x3 encode_frames l={l} vs reference: max |d p| = {err:.3e}")
    np.testing.assert_allclose(roll.cpu().numpy(), g[f"roll_l{l}"], rtol=0, atol=1e-4)
    if l == 14:
        assert torch.all(roll[:, 12:] == 0)


def test_encode_frames_bf16x3_chunking(params):
    """The chunk size never changes a result bit; rows past 3 t are zero; close to the fp32 CPU restatement."""
    from v2a_amd.synth import synthetic_piano_frames
    from v2a_amd.video2roll import Video2RollEngine
    x = synthetic_piano_frames(1, 9, seed=5)
    a = Video2RollEngine(params, DEV, compute="bf16x3", chunk=4).encode_frames(x, 30)
    b = Video2RollEngine(params, DEV, compute="bf16x3", chunk=9).encode_frames(x, 30)
    assert torch.equal(a, b)
    assert torch.all(a[:, 27:] == 0)
    with torch.no_grad():
        ref = VO.encode_frames(params, x, 30)
    err = float((a.cpu() - ref).abs().max())
    print(f"\nvideo2roll bf16x3 encode_frames vs CPU restatement: max {err:.3e}")
    assert err < 1e-4


# ------------------------------------------------------------------------------- E2TTS wiring
def test_e2tts_frames_compute_dtype(small, params):
    from conftest import make_model
    from v2a_amd.synth import synthetic_piano_frames
    cfg, P = small["cfg"], small["P"]
    g = np.load(os.path.join(GOLD, "video2roll_encode.npz"))
    x = synthetic_piano_frames(2, 4, seed=INPUT_SEED + 1)
    v2r = {"video2roll_net." + k: v for k, v in params.items()}
    m = make_model(cfg, P, "bf16x3", frames_compute_dtype="bf16x3")
    m.load_state_dict({**P, **v2r}, strict=True)
    np.testing.assert_allclose(m.encode_frames(x, 10).cpu().numpy(), g["roll_l10"], rtol=0, atol=1e-4)
    assert m._v2r.compute == "bf16x3"
    d = make_model(cfg, P, "bf16x3")                                   # no keyword: today's encoder mode
    d.load_state_dict({**P, **v2r}, strict=True)
    d.encode_frames(x, 10)
    assert d._v2r.compute == "fp32"
