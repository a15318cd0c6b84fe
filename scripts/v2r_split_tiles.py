#!/usr/bin/env python3
"""Time the split-operand implicit-GEMM convolutions of the bf16x3 Video2Roll encoder on each accepted tile shape
(tile_hint 1..4, and 0 = the library's choice) -- the measurement behind v2a_gemm's tile rule for split operands with offset
tables.  Shapes: the NHWC convolutions of one 251-frame clip in one pass (100 x 900 frames).
usage: python scripts/v2r_split_tiles.py [windows=251]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import v2a_amd  # noqa: E402,F401
from v2a_amd import _lib as L  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 251
# (label, H, W, C_in, k, stride, pad, C_out) of the source map
SHAPES = [("layer1 3x3 64", 25, 225, 64, 3, 1, 1, 64), ("layer2.0 3x3/2", 25, 225, 64, 3, 2, 1, 128),
          ("layer2 3x3 128", 13, 113, 128, 3, 1, 1, 128), ("FTB2 conv0 1x1p1", 13, 113, 128, 1, 1, 1, 128),
          ("layer3.0 3x3/2", 13, 113, 128, 3, 2, 1, 256), ("layer3 3x3 256", 7, 57, 256, 3, 1, 1, 256),
          ("FTB3 3x3 128", 9, 59, 128, 3, 1, 1, 128), ("layer4.0 3x3/2", 7, 57, 256, 3, 2, 1, 512),
          ("layer4 3x3 512", 4, 29, 512, 3, 1, 1, 512), ("FTB4 conv0 1x1p1", 4, 29, 512, 1, 1, 1, 128)]
for label, H, W, C, k, stride, pad, co in SHAPES:
    b = 1
    Hp, Wp = H + 2 * b, W + 2 * b
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = torch.randn(2, n, Hp, Wp, C, device="cuda").to(torch.bfloat16)
    ni = torch.arange(n, device="cuda")[:, None, None]
    yo, xo = torch.arange(Ho, device="cuda")[None, :, None], torch.arange(Wo, device="cuda")[None, None, :]
    a_row = (((ni * Hp + yo * stride - pad + b) * Wp + xo * stride - pad + b) * C).reshape(-1).int()
    k0 = torch.arange(0, k * k * C, 64, device="cuda")
    a_k = (((k0 // C) // k * Wp + (k0 // C) % k) * C + k0 % C).int()
    assert int(a_row.max()) + int(a_k.max()) + 64 <= x[0].numel() < 2 ** 31
    o_row = ((((ni * (Ho + 2) + yo + 1) * (Wo + 2) + xo + 1) * co).reshape(-1)).int()
    out = torch.zeros(n, Ho + 2, Wo + 2, co, device="cuda")
    sh = torch.zeros(2, n, Ho + 2, Wo + 2, co, device="cuda", dtype=torch.bfloat16)
    K = k * k * C
    w = torch.randn(co, 2 * K, device="cuda").to(torch.bfloat16)
    bias = torch.zeros(co, device="cuda")
    M = n * Ho * Wo
    res = []
    for hint in (0, 1, 2, 3, 4):
        call = lambda: L.gemm([(x, K, K, x[0].numel())], w, out, M=M, N=co, compute=L.BF16, epilogue=L.EPI_RESID, bias=bias, resid=out,
                              relu=True, ldo=co, ldr=co, out_bf16=sh, ld_out_bf16=co, a_split=True, out_bf16_split=True,
                              out_bf16_lo_offset=sh[0].numel(), a_row_offset=a_row, a_ktile_offset=a_k, out_row_offset=o_row, tile_hint=hint)
        call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        res.append(f"hint{hint} {ms * 1e3:8.1f} us {6.0 * M * co * K / ms / 1e9:6.0f} TF/s")
    print(f"{label:18s} M={M:8d} N={co:3d} K={K:4d}: " + " | ".join(res), flush=True)
    del x, out, sh, w
    torch.cuda.empty_cache()
