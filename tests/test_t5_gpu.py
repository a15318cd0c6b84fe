"""GPU: the FLAN-T5 prompt encoder kernels against float64 torch, run-to-run bit equality, the whole encoder against the
transformers fixtures of scripts/make_golden_t5.py, and E2TTS.sample / transformer_with_pred_head with prompt=."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _twice(fn, out):
    fn()
    a = out.clone()
    fn()
    torch.cuda.synchronize()
    assert torch.equal(a, out), "not bit-equal on a second run"
    return a


@pytest.mark.parametrize("gather", [False, True])
def test_t5_rmsnorm(gather):
    from v2a_amd import _lib as L
    d, rows, V, eps = 1024, 37, 300, 1e-6
    x = (3.0 * torch.randn(V if gather else rows, d, generator=_g(1))).to(DEV)
    w = (1 + 0.1 * torch.randn(d, generator=_g(2))).to(DEV)
    ids = torch.randint(0, V, (rows,), generator=_g(3), dtype=torch.int32).to(DEV)
    y = torch.empty(rows, d, device=DEV)
    res = torch.empty(rows, d, device=DEV)
    kw = dict(ids=ids, vocab=V, resid=res) if gather else {}
    got = _twice(lambda: L.t5_rmsnorm(x, y, w, rows=rows, d=d, eps=eps, **kw), y)
    xr = (x[ids.long()] if gather else x).double()
    ref = w.double() * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps))
    assert float((got.double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())
    if gather:
        assert torch.equal(res, x[ids.long()])


def _attn_ref(q, k, v, bias, mask, N):
    """q/k/v (B, N, H, 64) float64; bias (H, 2N-1); mask (B, N)."""
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    idx = torch.arange(N)[None, :] - torch.arange(N)[:, None] + N - 1
    s = s + bias[:, idx][None]
    s = s.masked_fill(~mask.bool()[:, None, None, :], float("-inf"))
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), v)


@pytest.mark.parametrize("N", [1, 7, 64, 200, 512])
def test_t5_attention(N):
    from v2a_amd import _lib as L
    B, H, inner = 3, 16, 1024
    qkv = (2.0 * torch.randn(B * N, 3 * inner, generator=_g(N))).to(DEV)
    bias = torch.randn(H, 2 * N - 1, generator=_g(N + 1)).to(DEV)
    mask = torch.zeros(B, N, dtype=torch.int32)
    mask[0] = 1                                                    # all valid
    mask[1, :max(1, (2 * N) // 3)] = 1                             # ragged prefix
    mask[2] = (torch.rand(N, generator=_g(N + 2)) < 0.5).int()     # non-prefix
    mask[2, N // 2] = 1
    out = torch.empty(B * N, inner, device=DEV)
    md = mask.to(DEV)
    got = _twice(lambda: L.t5_attention(qkv, out, bias, md, B=B, H=H, N=N, inner=inner), out)
    t = qkv.double().cpu().view(B, N, 3, H, 64)
    ref = _attn_ref(t[:, :, 0], t[:, :, 1], t[:, :, 2], bias.double().cpu(), mask, N).reshape(B * N, inner)
    err = float((got.double().cpu() - ref).abs().max())
    assert err < 2e-5 * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("K", [128, 1024, 2816])
@pytest.mark.parametrize("M", [1, 17, 64, 128, 300, 512])
def test_gemm_skinny(M, K):
    from v2a_amd import _lib as L
    from v2a_amd.t5 import pack_geglu
    N = 256
    a = torch.randn(M, K, generator=_g(M * 7 + K)).to(DEV)
    w = (torch.randn(2 * N, K, generator=_g(K)) / math.sqrt(K)).to(DEV)
    resid = torch.randn(M, N, generator=_g(5)).to(DEV)
    ref = a.double() @ w.double().t()
    scale = 4e-6 * max(1.0, math.sqrt(K / 128))
    # STORE
    out = torch.empty(M, 2 * N, device=DEV)
    got = _twice(lambda: L.gemm_skinny(a, w, out, M=M, N=2 * N, K=K), out)
    assert float((got.double() - ref).abs().max()) < scale * float(ref.abs().max())
    # RESID, in place on the residual stream (resid aliases out)
    h0 = resid.clone()
    h = resid.clone()

    def resid_step():
        h.copy_(h0)
        L.gemm_skinny(a, w[:N], h, M=M, N=N, K=K, epilogue=L.EPI_RESID, resid=h)
    got = _twice(resid_step, h)
    assert float((got.double() - (resid.double() + ref[:, :N])).abs().max()) < scale * float(ref.abs().max()) + 1e-6
    # GEGLU_TANH: value = second half rows, gate = first half rows, packed
    wp = pack_geglu(w[:N], w[N:]).contiguous()
    gout = torch.empty(M, N, device=DEV)
    got = _twice(lambda: L.gemm_skinny(a, wp, gout, M=M, N=2 * N, K=K, epilogue=L.EPI_GEGLU_TANH), gout)
    gg, vv = ref[:, :N], ref[:, N:]
    gref = vv * (0.5 * gg * (1 + torch.tanh(math.sqrt(2 / math.pi) * (gg + 0.044715 * gg ** 3))))
    assert float((got.double() - gref).abs().max()) < 2 * scale * float(ref.abs().max()) ** 2 + 1e-6


def test_gemm_skinny_rows_do_not_change_bits():
    """The same output row comes out with the same bits whatever M (and so the tile shape) the launch has."""
    from v2a_amd import _lib as L
    K, N = 1024, 3072
    a = torch.randn(300, K, generator=_g(9)).to(DEV)
    w = (torch.randn(N, K, generator=_g(10)) / 32).to(DEV)
    outs = []
    for M in (1, 17, 64, 300):
        o = torch.empty(M, N, device=DEV)
        L.gemm_skinny(a, w, o, M=M, N=N, K=K)
        outs.append(o[:1].clone())
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


_ENCODERS = {}


def _encoder(name):
    from v2a_amd.synth import random_t5_encoder_state_dict
    from v2a_amd.t5 import T5Encoder
    if name not in _ENCODERS:
        _ENCODERS.clear()
        fx = dict(np.load(os.path.join(GOLDEN, f"t5_{name}.npz")))
        meta = json.loads(str(fx["meta"]))
        sd = random_t5_encoder_state_dict(meta["config"], meta["weight_seed"], meta["amplify"])
        _ENCODERS[name] = (T5Encoder(sd, DEV), fx, meta)
    return _ENCODERS[name]


@pytest.mark.parametrize("name", ["small", "full", "amplified"])
def test_encoder_matches_transformers_fixture(name):
    enc, fx, meta = _encoder(name)
    for bi in range(len(meta["batches"])):
        p = f"b{bi}_"
        taps = {l: None for l in meta["taps"]}
        hid, mask = enc.encode_ids(torch.from_numpy(fx[p + "ids"]), torch.from_numpy(fx[p + "mask"]), taps=taps)
        rows = torch.from_numpy(fx[p + "rows"]).long()
        err = float((hid[:, rows].cpu().double() - torch.from_numpy(fx[p + "out"]).double()).abs().max())
        tap_err = {}
        for l in meta["taps"]:
            ref = torch.from_numpy(fx[p + f"tap{l}"]).double()
            tap_err[l] = float((taps[l][:, rows].cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(f"t5 {name} batch {bi}: max |d out| {err:.3e}; tap rel errors {tap_err}")
        assert torch.equal(mask.cpu(), torch.from_numpy(fx[p + "mask"]).bool())
        assert all(e <= 1e-4 for e in tap_err.values()), tap_err
        assert err <= 1e-4, err


def _small_t5_with_stub():
    enc, fx, meta = _encoder("small")
    ids, mask = fx["b0_ids"], fx["b0_mask"]
    prompts = ["prompt %d" % i for i in range(ids.shape[0])]
    table = {p: ids[i, :mask[i].sum()].tolist() for i, p in enumerate(prompts)}
    table["the sound of X X"] = [5, 7, 9, 11, 13, 1]

    class Tok:
        model_max_length = 512

        def __call__(self, ps, max_length, padding, truncation, return_tensors):
            rows = [table[p] for p in ps]
            n = max(map(len, rows))
            return dict(input_ids=torch.tensor([r + [0] * (n - len(r)) for r in rows]),
                        attention_mask=torch.tensor([[1] * len(r) + [0] * (n - len(r)) for r in rows]))
    enc.tokenizer = Tok()
    return enc, prompts, fx


def test_sample_with_prompt_matches_precomputed_context(small):
    enc, prompts, fx = _small_t5_with_stub()
    cfg, P = small["cfg"], small["P"]
    m = make_model(cfg, P, "fp32", device=DEV)
    m.load_text_encoder(enc)
    B, n = len(prompts), 40
    g = _g(77)
    y0 = torch.randn(B, n, cfg.num_channels, generator=g)
    text = 0.5 * torch.randn(B, n, cfg.dim_text, generator=g)
    ctx, _ = enc.encode_ids(torch.from_numpy(fx["b0_ids"]), torch.from_numpy(fx["b0_mask"]))
    ctx = ctx.cpu()
    cm = torch.from_numpy(fx["b0_mask"]).bool()
    assert float((ctx - torch.from_numpy(fx["b0_out"])).abs().max()) <= 1e-4
    kw = dict(y0=y0, text_embed=text, steps=4, cfg_strength=2.0, remove_parallel_component=False, return_raw_output=True)
    cond = torch.zeros(B, n, cfg.num_channels)
    got = m.sample(cond, prompt=prompts, **kw)
    ref = m.sample(cond, context=torch.from_numpy(fx["b0_out"]), context_mask=cm, **kw)
    assert float((got - ref).abs().max()) <= 1e-4
    # a dropped clip is encoded as "the sound of X X" (x3:2053-2057): its mask changes, its context is zeroed
    vdp = [False, True, False]
    got = m.sample(cond, prompt=prompts, video_drop_prompt=vdp, **kw)
    cm2 = cm.clone()
    cm2[1] = torch.arange(cm.shape[1]) < 6
    ref = m.sample(cond, context=torch.from_numpy(fx["b0_out"]), context_mask=cm2, video_drop_prompt=vdp, **kw)
    assert float((got - ref).abs().max()) <= 1e-4
    # one forward
    x = torch.randn(B, n, cfg.num_channels, generator=g)
    t = torch.tensor([0.1, 0.5, 0.9])
    got = m.transformer_with_pred_head(x, times=t, text=text, prompt=prompts)
    ref = m.transformer_with_pred_head(x, times=t, text=text, context=torch.from_numpy(fx["b0_out"]), context_mask=cm)
    assert float((got - ref).abs().max()) <= 1e-4
