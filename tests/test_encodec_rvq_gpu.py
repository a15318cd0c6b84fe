"""GPU: the Encodec quantizer kernels (csrc/encodec_rvq.hip) through `EncodecQuantizer`.

The result of `encode` is an index, so it is not compared value by value but by what makes an index right: in float64, from the
residual the kernel's own earlier picks leave, the codeword it chose scores within the rounding error of fp32 arithmetic of the
best one -- every frame, every stage.  Against the float64 vectors of the library's own quantizer (tests/golden/encodec_rvq.npz)
frames may then differ only where the two picks are that close, and only on 1 % of the frames.

The tolerance, derived (U = 2^-24, the unit round-off of fp32; K = 128 terms; E = the largest codeword norm of the stage).  The
kernel ranks by 2 r.e - |e|^2; half of that, h_j = r.e_j - |e_j|^2 / 2, ranks the same and is what is bounded here.
  * a K-term fp32 dot product, in any summation order, is within K U / (1 - K U) * sum |r_i e_i| <= (K + 1) U |r| |e| of the exact one;
  * |e|^2 / 2 is held as one fp32 number: U E^2 / 2;  the final fused multiply-add rounds once: U (|r| E + E^2 / 2);
    together <= (K + 8) U (|r| E + E^2), with room to spare;
  * the kernel's residual is fp32: every stage's subtraction rounds each element once, an error vector of norm <= U |r_j|, so after
    stage s the residual is within U sum_{j <= s} |r_j| of the float64 one, which moves h by at most E times that.
tol(s) = (K + 8) U (|r_s| E + E^2) + U E sum_{j <= s} |r_j|.  Two scores are compared, so the gap allowed is 2 tol(s)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "encodec_rvq.npz")
SHAPES = ((2, 750), (3, 17), (1, 1))               # the full clip (47 frame tiles per clip, the last partial), a partial tile, one frame
CASES = [f"{fam}_{b}x{t}" for fam in ("structured", "gaussian") for b, t in SHAPES]
K, U = 128, 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD, allow_pickle=False))
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def params(gold):
    from v2a_amd.synth import random_encodec_quantizer_state_dict
    return random_encodec_quantizer_state_dict(gold["meta"]["param_seed"])


@pytest.fixture(scope="module")
def quant(params):
    from v2a_amd.encodec import EncodecQuantizer
    return EncodecQuantizer(params, DEV)


@pytest.fixture(scope="module")
def cb64(quant, gold):
    cb = quant.codebooks.cpu()
    assert hashlib.md5(cb.numpy().tobytes()).hexdigest() == gold["meta"]["codebooks_md5"]
    return cb.double()


def float64_walk(cb64, x, codes):
    """x (b, 128, t) fp32, codes (S, b, t): walks the stages in float64 along `codes`.  Returns per stage and frame the gap between
    the best h and the chosen one's, and tol(s) of the module docstring."""
    S = codes.shape[0]
    r = x.double().permute(0, 2, 1).reshape(-1, K)
    c = codes.reshape(S, -1)
    carry = torch.zeros(r.shape[0], dtype=torch.float64)
    gaps, tols = [], []
    for s in range(S):
        e = cb64[s]
        E = e.norm(dim=1).max()
        rn = r.norm(dim=1)
        carry = carry + rn
        h = r @ e.t() - 0.5 * e.pow(2).sum(1)
        gaps.append(h.max(1).values - h.gather(1, c[s][:, None])[:, 0])
        tols.append((K + 8) * U * (rn * E + E * E) + U * E * carry)
        r = r - e[c[s]]
    return torch.stack(gaps), torch.stack(tols)


@pytest.fixture(scope="module")
def runs(gold, quant, cb64):
    """Every fixture case encoded once at 24 kbps, with its float64 walk: shared by the tests below, never modified."""
    from v2a_amd.synth import synthetic_encodec_latents
    out = {}
    for name in CASES:
        fam, shape = name.split("_")
        b, t = (int(v) for v in shape.split("x"))
        c = gold["meta"]["cases"][name]
        x = synthetic_encodec_latents(cb64.float(), b, t, c["seed"], structured=fam == "structured")
        assert hashlib.md5(x.numpy().tobytes()).hexdigest() == c["md5"], name
        codes = quant.encode(x.to(DEV), 24.0)
        assert codes.shape == (32, b, t) and codes.dtype == torch.int64 and codes.device.type == "cuda"
        codes = codes.cpu()
        assert int(codes.min()) >= 0 and int(codes.max()) < 1024
        gaps, tols = float64_walk(cb64, x, codes)
        out[name] = dict(x=x, codes=codes, gaps=gaps, tols=tols, want=torch.from_numpy(gold[name + "_codes"].astype(np.int64)))
    return out


@pytest.mark.parametrize("name", CASES)
def test_every_pick_is_optimal_to_fp32_rounding(runs, name):
    """Every frame and every stage, no exclusions: the chosen codeword's float64 score is within 2 tol(s) of the best."""
    r = runs[name]
    ratio = r["gaps"] / (2 * r["tols"])
    print(f"{name}: max gap / (2 tol) = {float(ratio.max()):.3e}; picks that are not the float64 best: {int((r['gaps'] > 0).sum())} of {ratio.numel()}")
    assert bool((r["gaps"] <= 2 * r["tols"]).all())


@pytest.mark.parametrize("name", CASES)
def test_codes_agree_with_the_float64_library(runs, cb64, name):
    """Frames whose codes differ from the library's float64 run: at the first differing stage (same residual on both sides) the two
    picks score within 2 tol(s) of each other, and such frames are at most 1 % of the case's."""
    r = runs[name]
    got, want = r["codes"].reshape(32, -1), r["want"].reshape(32, -1)
    differ = (got != want).any(0).nonzero()[:, 0]
    x64 = r["x"].double().permute(0, 2, 1).reshape(-1, K)
    print(f"{name}: {len(differ)} of {got.shape[1]} frames differ from the float64 library codes")
    for f in differ.tolist():
        s = int((got[:, f] != want[:, f]).nonzero()[0, 0])
        res = x64[f] - sum(cb64[u][int(got[u, f])] for u in range(s))             # what both sides enter stage s with
        pair = cb64[s][[int(got[s, f]), int(want[s, f])]]
        h = pair @ res - 0.5 * pair.pow(2).sum(1)
        assert abs(float(h[0] - h[1])) <= 2 * float(r["tols"][s, f]), (name, f, s, h.tolist(), float(r["tols"][s, f]))
    assert len(differ) <= 0.01 * got.shape[1]


def test_ties_go_to_the_lowest_index(params):
    """Duplicated rows, and frames equal to them: the two scores are the same bits, the lower index wins -- whether the twins sit in
    different waves' shares of the codebook, in one 16-codeword tile, or in two tiles of one wave."""
    from v2a_amd.encodec import EncodecQuantizer
    sd = {k: v.clone() for k, v in params.items() if k.endswith(".embed") and int(k.split(".")[1]) < 2}
    e0 = sd["layers.0.codebook.embed"]
    twins = ((37, 900), (130, 140), (200, 216), (0, 1023))
    for lo, hi in twins:
        e0[hi] = e0[lo]
    q = EncodecQuantizer(sd, DEV)
    x = torch.stack([e0[lo] for lo, _ in twins] + [e0[500]]).t()[None].contiguous()          # (1, 128, 5)
    codes = q.encode(x.to(DEV)).cpu()
    assert codes.shape == (2, 1, 5)
    assert codes[0, 0].tolist() == [lo for lo, _ in twins] + [500]
    # the same frames as rows 17 .. 21 of a longer clip: a second tile, other lanes
    long = torch.cat([torch.randn(1, 128, 17, generator=torch.Generator().manual_seed(1)), x], 2)
    assert q.encode(long.to(DEV)).cpu()[0, 0, 17:].tolist() == [lo for lo, _ in twins] + [500]


def test_codes_do_not_depend_on_batch_layout_or_stage_count(runs, quant):
    r = runs["gaussian_3x17"]
    x = r["x"].to(DEV)
    for i in range(3):                                             # alone == inside the batch of 3
        assert torch.equal(quant.encode(x[i:i + 1]).cpu(), r["codes"][:, i:i + 1])
    xl = x.permute(0, 2, 1)                                        # (3, 17, 128): a view, read in place through its strides
    assert torch.equal(quant.encode(xl, channels_last=True).cpu(), r["codes"])
    assert torch.equal(quant.encode(xl.contiguous(), channels_last=True).cpu(), r["codes"])
    assert torch.equal(quant.encode(x, 6.0).cpu(), r["codes"][:8])  # 8 stages == the first 8 rows of 32
    big = runs["structured_2x750"]
    xb = big["x"].to(DEV)
    assert torch.equal(quant.encode(xb[1:2]).cpu(), big["codes"][:, 1:2])
    assert torch.equal(quant.encode(xb[:, :, 5:38], 6.0).cpu(), big["codes"][:8, :, 5:38])      # a slice: other tiles, same codes
    assert torch.equal(quant.encode(xb.permute(0, 2, 1).contiguous(), 1.5, channels_last=True).cpu(), big["codes"][:2])


@pytest.mark.parametrize("name", CASES)
def test_decode_is_the_sequential_fp32_sum(gold, quant, runs, name):
    """Bit-equal to the stage-ordered fp32 sum of torch on the CPU, in both layouts, and within 1e-6 of the float64 library values
    relative to the largest of them (a sum of signed terms has no element-wise relative bound)."""
    from v2a_amd.encodec import rvq_decode_torch
    want = runs[name]["want"]
    ref = rvq_decode_torch(quant.codebooks.cpu(), want)
    got = quant.decode(want.to(DEV))
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(quant.decode(want, channels_last=True).cpu(), ref.permute(0, 2, 1))
    assert torch.equal(quant.decode(want[:8].to(torch.int32).to(DEV)).cpu(), rvq_decode_torch(quant.codebooks.cpu(), want[:8]))
    val = gold[name + "_dec_val"]
    err = np.abs(got.cpu().numpy()[tuple(gold[name + "_dec_idx"].T)] - val).max() / np.abs(val).max()
    print(f"{name}: decode, max |delta| / max |value| against float64 = {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_round_trip_leaves_the_library_residual(gold, quant, runs, cb64, name):
    """|x - decode(encode(x))| per frame equals the float64 library's residual norm on frames whose codes agree.  fp32 accuracy:
    the decoded frame is a 32-term fp32 sum, within 32 U sum_s |e^s[c_s]| (vector norms) of the float64 sum, and the norm of a
    difference moves by no more than the difference does."""
    r = runs[name]
    x = r["x"]
    xh = quant.decode(quant.encode(x.to(DEV))).cpu()
    got = (x.double() - xh.double()).norm(dim=1)
    agree = (r["codes"] == r["want"]).all(0)
    assert bool(agree.any())
    terms = sum(cb64[s][r["codes"][s]].norm(dim=-1) for s in range(32))      # (b, t)
    tol = 32 * U * terms
    err = (got - torch.from_numpy(gold[name + "_resid_norm"])).abs()
    print(f"{name}: round trip on {int(agree.sum())} agreeing frames, max | |x - x^| - library | / tol = {float((err / tol)[agree].max()):.3e}")
    assert bool((err <= tol)[agree].all())


def _small_dit(cond_proj_in):
    from oracle import e2_cfm_oracle as O
    cfg = O.DiTConfig(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, num_channels=128,
                      max_seq_len=256, cond_proj_in=cond_proj_in)
    return O, cfg, O.init_params(cfg, 77)


def test_sample_takes_a_prompt_of_codes(params, quant, runs):
    """sample(cond=codes (b, n_q, n)) == sample(cond=the decoded latents), bit for bit, with lens < duration."""
    from conftest import make_model
    O, cfg, P = _small_dit(True)
    y0, text, roll, ctx, cm = O.synthetic_inputs(cfg, 2, 40, nc=5, seed=5, piano=True)
    codes = runs["structured_2x750"]["codes"][:8, :, :8].transpose(0, 1).contiguous()          # (2, 8 codebooks, 8 frames)
    kw = dict(y0=y0, text_embed=text, context=ctx, context_mask=cm, frames_embed=roll, lens=torch.tensor([8, 8]),
              duration=torch.tensor([40, 33]), steps=4, cfg_strength=2.0, remove_parallel_component=False, return_raw_output=True)
    latent = quant.decode(codes.transpose(0, 1), channels_last=True)
    assert latent.shape == (2, 8, 128)
    m = make_model(cfg, P, "fp32")
    with pytest.raises(NotImplementedError, match="load_audio_quantizer"):
        m.sample(codes, **kw)
    assert m.load_audio_quantizer(quant) is quant
    ref = m.sample(latent, **kw).cpu()
    got = m.sample(codes, **kw).cpu()
    assert got.shape == (2, 40, 128) and torch.equal(got, ref)
    assert torch.equal(got[:, :8], latent.cpu())                   # the prompt frames come back unchanged
    m2 = make_model(cfg, P, "fp32")
    assert type(m2.load_audio_quantizer({"quantizer." + k: v for k, v in params.items()})) is type(quant)
    assert torch.equal(m2.sample(codes.to(torch.int32), **kw).cpu(), ref)
    back = m2.latents_to_codes(latent, 6.0)
    assert back.shape == (2, 8, 8) and back.dtype == torch.int64
    assert torch.equal(back, quant.encode(latent, 6.0, channels_last=True).transpose(0, 1))


def test_cli_writes_codes(tmp_path, params):
    """--codes 6: <name>.codes.npy is int16 (8, n) and equals latents_to_codes of the written latents' valid frames."""
    import v2a_amd
    from conftest import make_model
    from v2a_amd import cli
    from v2a_amd.synth import random_encodec_decoder_state_dict
    O, cfg, P = _small_dit(False)
    ck = tmp_path / "small.pt"
    torch.save({"model_state_dict": P}, ck)
    esd = {"decoder." + k: v for k, v in random_encodec_decoder_state_dict(1).items()}
    esd.update({"quantizer." + k: v for k, v in params.items()})
    torch.save(esd, tmp_path / "encodec.pt")
    vids = [str(tmp_path / f"clip{i}.mp4") for i in range(2)]
    (tmp_path / "list.scp").write_text("".join(f"{v}\tsound {i}\n" for i, v in enumerate(vids)))
    g = torch.Generator().manual_seed(5)
    for i, v in enumerate(vids):
        v2a_amd.save_clip_cache(v2a_amd.feature_cache_path(v), torch.randn(13 + i, cfg.dim_text, generator=g), 0.4 + 0.1 * i)
        np.savez(v.replace(".mp4", ".t5.npz"), (0.2 * torch.randn(4 + i, cfg.dim, generator=g)).numpy())
    mc = dict(dim=cfg.dim, dim_text=cfg.dim_text, dim_frames=cfg.dim_frames, depth=cfg.depth, heads=cfg.heads, dim_head=cfg.dim_head,
              frames_heads=cfg.frames_heads, num_registers=cfg.num_registers, max_seq_len=cfg.max_seq_len, num_channels=cfg.num_channels)
    out = tmp_path / "out"
    written = cli.main([str(ck), "0", str(tmp_path / "list.scp"), "0", "2", str(out), "--batch", "2", "--steps", "3", "--frames", "40",
                        "--dtype", "fp32", "--model-config", json.dumps(mc), "--encodec", str(tmp_path / "encodec.pt"), "--codes", "6"])
    assert len(written) == 2
    m = make_model(cfg, P, "fp32")
    m.load_audio_quantizer(esd)
    for i, p in enumerate(written):
        n = int((0.4 + 0.1 * i) * 24000) // 320                   # 30 and 37 valid frames of 40
        lat = torch.from_numpy(np.load(p))
        codes = np.load(p.replace(".latent.npy", ".codes.npy"))
        assert codes.dtype == np.int16 and codes.shape == (8, n)
        assert np.array_equal(codes, m.latents_to_codes(lat[None, :n], 6.0)[0].cpu().numpy())
        assert os.path.exists(p.replace(".latent.npy", ".wav"))
