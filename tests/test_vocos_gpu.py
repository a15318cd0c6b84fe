"""GPU: the Vocos vocoder (v2a_amd.Vocos: csrc/vocos.hip around the exact-fp32 v2a_gemm and v2a_clip_layernorm) against the float64
restatement of tests/vocos_ref.py, whose last stage is torch.istft; its bit-level promises; and `E2TTS.sample(return_raw_output=False)`
through `load_vocoder`.

Accuracy.  For every case and every tap (after embed + norm, after every block, after the final LayerNorm, the head logits, S, the wave)
    r = max |x - x64| / max |x64|     per clip, the largest over the clips.
The yardstick is r_cpu32, the same ratio for torch's CPU fp32 run of the same restatement; the assertion is r_gpu <= 4 r_cpu32, the
factor of tests/test_mel_spec_gpu.py: it covers another summation order and other transcendentals, and lies far below what an indexing,
border, window or envelope mistake gives (an r thousands of times larger).  Both ratios are printed per tap.

The weights (vocos_ref.py) make the clip at 100 bite and the phases span several turns; the test asserts both on the float64 reference.
Cases: T = 2 is the shortest wave, T = 3 shorter than the 7 taps, hop 32 of 64 two frames per sample, hop 24 no divisor of n_fft,
(20, 96, 160) dims that are no powers of two with M past one 64-row GEMM tile, and the real network at M past 128 rows, its inverse DFT
in K chunks.

Measured on an MI355X (profiles/vocos.txt): r_gpu / r_cpu32 lies in 0.55 - 1.66 over every case and tap, the largest at the embed tap of
the real network.  With every GEMM in one launch (K up to 1536 in one fp32 chain) the real network read 2.80 at embed and 4.48 at block0;
Vocos cuts every K into chunks of 256 for that reason.
"""
import math

import pytest
import torch

import vocos_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0

_VOC = {}


def vocoder(i):
    """The device module of case i, built once."""
    from v2a_amd import Vocos
    if i not in _VOC:
        d = R.case_data(i)
        _VOC[i] = Vocos(d["sd"], DEV, hop_length=d["hop"])
    return _VOC[i]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_float64_parity_of_every_tap(i):
    d = R.case_data(i)
    n_fft = d["n_fft"]
    nb = n_fft // 2 + 1
    lg = d["t64"]["logits"]
    clipped = float((lg[..., :nb] > math.log(100.0)).double().mean())
    assert 0.001 <= clipped <= 0.5, clipped                                     # the clip is hit, and not everywhere
    assert float(lg[..., nb:].abs().max()) > 4 * math.pi                        # phases of several turns
    taps = {}
    wave = vocoder(i).decode(d["x"], taps=taps)
    torch.cuda.synchronize()
    assert wave.shape == d["t64"]["wave"].shape and wave.dtype == torch.float32 and wave.is_cuda
    assert set(taps) == set(d["t64"])
    bad = []
    for name, want in d["t64"].items():
        got = taps[name].cpu()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), name
        r_gpu, r_cpu = R.ratio(got, want), R.ratio(d["t32"][name], want)
        print(f"vocos case {i} {R.CASES[i]} tap {name:8s} r_gpu = {r_gpu:.3e}  r_cpu32 = {r_cpu:.3e}  ratio = {r_gpu / r_cpu:.2f}")
        if not r_gpu <= FACTOR * r_cpu:
            bad.append((name, r_gpu, r_cpu))
    assert not bad, bad
    assert torch.equal(wave.cpu(), taps["wave"].cpu())


def test_clip_bounds_every_magnitude():
    """The head bias raised so that every magnitude clips: |S| <= 100 (1 + 2^-23) everywhere."""
    from v2a_amd import Vocos
    d = R.case_data(2, extra_bias=40.0)
    nb = d["n_fft"] // 2 + 1
    assert float(d["t64"]["logits"][..., :nb].min()) > math.log(100.0)
    taps = {}
    Vocos(d["sd"], DEV, hop_length=d["hop"]).decode(d["x"], taps=taps)
    S = taps["S"].cpu().double()
    mag = (S[..., 0] ** 2 + S[..., 1] ** 2).sqrt()
    assert float(mag.max()) <= 100.0 * (1 + 2.0 ** -23) and float(mag.min()) >= 100.0 * (1 - 2.0 ** -23)
    assert R.ratio(taps["wave"].cpu(), d["t64"]["wave"]) <= FACTOR * R.ratio(d["t32"]["wave"], d["t64"]["wave"])


@pytest.mark.parametrize("i", [2, 5, 6])
def test_bits_do_not_depend_on_batch_run_object_or_input_device(i):
    from v2a_amd import Vocos
    d = R.case_data(i)
    voc = vocoder(i)
    a = voc.decode(d["x"]).clone()
    assert torch.equal(a, voc.decode(d["x"]))                                   # two runs
    assert torch.equal(a, Vocos(d["sd"], DEV, hop_length=d["hop"]).decode(d["x"]))          # two objects
    assert torch.equal(a, voc.decode(d["x"].to(DEV)))                           # host and device inputs
    for k in range(d["x"].shape[0]):
        assert torch.equal(a[k], voc.decode(d["x"][k:k + 1])[0]), k             # row k of the batch = the single-clip call
    assert torch.equal(a[0], voc.decode(d["x"][0])[0])                          # (C, T)


def test_lens_decode_every_clip_as_if_alone():
    d = R.case_data(2)                                                          # T = 37, b = 3
    voc = vocoder(2)
    lens = (37, 20, 2)
    got = voc.decode(d["x"], lens=lens)
    assert isinstance(got, list) and [g.shape[0] for g in got] == [(n - 1) * d["hop"] for n in lens]
    for k, n in enumerate(lens):
        alone = voc.decode(d["x"][k:k + 1, :, :n])[0]
        assert torch.equal(got[k], alone), k
    # the real network: clips that end inside a dwconv tile and one frame behind a GEMM tile
    d = R.case_data(7)                                                          # T = 130, b = 2
    voc = vocoder(7)
    lens = torch.tensor([129, 17])
    got = voc.decode(d["x"], lens=lens)
    for k, n in enumerate(lens.tolist()):
        assert torch.equal(got[k], voc.decode(d["x"][k:k + 1, :, :n])[0]), k
    with pytest.raises(ValueError, match="lens"):
        voc.decode(d["x"], lens=(130, 1))
    with pytest.raises(ValueError, match="lens"):
        voc.decode(d["x"], lens=(131, 2))
    with pytest.raises(ValueError, match="lens"):
        voc.decode(d["x"], lens=(5,))


def test_out_view_with_its_own_row_stride_and_canary():
    d = R.case_data(4)                                                          # hop 24, T = 11, b = 3
    voc = vocoder(4)
    plain = voc.decode(d["x"]).clone()
    b, n = plain.shape
    CANARY = -777.0
    big = torch.full((b + 2, n + 13), CANARY, device=DEV)
    view = big[1:1 + b, 5:5 + n]
    ret = voc.decode(d["x"], out=view)
    torch.cuda.synchronize()
    assert ret.data_ptr() == view.data_ptr() and torch.equal(view, plain)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:1 + b, 5:5 + n] = False
    assert bool((big[mask] == CANARY).all())
    # with lens, nothing behind a clip's (lens - 1) hop samples is written
    big.fill_(CANARY)
    got = voc.decode(d["x"], lens=(11, 4, 2), out=view)
    for k, m in enumerate((11, 4, 2)):
        assert got[k].shape[0] == (m - 1) * d["hop"] and torch.equal(got[k], voc.decode(d["x"][k:k + 1, :, :m])[0])
        assert bool((view[k, (m - 1) * d["hop"]:] == CANARY).all())
    assert bool((big[mask] == CANARY).all())
    for bad in (torch.empty(b, n + 1, device=DEV), torch.empty(b, n, device=DEV, dtype=torch.float64), torch.empty(b, n),
                torch.empty(b, 2 * n, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            voc.decode(d["x"], out=bad)


def test_decode_refuses_wrong_shapes():
    d = R.case_data(2)
    voc = vocoder(2)
    with pytest.raises(ValueError, match="at least 2 frames"):
        voc.decode(d["x"][:, :, :1])
    with pytest.raises(ValueError, match="features are"):
        voc.decode(d["x"][:, :5])
    with pytest.raises(ValueError, match="features are"):
        voc.decode(d["x"][None])
    with pytest.raises(ValueError, match="floating point"):
        voc.decode(torch.zeros(1, 10, 5, dtype=torch.int32))


def test_sample_decodes_through_the_loaded_vocoder(small):
    """E2TTS.sample(return_raw_output=False) after load_vocoder: element i = voc.decode(raw[i, :duration[i]].T[None])[0] bit for bit,
    (duration[i] - 1) hop samples; `vocoder=` still takes precedence; without load_vocoder the raw latents come back as before."""
    from conftest import make_model
    from v2a_amd import Vocos
    cfg, P, inp = small["cfg"], small["P"], small["inp"]
    assert cfg.num_channels == 16
    ref = R.VocosRef(16, 64, 192, 2, 64, 16, seed=7)
    voc = Vocos(ref.state_dict(), DEV, hop_length=16)
    m = make_model(cfg, P, "fp32")
    b, n = inp["y0"].shape[0], inp["y0"].shape[1]
    assert b == 2
    duration = torch.tensor([n, n - 11])
    kw = dict(y0=inp["y0"], text_embed=inp["text"], context=inp["ctx"], context_mask=inp["ctx_mask"], frames_embed=inp["roll"], steps=3,
              cfg_strength=2.0, remove_parallel_component=False, lens=duration, duration=duration)
    cond = torch.zeros(b, n, 16)
    raw = m.sample(cond, return_raw_output=True, **kw)
    assert torch.equal(m.sample(cond, return_raw_output=False, **kw), raw)          # no vocoder loaded: the latents, as before
    assert m.load_vocoder(voc) is voc and m.vocos is voc
    audio = m.sample(cond, return_raw_output=False, **kw)
    assert isinstance(audio, list) and len(audio) == b
    for k in range(b):
        dk = int(duration[k])
        want = voc.decode(raw[k, :dk].transpose(0, 1)[None])[0]
        assert audio[k].shape == ((dk - 1) * 16,) and torch.equal(audio[k], want), k
    seen = {}
    got = m.sample(cond, return_raw_output=False, vocoder=lambda mel: seen.setdefault("shape", tuple(mel.shape)), **kw)
    assert got == (b, 16, n) and seen["shape"] == (b, 16, n)
    m2 = make_model(cfg, P, "fp32")
    assert m2.load_vocoder(ref.state_dict()).C == 16                               # a state dict


@pytest.mark.parametrize("d", [16, 528, 2048])
def test_dwconv_ln_kernel_at_the_widths_no_network_case_has(d):
    """v2a_vocos_dwconv_ln outside the networks above: one lane group, the first width past 512 (the kernel's other instantiation, a
    partly filled lane group) and the widest, whose tile holds 2 frames.  Against F.conv1d + F.layer_norm in float64, with torch's CPU
    fp32 evaluation of the same two calls as the yardstick and the factor of the parity test; rows behind lens[b] come out zero, rows
    behind T stay untouched, and a clip's rows do not depend on the other clip."""
    import torch.nn.functional as F
    from v2a_amd import _lib as L
    g = torch.Generator().manual_seed(d)
    B, T, lens = 2, 9, (9, 4)
    P = T + 6
    x = torch.randn(B, P, d, generator=g)
    w, bias = torch.randn(d, 1, 7, generator=g) / 7 ** 0.5, 0.1 * torch.randn(d, generator=g)
    gam, bet = 1 + 0.3 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)

    def ref(dt):
        out = []
        for k, n in enumerate(lens):
            c = F.conv1d(x[k, :n].to(dt).t()[None], w.to(dt), bias.to(dt), padding=3, groups=d)[0].t()
            out.append(F.layer_norm(c, (d,), gam.to(dt), bet.to(dt), 1e-6))
        return out

    r64, r32 = ref(torch.float64), ref(torch.float32)
    SENT = -555.0
    y = torch.full((B, P, d), SENT, device=DEV)
    xd, wt = x.to(DEV), w[:, 0].t().contiguous().to(DEV)
    args = [bias.to(DEV), gam.to(DEV), bet.to(DEV)]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    L.check(L.lib().v2a_vocos_dwconv_ln(xd.data_ptr(), d, wt.data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), 1e-6, B, T, P, d,
                                        lens_dev.data_ptr(), y.data_ptr(), d, L.stream_ptr()))
    torch.cuda.synchronize()
    y = y.cpu()
    for k, n in enumerate(lens):
        r_gpu = float((y[k, :n].double() - r64[k]).abs().max() / r64[k].abs().max())
        r_cpu = float((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max())
        print(f"dwconv_ln d = {d} clip {k}: r_gpu = {r_gpu:.3e}  r_cpu32 = {r_cpu:.3e}")
        assert r_gpu <= FACTOR * r_cpu, (k, r_gpu, r_cpu)
        assert bool((y[k, n:T] == 0).all()) and bool((y[k, T:] == SENT).all())
    alone = torch.full((1, P, d), SENT, device=DEV)
    L.check(L.lib().v2a_vocos_dwconv_ln(xd[1].data_ptr(), d, wt.data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), 1e-6, 1, lens[1], P,
                                        d, None, alone.data_ptr(), d, L.stream_ptr()))
    assert torch.equal(alone[0, :lens[1]].cpu(), y[1, :lens[1]])
