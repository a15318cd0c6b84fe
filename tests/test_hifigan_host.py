"""CPU: host side of the HiFi-GAN vocoder (v2a_amd.HiFiGAN, csrc/hifigan.hip) -- the float64 restatement against the reference module's
fixture, the polyphase and dilated-segment plans against torch's convolutions in float64, the length formula, weight-norm folding, prefix
stripping, every refusal of the class, the header and binding of the new entry points and their argument checks, E2TTS.load_vocoder."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as R
from v2a_amd import hifigan as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("v2a_hifigan_act_pad", "v2a_hifigan_post", "v2a_hifigan_conv")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("cfg", ["full", "small"])
def test_restatement_equals_the_reference_module_in_float64(gold, cfg):
    config, sd = R.CONFIGS[cfg], R.state_dict(cfg)
    for tag, mel in R.items(cfg):
        taps = R.generator(sd, mel, config, torch.float64)
        for name in ("wave", "pre"):
            want = gold[f"{cfg}_{tag}_{name}"]
            assert taps[name].shape == (1,) + want.shape
            assert np.abs(taps[name][0].numpy() - want).max() <= 1e-12 * np.abs(want).max(), (tag, name)
        assert np.array_equal(R.to_int16(taps["wave"][0]), gold[f"{cfg}_{tag}_pcm"])
        for name in R.tap_names(config)[:-2]:
            a, key = taps[name].numpy(), f"{cfg}_{tag}_{name}"
            assert a.shape == tuple(gold[key + "_shape"]), key
            top = np.abs(a).max()
            assert np.abs(a[tuple(gold[key + "_idx"].T)] - gold[key + "_val"]).max() <= 1e-12 * top, key
            assert np.abs(np.array([a.mean(), np.abs(a).mean(), a.max(), a.min()]) - gold[key + "_stats"]).max() <= 1e-12 * top, key


def test_expected_shapes_equal_the_module_key_list(gold):
    for cfg, config in R.CONFIGS.items():
        want = {k: tuple(int(d) for d in s.split("x")) for k, s in zip(gold[f"{cfg}_keys"], gold[f"{cfg}_shapes"])}
        got = H.expected_state_dict_shapes(config)
        assert list(got) == list(want) and got == want, cfg
        sd = R.state_dict(cfg)
        assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sum(math_prod(s) for s in H.expected_state_dict_shapes().values()) == 55_264_897


def math_prod(s):
    n = 1
    for d in s:
        n *= d
    return n


@pytest.mark.parametrize("k,u", [(16, 5), (16, 4), (8, 2), (4, 2), (4, 2), (8, 4)])
def test_polyphase_plan_equals_conv_transpose1d(k, u):
    g = torch.Generator().manual_seed(k * 10 + u)
    ci, co, halo = 6, 4, 4
    w = torch.randn(ci, co, k, dtype=torch.float64, generator=g)
    bias = torch.randn(co, dtype=torch.float64, generator=g)
    pl = H.convt_plan(k, u)
    assert pl.p == (k - u) // 2 and pl.reach <= halo
    wp = H.polyphase_weight(w, u)
    assert wp.shape == (u * co, pl.taps * ci)
    for n in (1, 2, 7):
        x = torch.randn(n, ci, dtype=torch.float64, generator=g)                  # time-major
        want = F.conv_transpose1d(x.t()[None], w, bias, stride=u, padding=pl.p)[0].t()
        assert want.shape[0] == pl.out_len(n) == (n - 1) * u - 2 * pl.p + k
        op = torch.zeros(n + 2 * halo, ci, dtype=torch.float64)
        op[halo:halo + n] = x
        flat = op.reshape(-1)
        blocks = n + pl.extra
        a = torch.stack([flat[(halo - pl.s_max + q) * ci:(halo - pl.s_max + q + pl.taps) * ci] for q in range(blocks)])     # overlapping rows
        got = (a @ wp.t() + bias.repeat(u)).reshape(blocks * u, co)[:pl.out_len(n)]
        assert (got - want).abs().max() <= 1e-13 * want.abs().max(), (k, u, n)
    assert H.convt_plan(16, 5).out_len(1) == 6                                    # 5 L + 1


@pytest.mark.parametrize("k", [3, 5, 7, 11])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_dilated_segment_plan_equals_conv1d(k, d):
    g = torch.Generator().manual_seed(k * 10 + d)
    C, co, n, chunk = 32, 16, 9, 48
    pad = (k - 1) * d // 2
    halo = pad + 2
    w = torch.randn(co, C, k, dtype=torch.float64, generator=g)
    bias = torch.randn(co, dtype=torch.float64, generator=g)
    x = torch.randn(n, C, dtype=torch.float64, generator=g)
    want = F.conv1d(x.t()[None], w, bias, dilation=d, padding=pad)[0].t()
    wm = w.permute(0, 2, 1).reshape(co, k * C)
    op = torch.zeros(n + 2 * halo, C, dtype=torch.float64)
    op[halo:halo + n] = x
    flat = op.reshape(-1)
    for k_chunk in (chunk, 16, 256):
        launches = H.conv_launches(k, d, C, k_chunk)
        assert all(1 <= len(segs) <= 3 and all(ka % 16 == 0 for _, ka in segs) for segs in launches)
        assert all(sum(ka for _, ka in segs) <= max(k_chunk, 16) for segs in launches)
        got, k0 = bias.expand(n, co).clone(), 0
        for segs in launches:
            a = torch.cat([torch.stack([flat[(halo - pad + t) * C + off:(halo - pad + t) * C + off + ka] for t in range(n)]) for off, ka in segs], 1)
            got = got + a @ wm[:, k0:k0 + a.shape[1]].t()
            k0 += a.shape[1]
        assert k0 == k * C
        assert (got - want).abs().max() <= 1e-13 * want.abs().max(), (k, d, k_chunk)


def test_output_lengths():
    assert [H.output_length(T) for T in (1, 4, 16)] == [192, 672, 2592]
    assert [H.output_length(T) for T in R.RAGGED_LENS] == [832, 2592, 1472] == [160 * T + 32 for T in R.RAGGED_LENS]
    assert H.stage_lengths(16, (5, 4, 2, 2, 2), (16, 16, 8, 4, 4)) == [16, 81, 324, 648, 1296, 2592]
    small = R.CONFIGS["small"]
    assert [H.output_length(T, small["upsample_rates"], small["upsample_kernel_sizes"]) for T in R.SMALL_T] == [24, 88]
    v = H.HiFiGAN(R.state_dict("small"), device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)
    assert v.output_length(11) == 88 and v.hop == 8 and v.C == 80
    lens, pitch, chans = v._geometry(2, 11)
    assert lens == [11, 44, 88] and chans == [128, 64, 32] and pitch[1] == 4 * pitch[0] and pitch[2] == 8 * pitch[0]
    assert all(p >= n + 2 * v.halo for n, p in zip(lens, pitch))


def test_weight_norm_folding_and_prefix_stripping():
    sd = R.state_dict("small")
    g = torch.Generator().manual_seed(3)
    normed = {}
    for key, v in sd.items():
        if key.endswith(".weight"):
            gain = torch.rand(v.shape[0], 1, 1, generator=g) + 0.5
            normed[key[:-7] + ".weight_g"], normed[key[:-7] + ".weight_v"] = gain, v
        else:
            normed[key] = v
    for key in ("conv_pre", "ups.1", "resblocks.3.convs2.2", "conv_post"):
        want = torch._weight_norm(normed[key + ".weight_v"].double(), normed[key + ".weight_g"].double(), 0)
        got = H.fold_weight_norm(normed[key + ".weight_g"], normed[key + ".weight_v"])
        assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-15 * want.abs().max()
    kw = dict(device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)
    v = H.HiFiGAN({"first_stage_model.vocoder." + k: t for k, t in normed.items()} | {"first_stage_model.decoder.x": torch.zeros(1)}, **kw)
    want = torch._weight_norm(normed["ups.0.weight_v"].double(), normed["ups.0.weight_g"].double(), 0)
    assert torch.equal(v._w64["ups.0.weight"], want) or (v._w64["ups.0.weight"] - want).abs().max() <= 1e-15
    plain = H.HiFiGAN({"vocoder." + k: t for k, t in sd.items()}, **kw)
    assert torch.equal(plain._w64["conv_post.weight"], sd["conv_post.weight"].double())
    assert (plain.c0, plain.up_kernels, plain.res_kernels, plain.c_last, plain.nk) == (128, (8, 4), (3, 5), 32, 2)
    full = H.expected_state_dict_shapes()
    assert full["ups.0.weight"] == (1024, 512, 16) and full["resblocks.14.convs1.2.weight"] == (32, 32, 11)


def test_constructor_refusals():
    sd = R.state_dict("small")
    kw = dict(device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)
    H.HiFiGAN(sd, **kw)
    with pytest.raises(TypeError):
        H.HiFiGAN([1], **kw)
    for key in ("conv_pre.weight", "ups.1.weight", "ups.0.bias", "resblocks.2.convs2.1.weight", "conv_post.bias"):
        with pytest.raises(ValueError, match=re.escape(key)):
            H.HiFiGAN({k: v for k, v in sd.items() if k != key}, **kw)
    with pytest.raises(ValueError, match=re.escape("resblocks.1.convs1.0.bias")):
        H.HiFiGAN({**sd, "resblocks.1.convs1.0.bias": torch.zeros(65)}, **kw)
    with pytest.raises(ValueError, match=re.escape("conv_post.weight")):
        H.HiFiGAN({**sd, "conv_post.weight": torch.zeros(1, 32, 5)}, **kw)
    with pytest.raises(ValueError, match="more stages"):
        H.HiFiGAN(sd, device="cpu", upsample_rates=(4,), resblock_dilations=((1, 2, 4),) * 2)
    with pytest.raises(ValueError, match="multiple of 16"):                       # num_mels = 72
        H.HiFiGAN({**sd, "conv_pre.weight": torch.zeros(128, 72, 7)}, **kw)
    bad = {k: (v[:24, :12] if k.startswith("resblocks.") and v.ndim == 3 else v) for k, v in sd.items()}
    bad.update({"conv_pre.weight": torch.zeros(48, 80, 7), "conv_pre.bias": torch.zeros(48), "ups.0.weight": torch.zeros(48, 24, 8)})
    with pytest.raises(ValueError, match="multiple of 16"):                       # 48 -> 24 channels
        H.HiFiGAN(bad, **kw)
    with pytest.raises(ValueError, match=re.escape("ups.1.weight")):              # kernel 4 under stride 8
        H.HiFiGAN(sd, device="cpu", upsample_rates=(4, 8), resblock_dilations=((1, 2, 4),) * 2)
    with pytest.raises(ValueError, match="no polyphase plan"):
        H.convt_plan(4, 8)
    with pytest.raises(ValueError, match="one to three"):
        H.HiFiGAN(sd, device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 4)
    with pytest.raises(ValueError, match="fused"):
        H.HiFiGAN(sd, fused="yes", **kw)
    v = H.HiFiGAN(sd, **kw)
    for bad_mel, match in ((torch.zeros(1, 64, 4), "mel frames are"), (torch.zeros(80), "mel frames are"), (torch.zeros(1, 80, 0), "at least one"),
                           (torch.zeros(1, 80, 4, dtype=torch.int32), "floating point")):
        with pytest.raises(ValueError, match=match):
            v.decode(bad_mel)
    for lens in ((0,), (5,), (2, 2)):
        with pytest.raises(ValueError, match="lens"):
            v.decode(torch.zeros(1, 80, 4), lens=lens)
    with pytest.raises(ValueError, match="dec is"):
        v.decode_to_waveform(torch.zeros(1, 80, 4))


def test_fused_default_keeps_the_lds_heavy_shapes_on_the_composition():
    on = {(C, k, d): H.fused_default(C, k, d) for C in (32, 64, 128, 256) for k in (3, 7, 11) for d in (1, 3, 5)}
    off = {key for key, v in on.items() if not v}
    assert off == {(128, 7, 5), (128, 11, 3), (128, 11, 5)} | {(256, k, d) for k in (3, 7, 11) for d in (1, 3, 5)}
    kw = dict(device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)
    assert H.HiFiGAN(R.state_dict("small"), fused=False, **kw)._fused_at(32, 3, 1) is False
    assert H.HiFiGAN(R.state_dict("small"), fused="all", **kw)._fused_at(128, 11, 5) is True
    assert H.HiFiGAN(R.state_dict("small"), **kw)._fused_at(128, 11, 5) is False


def test_fragment_packing_is_a_permutation_of_the_weight():
    w = torch.arange(3 * 32 * 32, dtype=torch.float32).reshape(32, 32, 3)
    wp = H.pack_conv_fragments(w).reshape(3, 2, 2, 64, 4)                         # (j, kq, n, lane, e)
    for j, kq, n, lane, e in ((0, 0, 0, 0, 0), (2, 1, 0, 37, 3), (1, 0, 1, 63, 2), (1, 1, 1, 16, 1)):
        assert wp[j, kq, n, lane, e] == w[16 * n + (lane & 15), 16 * kq + 4 * e + (lane >> 4), j]
    assert torch.equal(wp.reshape(-1).sort().values, w.reshape(-1))


def test_header_declares_the_entries_with_the_lines_they_replace():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ENTRIES:
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS, name
    assert "x3:470-490" in h and "utilities.py:76-86" in h and "models.py:163-180" in h
    assert h[h.index("HiFi-GAN vocoder"):].count("Replaces:") >= 3
    assert _lib.ABI_VERSION == 9
    assert "#define V2A_HIFIGAN_TILE %d" % H.TILE in h
    assert "hifigan" in open(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build.sh")).read()


def test_library_exports_the_entries_and_refuses_bad_arguments_without_a_gpu(lib):
    assert lib.v2a_abi_version() == 9
    A = 4096                                                                       # an aligned, non-null address: nothing is read before the checks pass
    ok = dict(s0=A, s1=None, s2=None, spc=8, lds=32, B=1, T=8, C=32, lens=None, div=1.0, slope=0.1, out=2 * A, opc=14, halo=3)
    act = lambda **k: lib.v2a_hifigan_act_pad(*[{**ok, **k}[n] for n in ("s0", "s1", "s2", "spc", "lds", "B", "T", "C", "lens", "div", "slope", "out", "opc",
                                                                          "halo")], None)
    for k, word in ((dict(s0=None), b"null"), (dict(out=A), b"aliased"), (dict(s2=3 * A), b"in order"), (dict(C=30), b"C=30"), (dict(T=0), b"T=0"),
                    (dict(B=70000), b"B=70000"), (dict(opc=13), b"out_rows_per_clip"), (dict(spc=7), b"src_rows_per_clip"), (dict(lds=30), b"ld_src"),
                    (dict(div=0.0), b"divisor"), (dict(out=2 * A + 4), b"alignment"), (dict(lens=2), b"alignment")):
        assert act(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(a=A, rpc=20, B=1, T=8, C=32, lens=None, w=2 * A, bias=3 * A, wave=4 * A, pcm=None, pre=None, obs=8)
    post = lambda **k: lib.v2a_hifigan_post(*[{**ok, **k}[n] for n in ("a", "rpc", "B", "T", "C", "lens", "w", "bias", "wave", "pcm", "pre", "obs")], None)
    for k, word in ((dict(w=None), b"null"), (dict(wave=None), b"required"), (dict(C=513), b"C=513"), (dict(C=0), b"C=0"), (dict(rpc=7), b"rows_per_clip"),
                    (dict(obs=7), b"out_batch_stride"), (dict(T=0), b"T=0"), (dict(pcm=5 * A + 1), b"alignment"), (dict(wave=4 * A + 2), b"alignment")):
        assert post(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(x=A, ldx=32, rpc=20, B=1, T=8, C=32, lens=None, wp=2 * A, bias=3 * A, k=3, d=1, slope=0.1, resid=None, ldr=0, out=4 * A, ldo=32)
    conv = lambda **k: lib.v2a_hifigan_conv(*[{**ok, **k}[n] for n in ("x", "ldx", "rpc", "B", "T", "C", "lens", "wp", "bias", "k", "d", "slope", "resid",
                                                                       "ldr", "out", "ldo")], None)
    for k, word in ((dict(wp=None), b"null"), (dict(out=A), b"aliased"), (dict(C=48), b"C=48"), (dict(C=256), b"C=256"), (dict(k=4), b"k=4"),
                    (dict(d=0), b"d=0"), (dict(C=128, ldx=128, ldo=128, k=11, d=20), b"LDS"), (dict(rpc=7), b"rows_per_clip"), (dict(ldx=30), b"ldx"),
                    (dict(resid=5 * A, ldr=16), b"ldr"), (dict(T=0), b"T=0"), (dict(bias=3 * A + 4), b"alignment")):
        assert conv(**k) == -1 and word in lib.v2a_last_error(), k


class _Stub:
    """What load_vocoder reads of a vocoder, without a device."""


def test_load_vocoder_takes_a_hifigan():
    import v2a_amd
    from v2a_amd import HiFiGAN, MelSpec
    tk = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=64, if_text_modules=True,
              if_cross_attn=True, if_audio_conv=True, if_text_conv=True)
    stub = HiFiGAN.__new__(HiFiGAN)                                                # a 64-channel model, no weights, no GPU
    stub.C, stub.hop = 64, 160
    m = v2a_amd.E2TTS(transformer=tk, num_channels=64, sampling_rate=16000, device="cpu")
    assert m.load_vocoder(stub) is stub and m.vocos is stub
    with pytest.raises(TypeError, match="keywords"):
        m.load_vocoder(stub, hop_length=160)
    m80 = v2a_amd.E2TTS(transformer=tk, num_channels=80, sampling_rate=16000, device="cpu")
    with pytest.raises(ValueError, match="num_channels=80"):
        m80.load_vocoder(stub)
    assert m80.vocos is None
    small = HiFiGAN(R.state_dict("small"), device="cpu", upsample_rates=(4, 2), resblock_dilations=((1, 2, 4),) * 2)
    assert m80.load_vocoder(small) is small and small.hop == 8
    m.load_mel_spec(MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=64, device="cpu"))
    with pytest.raises(ValueError, match="hop"):                                   # hop 160 against a mel_spec of hop 16
        m.load_vocoder(stub)
    with pytest.raises(TypeError, match="load_vocoder"):                           # a state dict still means Vocos, anything else is refused
        m.load_vocoder(3)
    with pytest.raises(ValueError, match="Vocos"):
        m.load_vocoder(R.state_dict("small"))
