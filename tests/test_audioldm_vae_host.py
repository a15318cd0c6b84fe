"""CPU: host side of the AudioLDM VAE decoder (v2a_amd.AudioLDMVaeDecoder / VaeVocoder, csrc/audioldm_vae.hip) -- the float64
restatement against the reference module's fixture, the state-dict layout against the module's recorded keys, the flat-grid launch plan
of a 3x3 convolution against torch's in float64, prefix stripping, scale_factor precedence, the refusals of the class, the v-bias fold,
the header and binding of the new entry points and their argument checks, E2TTS.load_vocoder and the CLI flag."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import audioldm_vae_ref as R
from v2a_amd import audioldm_vae as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("v2a_vae_stage_in", "v2a_vae_gn_stats", "v2a_vae_gn_act_pad", "v2a_vae_upsample_pad", "v2a_vae_softmax", "v2a_vae_conv_out")
CASES = [(c, r) for c in R.CONFIGS for r in R.REGIMES]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(R.GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("cfg,regime", CASES)
def test_restatement_equals_the_reference_module_in_float64(gold, cfg, regime):
    config, sd = R.CONFIGS[cfg], R.state_dict(cfg, regime)
    names = R.tap_names(config)
    for tag, emb, sf in R.items(cfg):
        taps = R.decoder(sd, R.to_z(emb), config, sf, torch.float64)
        key = f"{cfg}_{regime}_{tag}"
        want = gold[key + "_mel"]
        assert taps["mel"].shape == (1, 1) + want.shape
        assert np.abs(taps["mel"][0, 0].numpy() - want).max() <= 1e-12 * np.abs(want).max(), key
        for t, name in enumerate(names[:-1]):
            a = taps[name].numpy()
            assert a.shape == tuple(gold[key + "_tap_shape"][t]), (key, name)
            top = np.abs(a).max()
            assert np.abs(a[tuple(gold[key + "_tap_idx"][t].astype(np.int64).T)] - gold[key + "_tap_val"][t]).max() <= 1e-12 * top, (key, name)
            assert np.abs(np.array([a.mean(), np.abs(a).mean(), a.max(), a.min()]) - gold[key + "_tap_stats"][t]).max() <= 1e-12 * top, (key, name)
        assert gold[f"{cfg}_{regime}_scale"].shape == (len(names),) and bool((gold[f"{cfg}_{regime}_scale"] > 0).all())


def test_expected_shapes_equal_the_module_key_list(gold):
    for cfg, config in R.CONFIGS.items():
        want = {k: tuple(int(d) for d in s.split("x")) for k, s in zip(gold[f"{cfg}_keys"], gold[f"{cfg}_shapes"])}
        got = V.expected_state_dict_shapes(config)
        assert list(got) == list(want) and got == want, cfg
        assert {k: tuple(v.shape) for k, v in R.state_dict(cfg, "plain").items()} == want
        assert V.config_from_state_dict(R.state_dict(cfg, "plain")) == {**config, "ch_mult": tuple(config["ch_mult"])}
    full = V.expected_state_dict_shapes()
    dec = {k: s for k, s in full.items() if k.startswith("decoder.")}
    assert len(dec) == 112 and len(full) == 114
    n = sum(int(np.prod(s)) for s in full.values())
    assert 32.9e6 < n < 33.1e6, n                                                  # 33.0 M parameters
    assert V.tap_names() == ["conv_in", "mid1", "attn", "mid2", "up2b0", "up2b1", "up2b2", "up2us", "up1b0", "up1b1", "up1b2", "up1us", "up0b0",
                             "up0b1", "up0b2", "mel"]


@pytest.mark.parametrize("C,k_chunk", [(32, 512), (32, 64), (64, 64), (128, 512), (512, 512), (96, 80)])
def test_flat_grid_launch_plan_equals_conv2d(C, k_chunk):
    """The segments of `conv2d_launches` over the flat padded grid of a two-clip bordered map, added launch by launch in float64, against
    F.conv2d of each clip: pixel (y, x) of clip b comes out at row b * pitch + y * Wp + x, and the last window ends inside the map."""
    g = torch.Generator().manual_seed(C + k_chunk)
    b, H, W, co = 2, 3, 4, 5
    Wp, pitch = W + 2, (H + 2) * (W + 2)
    x = torch.randn(b, C, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(co, C, 3, 3, dtype=torch.float64, generator=g)
    bias = torch.randn(co, dtype=torch.float64, generator=g)
    want = F.conv2d(x, w, bias, padding=1)
    op = torch.zeros(b, H + 2, Wp, C, dtype=torch.float64)
    op[:, 1:H + 1, 1:W + 1] = x.permute(0, 2, 3, 1)
    flat = op.reshape(-1)
    wm = w.permute(0, 2, 3, 1).reshape(co, 9 * C)
    M = (b - 1) * pitch + (H - 1) * Wp + W
    launches = V.conv2d_launches(C, Wp, k_chunk)
    assert all(1 <= len(segs) <= 3 and all(ka % 16 == 0 for _, ka in segs) and sum(ka for _, ka in segs) <= k_chunk for segs in launches)
    got, k0 = bias.expand(M, co).clone(), 0
    for segs in launches:
        a = torch.cat([torch.stack([flat[m * C + off:m * C + off + ka] for m in range(M)]) for off, ka in segs], 1)      # raises past the map's end
        got = got + a @ wm[:, k0:k0 + a.shape[1]].t()
        k0 += a.shape[1]
    assert k0 == 9 * C and (M - 1) * C + max(off + ka for segs in launches for off, ka in segs) == flat.numel()
    for i in range(b):
        rows = torch.stack([got[i * pitch + y * Wp + xx] for y in range(H) for xx in range(W)]).reshape(H, W, co).permute(2, 0, 1)
        assert (rows - want[i]).abs().max() <= 1e-13 * want.abs().max(), (C, k_chunk, i)
    assert V.plain_launches(640, 512) == [[(0, 512)], [(512, 128)]]                 # P V at 640 tokens: two launches


def test_prefix_stripping_and_scale_factor_precedence():
    sd = R.state_dict("small", "plain")
    ck = {"first_stage_model." + k: v for k, v in sd.items()}
    ck.update({"first_stage_model.encoder.conv_in.weight": torch.zeros(3), "first_stage_model.quant_conv.weight": torch.zeros(2),
               "first_stage_model.vocoder.conv_pre.bias": torch.zeros(1), "first_stage_model.loss.logvar": torch.zeros(1)})
    d = V.AudioLDMVaeDecoder(ck, device="cpu")
    assert d.scale_factor == 1.0 and d.config == {**R.REDUCED, "ch_mult": (1, 2)}
    assert torch.equal(d._w64["decoder.conv_out.weight"], sd["decoder.conv_out.weight"].double())
    assert (d.C, d.up, d.bins, d.zc, d.c_pad, d.levels) == (128, 2, 32, 8, 16, 2)
    assert V.AudioLDMVaeDecoder({**ck, "scale_factor": torch.tensor(0.25)}, device="cpu").scale_factor == 0.25
    assert V.AudioLDMVaeDecoder({**ck, "scale_factor": torch.tensor(0.25)}, device="cpu", scale_factor=0.5).scale_factor == 0.5
    full = V.AudioLDMVaeDecoder(R.state_dict("full", "plain"), device="cpu")
    assert (full.C, full.up, full.bins, full.widths) == (128, 4, 64, [128, 256, 512])
    assert full._stages(250) == [(250, 16, 252 * 18), (500, 32, 502 * 34), (1000, 64, 1002 * 66)]


def test_constructor_refusals():
    sd = R.state_dict("small", "plain")
    V.AudioLDMVaeDecoder(sd, device="cpu")
    with pytest.raises(TypeError):
        V.AudioLDMVaeDecoder([1], device="cpu")
    for key in ("decoder.conv_in.weight", "decoder.mid.attn_1.q.bias", "decoder.up.1.upsample.conv.weight", "decoder.up.0.block.0.nin_shortcut.weight",
                "decoder.norm_out.bias", "post_quant_conv.weight"):
        with pytest.raises(KeyError, match=re.escape(key)):
            V.AudioLDMVaeDecoder({k: v for k, v in sd.items() if k != key}, device="cpu")
    with pytest.raises(ValueError, match=re.escape("decoder.mid.block_2.norm2.bias")):
        V.AudioLDMVaeDecoder({**sd, "decoder.mid.block_2.norm2.bias": torch.zeros(65)}, device="cpu")
    with pytest.raises(ValueError, match=re.escape("decoder.up.1.attn.0.q.weight")):          # attention outside the middle
        V.AudioLDMVaeDecoder({**sd, "decoder.up.1.attn.0.q.weight": torch.zeros(64, 64, 1, 1)}, device="cpu")
    with pytest.raises(ValueError, match=re.escape("decoder.up.1.upsample.conv.weight")):     # UpsampleTimeStride4
        V.AudioLDMVaeDecoder({**sd, "decoder.up.1.upsample.conv.weight": torch.zeros(64, 64, 5, 5)}, device="cpu")
    with pytest.raises(ValueError, match=re.escape("decoder.up.0.block.0.conv_shortcut.weight")):
        V.AudioLDMVaeDecoder({**sd, "decoder.up.0.block.0.conv_shortcut.weight": torch.zeros(32, 64, 3, 3)}, device="cpu")
    odd = dict(ch=48, ch_mult=(1, 2), num_res_blocks=1, z_channels=8)                          # 48 channels: no 32 groups
    from v2a_amd.synth import random_audioldm_vae_state_dict
    with pytest.raises(ValueError, match="multiple of 32"):
        V.AudioLDMVaeDecoder(random_audioldm_vae_state_dict(odd, 1), device="cpu")
    with pytest.raises(ValueError, match="k_chunk"):
        V.AudioLDMVaeDecoder(sd, device="cpu", k_chunk=40)
    with pytest.raises(ValueError, match="scale_factor"):
        V.AudioLDMVaeDecoder(sd, device="cpu", scale_factor=0.0)
    d = V.AudioLDMVaeDecoder(sd, device="cpu")
    for bad, match in ((torch.zeros(1, 64, 4), "latents are"), (torch.zeros(1, 128, 0), "latents are"), (torch.zeros(1, 128, 4, dtype=torch.int32), "latents are")):
        with pytest.raises(ValueError, match=match):
            d.decode_latents(bad)
    with pytest.raises(ValueError, match="z is"):
        d.decode_first_stage(torch.zeros(1, 8, 4, 8))


def test_v_bias_fold_equals_the_unfolded_attention_in_float64():
    sd = {k: v.double() for k, v in R.state_dict("small", "offset").items()}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 64, 3, 16, dtype=torch.float64, generator=g) * 3 + 2
    pre = "decoder.mid.attn_1"
    want = R.attn_block(sd, pre, x)
    folded = dict(sd)
    folded[pre + ".proj_out.bias"] = V.fold_v_bias(sd[pre + ".proj_out.weight"], sd[pre + ".proj_out.bias"], sd[pre + ".v.bias"])
    folded[pre + ".v.bias"] = torch.zeros(64, dtype=torch.float64)
    got = R.attn_block(folded, pre, x)
    assert (got - want).abs().max() <= 1e-13 * want.abs().max()
    assert float(sd[pre + ".v.bias"].abs().max()) > 1.0                           # the fold moves something


def test_header_declares_the_entries_with_the_lines_they_replace():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ENTRIES:
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS, name
    block = h[h.index("AudioLDM VAE decoder"):]
    assert "x3:470-490" in block and "modules.py:650-683" in block and block.count("Replaces:") >= 6
    assert _lib.ABI_VERSION == 9
    assert "#define V2A_VAE_GN_TILE %d" % V.GN_TILE in h and "#define V2A_VAE_GROUPS %d" % V.GROUPS in h
    assert "audioldm_vae" in open(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build.sh")).read()


def test_library_exports_the_entries_and_refuses_bad_arguments_without_a_gpu(lib):
    assert lib.v2a_abi_version() == 9
    A = 4096                                                                       # an aligned, non-null address: nothing is read before the checks pass
    call = lambda fn, ok, order: (lambda **k: fn(*[{**ok, **k}[n] for n in order], None))
    ok = dict(src=A, sb=128 * 4, sc=16 * 4, st=1, sw=4, B=1, H=4, W=16, zc=8, lens=None, w=2 * A, bias=3 * A, out=4 * A, cpad=16, opc=6 * 18)
    f = call(lib.v2a_vae_stage_in, ok, ("src", "sb", "sc", "st", "sw", "B", "H", "W", "zc", "lens", "w", "bias", "out", "cpad", "opc"))
    for k, word in ((dict(src=None), b"null"), (dict(out=A), b"aliased"), (dict(H=0), b"H=0"), (dict(B=70000), b"B=70000"), (dict(zc=0), b"zc=0"),
                    (dict(zc=17), b"zc=17"), (dict(cpad=24), b"c_pad=24"), (dict(cpad=80), b"c_pad=80"), (dict(st=0), b"strides"),
                    (dict(opc=6 * 18 - 1), b"out_rows_per_clip"), (dict(out=4 * A + 4), b"alignment"), (dict(lens=2), b"alignment")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(x=A, spc=6 * 18, swp=18, B=1, H=4, W=16, C=64, lens=None, part=2 * A, tiles=1)
    f = call(lib.v2a_vae_gn_stats, ok, ("x", "spc", "swp", "B", "H", "W", "C", "lens", "part", "tiles"))
    for k, word in ((dict(part=None), b"null"), (dict(C=48), b"C=48"), (dict(C=0), b"C=0"), (dict(C=8192), b"C=8192"), (dict(swp=15), b"src_wp=15"),
                    (dict(spc=3 * 18 + 15), b"src_rows_per_clip"), (dict(tiles=0), b"tiles=0"), (dict(H=40, spc=42 * 18), b"tiles=1"), (dict(W=0), b"W=0"),
                    (dict(part=2 * A + 4), b"alignment")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(x=A, spc=6 * 18, swp=18, B=1, H=4, W=16, C=64, lens=None, part=2 * A, tiles=1, g=3 * A, b=4 * A, eps=1e-6, swish=1, out=5 * A, opc=6 * 18,
              border=1)
    f = call(lib.v2a_vae_gn_act_pad, ok, ("x", "spc", "swp", "B", "H", "W", "C", "lens", "part", "tiles", "g", "b", "eps", "swish", "out", "opc", "border"))
    for k, word in ((dict(g=None), b"null"), (dict(out=A), b"aliased"), (dict(C=48), b"C=48"), (dict(border=2), b"border=2"), (dict(swish=3), b"swish=3"),
                    (dict(eps=0.0), b"eps"), (dict(opc=6 * 18 - 1), b"out_rows_per_clip"), (dict(border=0, opc=63), b"out_rows_per_clip"),
                    (dict(tiles=0), b"tiles=0"), (dict(swp=15), b"src_wp=15"), (dict(H=0), b"H=0"), (dict(out=5 * A + 8), b"alignment")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(x=A, spc=6 * 18, swp=18, B=1, H=4, W=16, C=64, lens=None, out=2 * A, opc=10 * 34)
    f = call(lib.v2a_vae_upsample_pad, ok, ("x", "spc", "swp", "B", "H", "W", "C", "lens", "out", "opc"))
    for k, word in ((dict(x=None), b"null"), (dict(out=A), b"aliased"), (dict(C=6), b"C=6"), (dict(opc=10 * 34 - 1), b"out_rows_per_clip"),
                    (dict(spc=60), b"src_rows_per_clip"), (dict(W=4096), b"W=4096"), (dict(H=0), b"H=0"), (dict(lens=2), b"alignment")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(s=A, ld=32, rows=18, n=16, scale=0.5)
    f = call(lib.v2a_vae_softmax, ok, ("s", "ld", "rows", "n", "scale"))
    for k, word in ((dict(s=None), b"null"), (dict(s=A + 2), b"misaligned"), (dict(ld=15), b"ld=15"), (dict(n=0), b"n=0"), (dict(rows=0), b"rows=0"),
                    (dict(scale=0.0), b"scale"), (dict(scale=float("nan")), b"scale"), (dict(scale=float("inf")), b"scale")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k
    ok = dict(a=A, rpc=6 * 18, B=1, H=4, W=16, C=32, lens=None, w=2 * A, bias=3 * A, out=4 * A)
    f = call(lib.v2a_vae_conv_out, ok, ("a", "rpc", "B", "H", "W", "C", "lens", "w", "bias", "out"))
    for k, word in ((dict(w=None), b"null"), (dict(out=A), b"aliased"), (dict(C=30), b"C=30"), (dict(C=0), b"C=0"), (dict(rpc=6 * 18 - 1), b"rows_per_clip"),
                    (dict(H=0), b"H=0"), (dict(a=A + 4), b"alignment"), (dict(out=4 * A + 2), b"alignment")):
        assert f(**k) == -1 and word in lib.v2a_last_error(), k


def _stub_vocoder(C, hop):
    stub = V.VaeVocoder.__new__(V.VaeVocoder)                                      # no weights, no GPU: what load_vocoder reads
    stub.C, stub.hop = C, hop
    return stub


def test_load_vocoder_takes_a_vae_vocoder():
    import v2a_amd
    tk = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=64, if_text_modules=True,
              if_cross_attn=True, if_audio_conv=True, if_text_conv=True)
    stub = _stub_vocoder(128, 640)
    m = v2a_amd.E2TTS(transformer=tk, num_channels=128, sampling_rate=16000, device="cpu")
    assert m.load_vocoder(stub) is stub and m.vocos is stub
    with pytest.raises(TypeError, match="keywords"):
        m.load_vocoder(stub, hop_length=640)
    m64 = v2a_amd.E2TTS(transformer=tk, num_channels=64, sampling_rate=16000, device="cpu")
    with pytest.raises(ValueError, match="num_channels=64"):
        m64.load_vocoder(stub)
    assert m64.vocos is None
    with pytest.raises(ValueError, match="Vocos"):                                 # a state dict still means Vocos
        m.load_vocoder(R.state_dict("small", "plain"))


def test_vae_vocoder_joins_the_two_halves():
    import hifigan_ref as HR
    from v2a_amd import HiFiGAN, VaeVocoder
    dec = V.AudioLDMVaeDecoder(R.state_dict("full", "plain"), device="cpu")
    hifi = HiFiGAN(HR.state_dict("full"), device="cpu")
    voc = VaeVocoder(dec, hifi)
    assert (voc.C, voc.hop) == (128, 640) and [voc.output_length(l) for l in (1, 3, 250)] == [672, 1952, 160032]
    ck = {"first_stage_model." + k: v for k, v in R.state_dict("full", "plain").items()}
    ck.update({"first_stage_model.vocoder." + k: v for k, v in HR.state_dict("full").items()})
    ck["scale_factor"] = torch.tensor(0.5)
    both = VaeVocoder.from_state_dict(ck, device="cpu")
    assert both.decoder.scale_factor == 0.5 and both.hop == 640 and both.hifigan.c0 == 1024
    with pytest.raises(TypeError, match="VaeVocoder"):
        VaeVocoder(hifi, dec)
    small = V.AudioLDMVaeDecoder(R.state_dict("small", "plain"), device="cpu")     # 32 mel bins against a 64-bin HiFiGAN
    with pytest.raises(ValueError, match="32 mel bins"):
        VaeVocoder(small, hifi)


class _NotATensor:
    pass


def test_cli_checkpoint_loader_names_what_is_wrong(tmp_path):
    from v2a_amd import cli
    sd = {"first_stage_model.decoder.conv_in.bias": torch.zeros(4), "scale_factor": torch.tensor(0.5)}
    torch.save(sd, tmp_path / "plain.pt")
    torch.save({"state_dict": sd, "epoch": 3}, tmp_path / "nested.pt")
    for name in ("plain.pt", "nested.pt"):
        got = cli.load_audioldm_state_dict(str(tmp_path / name))
        assert list(got) == list(sd) and torch.equal(got["scale_factor"], sd["scale_factor"])
    torch.save([torch.zeros(2)], tmp_path / "list.pt")
    with pytest.raises(ValueError, match="expected a state dict"):
        cli.load_audioldm_state_dict(str(tmp_path / "list.pt"))
    torch.save({"state_dict": sd, "callbacks": _NotATensor()}, tmp_path / "objects.pt")
    with pytest.raises(ValueError, match="objects other than tensors"):
        cli.load_audioldm_state_dict(str(tmp_path / "objects.pt"))


def test_cli_takes_audioldm_as_the_vocoder(capsys):
    from v2a_amd import cli
    args = ["ckpt", "0", "scp", "0", "1", "out"]
    a = cli.build_parser().parse_args(args + ["--audioldm", "vae.ckpt"])
    assert a.audioldm == "vae.ckpt" and a.vocos is None and a.encodec is None
    assert cli.build_parser().parse_args(args).audioldm is None
    for other in (["--vocos", "dir"], ["--encodec", "state.pt"]):
        with pytest.raises(SystemExit):
            cli.main(args + ["--audioldm", "vae.ckpt"] + other)
        assert "exclusive" in capsys.readouterr().err
