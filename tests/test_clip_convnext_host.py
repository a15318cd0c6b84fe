"""CPU: the host side of the ConvNeXt and mixed image encoders (convnext.py): shape inference, key prefixes, the layer-scale fold,
refusals, from_pretrained, the E2TTS and CLI wiring and the cache names.  Nothing here launches a kernel."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=128)


def _sd(config=SMALL, seed=1, outlier=0.0):
    from v2a_amd.synth import random_convnext_state_dict
    return random_convnext_state_dict(config, seed, outlier)


def _enc(sd=None, **kw):
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    kw.setdefault("compute", "fp32")
    kw.setdefault("resize", 64)
    kw.setdefault("crop", 64)
    return CLIPConvNeXtImageEncoder(_sd() if sd is None else sd, "cpu", **kw)


def test_shapes_prefixes_and_eps():
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder, infer_config, strip_prefixes
    from v2a_amd.resample import normalize_table
    sd = _sd()
    bare = strip_prefixes(sd)
    assert "trunk.stem.0.weight" in bare and "head.proj.weight" in bare and all(k.startswith(("trunk.", "head.")) for k in bare)
    assert infer_config(bare) == dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=128, layer_norm_eps=1e-5)
    e = _enc(sd)
    assert (e.depths, e.dims, e.out_dim, e.eps) == ((1, 1, 2, 1), (64, 128, 256, 512), 128, 1e-5)
    assert (e.S, e.resize, e.P, e.g, e.sizes, e.kp, e.crop_offset) == (64, 64, 4, 16, (16, 8, 4, 2), 64, "torchvision")
    assert np.array_equal(e.lut.numpy(), normalize_table(formula="torchvision"))
    assert _enc(sd, config=dict(layer_norm_eps=1e-6, depths=(9,))).eps == 1e-6             # only eps is taken from a config
    # the reference checkpoint's prefix (also under model_state_dict, beside other modules' keys) and the bare keys
    ck = {"model_state_dict": dict({"image_encoder." + k: v for k, v in sd.items()}, **{"transformer.x": torch.zeros(1)})}
    for other in (ck, bare, {"image_encoder." + k: v for k, v in bare.items()}):
        o = _enc(other)
        assert o.dims == e.dims and torch.equal(o.patch_w, e.patch_w) and torch.equal(o.proj, e.proj)
    # prepared layouts: the stem's patch GEMM weight (K zero-padded 48 -> 64), tap-major depthwise weights, (ky, kx, c) downsample rows
    assert e.patch_w.shape == (64, 64) and float(e.patch_w[:, 48:].abs().max()) == 0.0
    assert torch.equal(e.patch_w[:, :48], bare["trunk.stem.0.weight"].reshape(64, 48))
    b = e.stages[2]["blocks"][1]
    w = bare["trunk.stages.2.blocks.1.conv_dw.weight"]
    assert b["dw_w"].shape == (49, 256) and b["dw_w"].is_contiguous() and float(b["dw_w"][3 * 7 + 5, 17]) == float(w[17, 0, 3, 5])
    ds = bare["trunk.stages.1.downsample.1.weight"]
    assert e.stages[1]["ds_w"].shape == (128, 256) and float(e.stages[1]["ds_w"][5, (1 * 2 + 0) * 64 + 9]) == float(ds[5, 9, 1, 0])
    assert "ds_w" not in e.stages[0] and e.proj_b is None
    # bf16x3: hi | lo planes of the same values
    s = _enc(sd, compute="bf16x3")
    hi, lo = s.proj[:, :512].float(), s.proj[:, 512:].float()
    assert s.proj.dtype == torch.bfloat16 and float((hi + lo - e.proj).abs().max()) <= 2.0 ** -16 * float(e.proj.abs().max())
    with_bias = dict(sd, **{"visual.head.proj.bias": torch.ones(128)})
    assert torch.equal(_enc(with_bias).proj_b, torch.ones(128))
    assert isinstance(e, CLIPConvNeXtImageEncoder)


def test_layer_scale_is_folded_in_float64():
    sd = _sd(seed=5)
    e = _enc(sd)
    for (s, j) in ((0, 0), (2, 1), (3, 0)):
        p = f"visual.trunk.stages.{s}.blocks.{j}."
        g, w, b = sd[p + "gamma"].double(), sd[p + "mlp.fc2.weight"].double(), sd[p + "mlp.fc2.bias"].double()
        assert 0.1 <= float(g.min()) and float(g.max()) <= 1.0 and float(g.max() - g.min()) > 0.5
        blk = e.stages[s]["blocks"][j]
        assert torch.equal(blk["fc2"], (g[:, None] * w).float()) and torch.equal(blk["fc2_b"], (g * b).float())
        # what the fold stands for: gamma * (W x + b) on a float64 vector
        x = torch.randn(w.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(s))
        assert float((blk["fc2"].double() @ x + blk["fc2_b"].double() - g * (w @ x + b)).abs().max()) <= 1e-6


def test_outlier_regime_of_the_seeded_weights():
    plain, hot = _sd(seed=3), _sd(seed=3, outlier=30.0)
    k = "visual.trunk.stages.2.blocks.0.mlp.fc2.weight"
    # four rows of every stage's fc2 (and their biases) stand 30x above the rest; the plain regime has none (the draw of the hot
    # channels moves the generator, so the two regimes' other weights differ as well)
    norms = lambda sd: sd[k].norm(dim=1) / sd[k].norm(dim=1).median()
    assert int((norms(hot) > 20).sum()) == 4 and int((norms(hot) < 1.5).sum()) == 256 - 4 and int((norms(plain) > 1.5).sum()) == 0
    assert torch.equal(hot["visual.trunk.stem.0.weight"], plain["visual.trunk.stem.0.weight"])
    assert torch.equal(_sd(seed=3)[k], plain[k]) and not torch.equal(_sd(seed=4)[k], plain[k])


def test_refusals():
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    sd = _sd()
    with pytest.raises(KeyError, match="stem.0.weight"):
        _enc({"vision_model.embeddings.class_embedding": torch.zeros(4)})
    short = {k: v for k, v in sd.items() if not k.endswith("blocks.1.norm.bias")}
    with pytest.raises(KeyError, match="norm.bias"):
        _enc(short)
    with pytest.raises(KeyError, match="gamma"):
        _enc({k: v for k, v in sd.items() if not k.endswith("stages.1.blocks.0.gamma")})
    with pytest.raises(ValueError, match="shape"):
        _enc(dict(sd, **{"visual.trunk.stages.1.downsample.1.bias": torch.zeros(64)}))
    # variants outside the reference's model, by their keys
    with pytest.raises(NotImplementedError, match="conv_mlp"):
        _enc({k: (v[:, :, None, None] if k.endswith("mlp.fc1.weight") or k.endswith("mlp.fc2.weight") else v) for k, v in sd.items()})
    mlp_head = {k: v for k, v in sd.items() if k != "visual.head.proj.weight"}
    mlp_head.update({"visual.head.mlp.fc1.weight": torch.zeros(8, 512), "visual.head.mlp.fc2.weight": torch.zeros(128, 8)})
    with pytest.raises(NotImplementedError, match="projection"):
        _enc(mlp_head)
    with pytest.raises(NotImplementedError, match="pooling"):
        _enc(dict(sd, **{"visual.trunk.head.attn_pool.q.weight": torch.zeros(4, 4)}))
    # geometry: the crop must survive the stem's 4 and three halvings; the resize may not lie below it
    for kw in (dict(crop=72), dict(crop=48), dict(resize=32)):
        with pytest.raises(ValueError, match="crop"):
            _enc(sd, **kw)
    assert _enc(sd, resize=80, crop=64).sizes == (16, 8, 4, 2) and _enc(sd, resize=96, crop=96).sizes == (24, 12, 6, 3)
    with pytest.raises(ValueError, match="compute"):
        _enc(sd, compute="bf16")
    with pytest.raises(ValueError, match="multiples of 64"):
        from v2a_amd.synth import random_convnext_state_dict
        CLIPConvNeXtImageEncoder(random_convnext_state_dict(dict(depths=(1, 1), dims=(32, 96), embed_dim=64), 1), "cpu", compute="fp32", resize=64, crop=64)
    with pytest.raises(ValueError, match="frames"):
        _enc(sd)(np.zeros((2, 8, 8, 3), np.float32))


def test_from_pretrained_reads_open_clip_config(tmp_path):
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    from v2a_amd.resample import normalize_table
    sd = _sd()
    d = tmp_path / "CLIP-convnext_xxlarge"
    d.mkdir()
    torch.save(sd, str(d / "open_clip_pytorch_model.bin"))
    vc = dict(timm_model_name="convnext_xxlarge", timm_model_pretrained=False, timm_pool="", timm_proj="linear", image_size=64)
    (d / "open_clip_config.json").write_text(json.dumps(dict(model_cfg=dict(embed_dim=128, vision_cfg=vc, text_cfg=dict(width=8)),
                                                             preprocess_cfg=dict(mean=[0.5, 0.4, 0.3], std=[0.2, 0.3, 0.4]))))
    e = CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert (e.eps, e.S, e.resize, e.out_dim) == (1e-5, 64, 64, 128)
    assert np.array_equal(e.lut.numpy(), normalize_table((0.5, 0.4, 0.3), (0.2, 0.3, 0.4), formula="torchvision"))
    # timm's other sizes norm with 1e-6; a caller's keyword wins over the file
    (d / "open_clip_config.json").write_text(json.dumps(dict(model_cfg=dict(vision_cfg=dict(vc, timm_model_name="convnext_large_d")))))
    e = CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu", compute="fp32", resize=96)
    assert (e.eps, e.S, e.resize) == (1e-6, 64, 96) and np.array_equal(e.lut.numpy(), normalize_table(formula="torchvision"))
    assert CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu", compute="fp32", config=dict(layer_norm_eps=1e-5)).eps == 1e-5
    # safetensors wins over the .bin when both are there
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in _sd(seed=2).items()}, str(d / "open_clip_model.safetensors"))
    e2 = CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert not torch.equal(e2.proj, e.proj) and torch.equal(e2.proj, _enc(_sd(seed=2)).proj)
    for bad, what in ((dict(vc, timm_model_name="vit_base_patch16_224"), "ConvNeXt"), (dict(vc, timm_pool="abs_attn"), "pooling"),
                      (dict(vc, timm_proj="mlp"), "projection")):
        (d / "open_clip_config.json").write_text(json.dumps(dict(model_cfg=dict(vision_cfg=bad))))
        with pytest.raises(NotImplementedError, match=what):
            CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu")
    (d / "open_clip_config.json").write_text(json.dumps(dict(model_cfg=dict(vision_cfg=vc), preprocess_cfg=dict(interpolation="bilinear"))))
    with pytest.raises(NotImplementedError, match="BICUBIC"):
        CLIPConvNeXtImageEncoder.from_pretrained(str(d), "cpu")


class _Stub:
    """An encoder's interface as MixedImageEncoder uses it: rows of a constant, `short` frames fewer than it was given."""

    def __init__(self, dim, value, short=0):
        self.out_dim, self.value, self.short, self.calls = dim, value, short, 0

    def __call__(self, frames):
        self.calls += 1
        return torch.full((len(frames) - self.short, self.out_dim), float(self.value))


def _stubs(**kw):
    return dict(dinov2=_Stub(5, 4, **kw), clip_vit=_Stub(2, 1), clip_convnext=_Stub(4, 3), clip_vit2=_Stub(3, 2))


def test_mixed_encoder_order_width_and_shortest_cut():
    import v2a_amd
    from v2a_amd.convnext import MIXED_ORDER, MixedImageEncoder
    assert MIXED_ORDER == ("clip_vit", "clip_vit2", "clip_convnext", "dinov2") and v2a_amd.MixedImageEncoder is MixedImageEncoder
    m = MixedImageEncoder(_stubs())
    assert m.out_dim == 14 and list(m.encoders) == list(MIXED_ORDER)
    rows = m(np.zeros((6, 8, 8, 3), np.uint8))
    assert rows.shape == (6, 14) and rows.dtype == torch.float32
    assert rows[0].tolist() == [1.0] * 2 + [2.0] * 3 + [3.0] * 4 + [4.0] * 5
    assert MixedImageEncoder(_stubs(short=2))(np.zeros((6, 8, 8, 3), np.uint8)).shape == (4, 14)            # x3:1786-1788
    for bad in (dict(clip_vit=_Stub(2, 1)), dict(_stubs(), extra=_Stub(1, 0))):
        with pytest.raises(ValueError, match="exactly"):
            MixedImageEncoder(bad)


def _small_e2tts(dim_text=128, **kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=dim_text, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_e2tts_wiring_under_clip_convnext(tmp_path):
    import v2a_amd
    from v2a_amd.convnext import CLIPConvNeXtImageEncoder
    from v2a_amd.e2tts import IMAGE_ENCODERS
    from v2a_amd.synth import random_clip_vision_state_dict, random_dinov2_state_dict
    assert IMAGE_ENCODERS["clip_convnext"] is CLIPConvNeXtImageEncoder and "CLIPConvNeXtImageEncoder" in v2a_amd.__all__
    assert v2a_amd.CLIPConvNeXtImageEncoder is CLIPConvNeXtImageEncoder and list(IMAGE_ENCODERS) == ["clip_vit", "clip_vit2", "clip_convnext", "dinov2", "mixed"]
    sd = _sd()
    m = _small_e2tts(video_encoder="clip_convnext")
    enc = m.load_image_encoder(sd, compute="fp32", resize=64, crop=64)
    assert isinstance(enc, CLIPConvNeXtImageEncoder) and m._clip is enc and m.load_image_encoder(enc) is enc
    assert m.load_image_encoder({"image_encoder." + k: v for k, v in sd.items()}, compute="fp32", resize=64, crop=64).out_dim == 128
    d = tmp_path / "convnext"
    d.mkdir()
    torch.save(sd, str(d / "open_clip_pytorch_model.bin"))
    (d / "open_clip_config.json").write_text(json.dumps(dict(model_cfg=dict(vision_cfg=dict(timm_model_name="convnext_xxlarge", image_size=64)))))
    assert type(m.load_image_encoder(str(d), compute="fp32")) is CLIPConvNeXtImageEncoder
    with pytest.raises(TypeError):
        m.load_image_encoder(3)
    with pytest.raises(ValueError, match="dim_text"):
        _small_e2tts(dim_text=64, video_encoder="clip_convnext").load_image_encoder(sd, compute="fp32", resize=64, crop=64)
    # the weights of the other choices are refused by name, with or without config=
    vit = random_clip_vision_state_dict(dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=56,
                                             patch_size=14, projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3), 1)
    dino_cfg = dict(hidden_size=192, num_hidden_layers=1, num_attention_heads=3, mlp_ratio=4, image_size=70, patch_size=14, layer_norm_eps=1e-6,
                    use_swiglu_ffn=True, num_channels=3, layerscale_value=1.0)
    for other in ("clip_convnext", "mixed"):
        for wrong, kw in ((vit, {}), (random_dinov2_state_dict(dino_cfg, 1), dict(config=dino_cfg))):
            with pytest.raises(NotImplementedError, match="clip_vit2") as ei:
                _small_e2tts(video_encoder=other).load_image_encoder(wrong, **kw)
            assert "dinov2" in str(ei.value) and "trunk.stem.0.weight" in str(ei.value)
    bare = _small_e2tts(video_encoder="clip_convnext")
    with pytest.raises(RuntimeError, match="load_image_encoder"):
        bare.sample(torch.zeros(1, 8, 16), video_frames=[(np.zeros((2, 8, 8, 3), np.uint8), 1.0)])


def test_e2tts_wiring_under_mixed_and_part_caches(tmp_path):
    from v2a_amd.convnext import MixedImageEncoder
    from v2a_amd.e2tts import IMAGE_ENCODERS
    from v2a_amd.features import encode_mixed_cached, feature_cache_path, load_clip_cache, save_clip_cache
    assert IMAGE_ENCODERS["mixed"] is MixedImageEncoder
    m = _small_e2tts(dim_text=14, video_encoder="mixed")
    mixed = MixedImageEncoder(_stubs())
    assert m.load_image_encoder(mixed) is mixed
    built = m.load_image_encoder(_stubs())                                   # a dict with one entry per choice
    assert isinstance(built, MixedImageEncoder) and built.out_dim == 14 and m._clip is built
    with pytest.raises(ValueError, match="dim_text"):
        _small_e2tts(dim_text=15, video_encoder="mixed").load_image_encoder(mixed)
    with pytest.raises(NotImplementedError, match="one entry per choice"):
        m.load_image_encoder(_sd())                                          # ConvNeXt weights alone are one part of four
    # the parts' own caches: an existing one is read (and its encoder not run), the others are written under their choices' names
    vp = str(tmp_path / "v.mp4")
    fr = np.zeros((5, 8, 8, 3), np.uint8)
    save_clip_cache(feature_cache_path(vp, "clip_vit2"), torch.full((4, 3), 9.0), 2.0)         # one frame short: the cut
    rows = encode_mixed_cached(vp, fr, 2.0, mixed)
    assert rows.shape == (4, 14) and rows[0].tolist() == [1.0] * 2 + [9.0] * 3 + [3.0] * 4 + [4.0] * 5
    assert mixed.encoders["clip_vit2"].calls == 0 and all(mixed.encoders[k].calls == 1 for k in ("clip_vit", "clip_convnext", "dinov2"))
    names = {"clip_vit": "v.generated.npz", "clip_vit2": "v.generated.clip_vit2.npz", "clip_convnext": "v.generated.clip_convnext.npz",
             "dinov2": "v.generated.dinov2.npz"}
    for k, n in names.items():
        emb, dur = load_clip_cache(str(tmp_path / n))
        assert dur == 2.0 and emb.shape == ((4, 3) if k == "clip_vit2" else (5, mixed.encoders[k].out_dim))
    assert not os.path.exists(str(tmp_path / "v.generated.mixed.npz"))       # the caller's to write
    # E2TTS: video_paths without a cache go through the same function and the mixed cache is written
    m.load_image_encoder(mixed)
    outs = m._encode_video_frames([(fr, 2.0), None], [vp, None])
    assert outs[1] is None and outs[0][1] == 2.0 and torch.equal(outs[0][0], rows)
    assert m._encode_video_frames([(fr, 2.0)])[0][0].shape == (5, 14)        # without paths: the encoders alone


def test_cli_arguments_and_cache_names(tmp_path):
    from v2a_amd import cli
    from v2a_amd.features import feature_cache_path, load_clip_cache
    assert feature_cache_path("/d/v.mp4", "clip_convnext") == "/d/v.generated.clip_convnext.npz"
    assert feature_cache_path("/d/v.mp4", "mixed") == "/d/v.generated.mixed.npz"
    vgg = "/ailab-train2/speech/zhanghaomin/VGGSound/"
    assert feature_cache_path(vgg + "video/a.mp4", "clip_convnext") == vgg + "feature_clip_convnext/a.npz"
    assert feature_cache_path(vgg + "video/a.mp4", "mixed") == vgg + "feature_mixed/a.npz"
    base = ["ck", "0", "scp", "0", "1", "out"]
    for choice in ("clip_convnext", "mixed"):
        a = cli.build_parser().parse_args(base + ["--video-encoder", choice, "--clip", "/m/dir"])
        assert a.video_encoder == choice and a.clip == "/m/dir"
        with pytest.raises(SystemExit):                                      # the choice comes with --clip DIR only
            cli.build_parser().parse_args(base + ["--video-encoder", choice])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--video-encoder", "convnext", "--clip", "/m/dir"])
    vp = str(tmp_path / "v.mp4")
    np.savez(str(tmp_path / "v.t5.npz"), np.zeros((3, 8), np.float32))
    enc = lambda path: (torch.arange(12, dtype=torch.float32).reshape(4, 3), 2.0)
    for choice in ("clip_convnext", "mixed"):
        reqs = cli.build_requests([(vp, "cap")], False, 30, clip_encode=enc, video_encoder=choice)
        emb, dur = load_clip_cache(str(tmp_path / f"v.generated.{choice}.npz"))
        assert dur == 2.0 and emb.shape == (4, 3) and reqs[0].clip_embed.shape == (30, 3)
    assert not os.path.exists(str(tmp_path / "v.generated.npz"))


def test_header_and_binding_declare_the_kernels():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ("v2a_convnext_dwconv", "v2a_convnext_pool_ln"):
        assert name in _lib.EXPORTS and f"int {name}(" in h
    assert _lib.ABI_VERSION == 9
    L = _lib.lib()
    # argument validation answers before any HIP call
    assert L.v2a_convnext_dwconv(16, 16, 16, 16, 1, 4, 4, 64, None) == -1 and b"in place" in L.v2a_last_error()
    assert L.v2a_convnext_dwconv(16, 32, 16, 16, 1, 4, 4, 62, None) == -1 and b"multiple of 4" in L.v2a_last_error()
    assert L.v2a_convnext_dwconv(None, 32, 16, 16, 1, 4, 4, 64, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_convnext_pool_ln(16, 64 * 4, 1, 4, 8192, 16, 16, 1e-5, 16, 8192, None) == -1 and b"4096" in L.v2a_last_error()
    assert L.v2a_convnext_pool_ln(16, 8, 1, 4, 64, 16, 16, 1e-5, 16, 64, None) == -1 and b"frame_stride" in L.v2a_last_error()


def test_kernels_have_no_scratch():
    import glob
    import re
    from v2a_amd import _lib
    _lib.build(verbose=False)
    paths = glob.glob(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build", "convnext-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert paths, "no device assembly for convnext.hip: csrc/build.sh must compile it with -save-temps=obj"
    found = []
    for b in open(paths[0]).read().split("- .agpr_count:")[1:]:
        n = re.search(r"\.name:\s+(\S+)", b).group(1)
        found.append(n)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
    assert len(found) == 2 and any("dwconv" in n for n in found) and any("pool_ln" in n for n in found)
