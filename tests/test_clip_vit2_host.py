"""CPU: the host half of the CLIP ViT-L/14-336 image encoder (clip.py CLIPViT2ImageEncoder) -- the QUICK_GELU enum in the header and the
binding, config inference on ViT-L/14-336 shapes, CLIPImageEncoder's own defaults, the E2TTS / CLI / cache-name wiring, and
from_pretrained on a temporary directory (nested vision_config, integer and dict sizes, refusals).  Nothing here touches a device."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
             projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu", num_channels=3)
SMALL104 = dict(hidden_size=208, intermediate_size=832, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                projection_dim=128, layer_norm_eps=1e-5, hidden_act="gelu", num_channels=3)


def _sd(cfg=SMALL, seed=3):
    from v2a_amd.synth import random_clip_vision_state_dict
    return random_clip_vision_state_dict(cfg, seed)


def test_header_and_binding_declare_quick_gelu():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    assert "V2A_EPI_QUICK_GELU = 9" in h and "x3:1426-1428" in h
    assert _lib.EPI_QUICK_GELU == 9 and _lib._EPI_NAMES[9] == "quick_gelu"
    assert _lib.ABI_VERSION == 9 and "v2a_abi_version" in _lib.EXPORTS
    # the values beside it are where they were
    assert (_lib.EPI_GELU, _lib.EPI_SWIGLU) == (6, 7) and "V2A_EPI_GELU = 6" in h and "V2A_EPI_CFG_EULER = 8" in h


def test_gemm_choice_treats_quick_gelu_as_gelu():
    """v2a_gemm_choose (nothing is launched): the kernel family, tile, stage count and grid of a QUICK_GELU launch are those of the GELU
    launch with the same arguments -- exact-fp32 compute at both tile sizes, split operands by shape and by every hint, fp32 and plane
    output -- and both are refused alike on plain bf16 compute."""
    from v2a_amd import _lib as L
    fields = [f for f, _ in L.GemmChoice._fields_]
    ch = lambda *a, **k: [getattr(L.gemm_choice(*a, **k), f) for f in fields]
    for M, N, K in ((514, 1024, 640), (577 * 2, 4096, 1024), (577 * 32, 4096, 1024)):
        a, w, b, o = torch.empty(M, K), torch.empty(N, K), torch.empty(N), torch.empty(M, N)
        got = [ch([(a, K, K)], w, o, M=M, N=N, compute=L.F32, epilogue=e, bias=b) for e in (L.EPI_GELU, L.EPI_QUICK_GELU)]
        assert got[0] == got[1], (M, N, K)
        As, Ws, osp = torch.empty(M, 2 * K, dtype=torch.bfloat16), torch.empty(N, 2 * K, dtype=torch.bfloat16), torch.empty(M, 2 * N, dtype=torch.bfloat16)
        for hint in range(8):
            for kw in (dict(), dict(out_split=True, ldo=2 * N)):
                got = [ch([(As, 2 * K, K)], Ws, osp if kw else o, M=M, N=N, compute=L.BF16, epilogue=e, bias=b, a_split=True, tile_hint=hint, **kw)
                       for e in (L.EPI_GELU, L.EPI_QUICK_GELU)]
                assert got[0] == got[1], (M, N, K, hint, kw)
        for e, name in ((L.EPI_GELU, "GELU"), (L.EPI_QUICK_GELU, "QUICK_GELU")):
            with pytest.raises(L.V2AError, match=name):
                L.gemm_choice([(As, 2 * K, 2 * K)], Ws, o, M=M, N=N, compute=L.BF16, epilogue=e, bias=b)


def test_quick_gelu_instantiations_have_no_scratch_and_a_gelu_twin():
    """Every v2a_gemm kernel built with the QUICK_GELU epilogue (template argument 9): the exact-fp32 kernel's two tile shapes, the six split
    ring shapes and the split 8-phase kernel's two forms, each of the latter with fp32 and plane output -- no private segment, no spills,
    and a GELU twin (template argument 6) for every one of them."""
    import glob
    import re
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    found = {6: [], 9: []}
    for src in ("gemm", "gemm_8phase"):
        paths = glob.glob(os.path.join(build, f"{src}-hip-amdgcn-amd-amdhsa-gfx950.s"))
        assert paths, f"no device assembly for {src}.hip: csrc/build.sh must compile it with -save-temps=obj"
        for b in open(paths[0]).read().split("- .agpr_count:")[1:]:
            n = re.search(r"\.name:\s+(\S+)", b).group(1)
            m = re.search(r"gemm_(?:bf16_dma_|bf16_8ph_)?kernelI(?:fLb0E)?Li([69])E", n)
            if not m:
                continue
            found[int(m.group(1))].append(n)
            if m.group(1) == "9":
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
                assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
    assert len(found[9]) == 2 + 2 * 6 + 2 * 2, found[9]
    as_gelu = sorted(re.sub(r"kernelI((?:fLb0E)?)Li9E", r"kernelI\1Li6E", n) for n in found[9])
    assert as_gelu == sorted(found[6]), (as_gelu, found[6])


def test_vit_l_14_336_config_is_inferred_from_shapes():
    """Meta tensors of the real shapes: 16 heads of 64 and quick_gelu are the subclass's defaults, the rest is read off the shapes."""
    from v2a_amd.clip import CLIPViT2ImageEncoder, infer_config
    from v2a_amd.synth import VIT_L_14_336
    c = VIT_L_14_336
    assert (c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["num_attention_heads"]) == (1024, 4096, 24, 16)
    assert (c["image_size"], c["patch_size"], c["projection_dim"], c["hidden_act"]) == (336, 14, 768, "quick_gelu")
    d, dff, T = 1024, 4096, 577
    with torch.device("meta"):
        sd = {"vision_model.embeddings.patch_embedding.weight": torch.empty(d, 3, 14, 14),
              "vision_model.embeddings.position_embedding.weight": torch.empty(T, d),
              "visual_projection.weight": torch.empty(768, d)}
        for i in range(24):
            sd[f"vision_model.encoder.layers.{i}.mlp.fc1.weight"] = torch.empty(dff, d)
    got = infer_config(sd, CLIPViT2ImageEncoder._HEAD_DIM, CLIPViT2ImageEncoder._HIDDEN_ACT)
    assert got == c
    # CLIPImageEncoder's own inference: 104-wide heads and gelu, as before (hidden 1024 is then no multiple of the head width)
    own = infer_config(sd)
    assert own["num_attention_heads"] == 1024 // 104 == 9 and own["hidden_act"] == "gelu" and 1024 % 9


def test_subclass_defaults_on_a_tiny_state_dict():
    from v2a_amd import _lib as L
    from v2a_amd.clip import CLIPImageEncoder, CLIPViT2ImageEncoder
    sd = _sd()
    e = CLIPViT2ImageEncoder(sd, "cpu", compute="fp32")                        # no config at all
    assert e.cfg == SMALL and (e.H, e.dh, e.T, e.S, e.resize) == (2, 64, 17, 56, 56)
    assert e.ffn == (L.EPI_QUICK_GELU, 256) and e.mfma_attention and e.dp == 128 and e.out_dim == 64
    assert e._attn_frames(1) == 1                                              # 17 keys: no key split, no floor
    # the base class on the same weights: its own defaults make 128 / (128 // 104) = 128-wide heads a ValueError; given 64-wide heads it
    # runs them on the MFMA attention, with its own gelu; quick_gelu stays the subclass's alone
    with pytest.raises(ValueError):
        CLIPImageEncoder(sd, "cpu", compute="fp32")
    b = CLIPImageEncoder(sd, "cpu", config=dict(SMALL, hidden_act="gelu"), compute="bf16x3")
    assert b.ffn == (L.EPI_GELU, 256) and b.mfma_attention
    with pytest.raises(NotImplementedError, match="CLIPViT2ImageEncoder"):
        CLIPImageEncoder(sd, "cpu", config=SMALL)
    g = CLIPViT2ImageEncoder(sd, "cpu", config=dict(SMALL, hidden_act="gelu"), compute="fp32")
    assert g.ffn == (L.EPI_GELU, 256)
    # 104-wide heads: the VALU attention, gelu unless the config says otherwise, K padded to 256
    sd104 = _sd(SMALL104)
    c = CLIPImageEncoder(sd104, "cpu", compute="fp32")
    assert c.cfg == SMALL104 and c.ffn == (L.EPI_GELU, 832) and not c.mfma_attention and (c.dh, c.dp) == (104, 256)
    q = CLIPViT2ImageEncoder(sd104, "cpu", config=dict(num_attention_heads=2), compute="fp32")
    assert q.ffn == (L.EPI_QUICK_GELU, 832) and not q.mfma_attention and q.cfg["hidden_act"] == "quick_gelu"
    for act in ("relu", "gelu_new"):
        for cls in (CLIPImageEncoder, CLIPViT2ImageEncoder):
            with pytest.raises(NotImplementedError, match="hidden_act"):
                cls(sd, "cpu", config=dict(SMALL, hidden_act=act))


def test_attention_floor_at_577_tokens_is_the_engines():
    """The floor on the workgroups of an attention launch lives in the engine: at T = 577 and 16 heads a frame has 160 workgroups, so a
    bf16x3 launch never covers fewer than 2 frames; fp32 and the VALU path have none."""
    from v2a_amd import dinov2, vit
    from v2a_amd.clip import CLIPViT2ImageEncoder
    assert vit._ATTN_KEY_SPLIT_BELOW == 200 and not hasattr(dinov2, "_ATTN_KEY_SPLIT_BELOW")
    assert "_attn_frames" not in vars(dinov2.DINOv2ImageEncoder) and "attention" not in vars(dinov2.DINOv2ImageEncoder)
    e = object.__new__(CLIPViT2ImageEncoder)
    e.H, e.T, e.split, e.mfma_attention = 16, 577, True, True
    assert [e._attn_frames(f) for f in (1, 2, 3, 32)] == [2, 2, 3, 32]
    e.split = False
    assert e._attn_frames(1) == 1
    e.split, e.mfma_attention = True, False
    assert e._attn_frames(1) == 1
    e.mfma_attention, e.T = True, 128
    assert e._attn_frames(1) == 1


def _small_e2tts(dim_text=64, **kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=dim_text, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_e2tts_wiring_under_clip_vit2(tmp_path):
    import v2a_amd
    from v2a_amd.clip import CLIPImageEncoder, CLIPViT2ImageEncoder
    from v2a_amd.e2tts import IMAGE_ENCODERS
    assert v2a_amd.CLIPViT2ImageEncoder is CLIPViT2ImageEncoder and "CLIPViT2ImageEncoder" in v2a_amd.__all__
    assert IMAGE_ENCODERS["clip_vit2"] is CLIPViT2ImageEncoder and IMAGE_ENCODERS["clip_vit"] is CLIPImageEncoder
    sd = _sd()
    m = _small_e2tts(video_encoder="clip_vit2")
    enc = CLIPViT2ImageEncoder(sd, "cpu", compute="fp32")
    assert m.load_image_encoder(enc) is enc and m._clip is enc
    d = tmp_path / "clip-vit-large-patch14-336"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(vision_config=SMALL)))
    torch.save({"image_encoder." + k: v for k, v in sd.items()}, str(d / "pytorch_model.bin"))
    from_dir = m.load_image_encoder(str(d), compute="fp32")
    assert type(from_dir) is CLIPViT2ImageEncoder and from_dir.cfg == SMALL and from_dir.d == 128
    # a bare state dict is refused under this choice (it names neither the activation nor the head width)
    with pytest.raises(NotImplementedError, match="state dict"):
        m.load_image_encoder(sd, compute="fp32")
    with pytest.raises(TypeError):
        m.load_image_encoder(3)
    with pytest.raises(ValueError, match="dim_text"):
        _small_e2tts(dim_text=128, video_encoder="clip_vit2").load_image_encoder(enc)
    with pytest.raises(ValueError, match="dim_text"):
        _small_e2tts(dim_text=128, video_encoder="clip_vit2").load_image_encoder(str(d))
    # clip_vit keeps its behaviour: no check of the width, and its own class
    assert type(_small_e2tts(dim_text=32).load_image_encoder(_sd(SMALL104), compute="fp32")) is CLIPImageEncoder
    for other in ("clip_convnext", "mixed"):
        with pytest.raises(NotImplementedError, match="clip_vit2"):
            _small_e2tts(video_encoder=other).load_image_encoder(sd)
    bare = _small_e2tts(video_encoder="clip_vit2")
    with pytest.raises(RuntimeError, match="load_image_encoder"):
        bare.sample(torch.zeros(1, 8, 16), video_frames=[(np.zeros((2, 8, 8, 3), np.uint8), 1.0)])


def test_cli_video_encoder_argument_and_cache_name(tmp_path):
    from v2a_amd import cli
    from v2a_amd.features import feature_cache_path, load_clip_cache
    assert feature_cache_path("/d/v.mp4", "clip_vit2") == "/d/v.generated.clip_vit2.npz"
    vgg = "/ailab-train2/speech/zhanghaomin/VGGSound/"                       # the reference's own tree keeps the features beside /video/
    assert feature_cache_path(vgg + "video/a.mp4", "clip_vit2") == vgg + "feature_clip_vit2/a.npz"
    base = ["ck", "0", "scp", "0", "1", "out"]
    a = cli.build_parser().parse_args(base + ["--video-encoder", "clip_vit2", "--clip", "/m/clip-vit-large-patch14-336"])
    assert a.video_encoder == "clip_vit2" and a.clip == "/m/clip-vit-large-patch14-336"
    assert cli.build_parser().parse_args(base).video_encoder == "clip_vit"
    for bad in (["--video-encoder", "mixed"], ["--video-encoder", "clip_vit2"]):       # the choice comes with --clip DIR only
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
    vp = str(tmp_path / "v.mp4")
    np.savez(str(tmp_path / "v.t5.npz"), np.zeros((3, 8), np.float32))
    enc = lambda path: (torch.arange(12, dtype=torch.float32).reshape(4, 3), 2.0)
    reqs = cli.build_requests([(vp, "cap")], False, 30, clip_encode=enc, video_encoder="clip_vit2")
    emb, dur = load_clip_cache(str(tmp_path / "v.generated.clip_vit2.npz"))
    assert dur == 2.0 and emb.shape == (4, 3) and reqs[0].clip_embed.shape == (30, 3)
    assert not os.path.exists(str(tmp_path / "v.generated.npz"))


def test_from_pretrained_reads_config_and_preprocessor(tmp_path):
    from v2a_amd.clip import CLIPViT2ImageEncoder, normalize_table
    from v2a_amd.resample import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    sd = _sd()
    d = tmp_path / "clip-vit-large-patch14-336"
    d.mkdir()
    torch.save(sd, str(d / "pytorch_model.bin"))
    # a whole CLIPConfig: the vision tower's fields are nested; no preprocessor_config.json: the model's own sizes, OpenAI's mean / std
    (d / "config.json").write_text(json.dumps(dict(model_type="clip", projection_dim=64, text_config=dict(hidden_size=32),
                                                   vision_config=dict(SMALL, model_type="clip_vision_model"))))
    e = CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert e.cfg == SMALL and (e.resize, e.S, e.T) == (56, 56, 17)
    assert np.array_equal(e.lut.numpy(), normalize_table(OPENAI_CLIP_MEAN, OPENAI_CLIP_STD))
    # a flat CLIPVisionConfig without hidden_act / heads: the subclass's defaults
    flat = {k: v for k, v in SMALL.items() if k not in ("hidden_act", "num_attention_heads")}
    (d / "config.json").write_text(json.dumps(flat))
    e = CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert e.cfg == SMALL
    pp = d / "preprocessor_config.json"
    # the dict forms (the processor's current layout), with a resize target above the crop and other statistics
    pc = dict(do_resize=True, do_center_crop=True, do_normalize=True, size={"shortest_edge": 64}, crop_size={"height": 56, "width": 56}, resample=3,
              image_mean=[0.5, 0.4, 0.3], image_std=[0.2, 0.3, 0.4])
    pp.write_text(json.dumps(pc))
    e = CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert (e.resize, e.S) == (64, 56) and np.array_equal(e.lut.numpy(), normalize_table((0.5, 0.4, 0.3), (0.2, 0.3, 0.4)))
    # the legacy integer forms (openai/clip-vit-large-patch14-336 ships size = 336, crop_size = 336): the integer size is the shortest edge
    pp.write_text(json.dumps(dict(size=56, crop_size=56, resample=3, image_mean=list(OPENAI_CLIP_MEAN), image_std=list(OPENAI_CLIP_STD))))
    e = CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert (e.resize, e.S) == (56, 56) and np.array_equal(e.lut.numpy(), normalize_table())
    # a keyword of the caller wins over the file
    assert CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32", resize=60).resize == 60
    # refusals
    pp.write_text(json.dumps(dict(pc, resample=2)))
    with pytest.raises(NotImplementedError, match="BICUBIC"):
        CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu")
    pp.write_text(json.dumps(dict(pc, crop_size={"height": 56, "width": 42})))
    with pytest.raises(NotImplementedError, match="square"):
        CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu")
    for k in ("do_resize", "do_center_crop", "do_normalize"):
        pp.write_text(json.dumps(dict(pc, **{k: False})))
        with pytest.raises(NotImplementedError, match=k):
            CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu")
    pp.write_text(json.dumps(dict(pc, crop_size=42)))
    with pytest.raises(NotImplementedError, match="image size"):
        CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu")
    pp.write_text(json.dumps(dict(pc, size={"shortest_edge": 42})))
    with pytest.raises(ValueError, match="resize"):
        CLIPViT2ImageEncoder.from_pretrained(str(d), "cpu")
