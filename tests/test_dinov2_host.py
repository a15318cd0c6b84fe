"""CPU: the host half of the DINOv2 image encoder (dinov2.py) -- key mapping, the SWIGLU row packing, the LayerScale fold, the
interpolated position table against the library's own call, the resize-then-crop tables against the processor's crops of the
fixtures, config refusals, the E2TTS / CLI wiring, and the SWIGLU instantiations' device assembly (no scratch)."""
import glob
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = dict(hidden_size=192, num_hidden_layers=2, num_attention_heads=3, mlp_ratio=4, image_size=70, patch_size=14, layer_norm_eps=1e-6,
             use_swiglu_ffn=True, num_channels=3)
RUN = dict(resize=64, crop=56)


def _sd(cfg=SMALL, seed=3, **kw):
    from v2a_amd.synth import random_dinov2_state_dict
    return random_dinov2_state_dict(cfg, seed, **kw)


def _enc(sd, cfg=SMALL, **kw):
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    return DINOv2ImageEncoder(sd, "cpu", config=cfg, **{**RUN, **kw})


def test_seeded_weights_load_into_the_library_model_and_are_reproducible():
    from transformers import Dinov2Config, Dinov2Model
    for cfg in (SMALL, dict(SMALL, use_swiglu_ffn=False)):
        a, b = _sd(cfg, 5), _sd(cfg, 5)
        assert all(torch.equal(a[k], b[k]) for k in a)
        m = Dinov2Model(Dinov2Config(**cfg))
        assert set(m.state_dict()) == set(a) and all(m.state_dict()[k].shape == a[k].shape for k in a)
        assert all(a[k].abs().max() > 0.01 for k in a if k.endswith("bias"))
        ls = torch.cat([a[k] for k in a if "layer_scale" in k])
        assert 0.05 <= float(ls.min()) < 0.2 and 0.8 < float(ls.max()) <= 1.0
    o = _sd(SMALL, 5, outlier=30.0)
    k = "encoder.layer.0.mlp.weights_out.weight"
    assert int((o[k].abs().amax(1) / _sd(SMALL, 5)[k].abs().amax(1) > 10).sum()) == 4


def test_key_mapping_with_and_without_prefix():
    sd = _sd()
    a = _enc(sd, compute="fp32")
    b = _enc({"image_encoder." + k: v for k, v in sd.items()}, compute="fp32")
    c = _enc({"model_state_dict": {"image_encoder." + k: v for k, v in sd.items()}}, cfg=None, compute="fp32")
    assert a.cfg == b.cfg == c.cfg and a.cfg["num_hidden_layers"] == 2 and a.T == 17 and a.dh == 64 and a.dff == 512 and a.swiglu
    for other in (b, c):
        assert all(torch.equal(x[k], y[k]) for x, y in zip(a.layers, other.layers) for k in ("qkv", "qkv_b", "o", "fc1", "fc2", "fc2_b"))
    P = "encoder.layer.1.attention.attention."
    assert torch.equal(a.layers[1]["qkv"], torch.cat([sd[P + f"{n}.weight"] for n in ("query", "key", "value")], 0))
    assert torch.equal(a.layers[1]["qkv_b"], torch.cat([sd[P + f"{n}.bias"] for n in ("query", "key", "value")], 0))
    assert torch.equal(a.patch_w[:, :588], sd["embeddings.patch_embeddings.projection.weight"].reshape(192, 588))
    assert a.kp == 640 and float(a.patch_w[:, 588:].abs().max()) == 0.0
    assert torch.equal(a.cls, sd["embeddings.cls_token"].reshape(192))
    split = _enc(sd, compute="bf16x3")
    w = split.layers[0]["fc1"]
    assert w.dtype == torch.bfloat16 and w.shape == (1024, 2 * 192)
    ref = a.layers[0]["fc1"]                  # hi + lo keeps 16 mantissa bits: |error| <= 2^-17 |w|
    assert float((w[:, :192].float() + w[:, 192:].float() - ref).abs().max()) <= 2.0 ** -17 * float(ref.abs().max())


def test_swiglu_row_packing_gate_is_x1_value_is_x2():
    from v2a_amd.dinov2 import pack_swiglu
    sd = _sd()
    w_in, b_in = sd["encoder.layer.0.mlp.weights_in.weight"], sd["encoder.layer.0.mlp.weights_in.bias"]
    a = _enc(sd, compute="fp32")
    pw, pb = a.layers[0]["fc1"], a.layers[0]["fc1_b"]
    hf = 512
    assert pw.shape == (2 * hf, 192) and torch.equal(pw, pack_swiglu(w_in))
    for g in range(hf // 16):
        assert torch.equal(pw[32 * g:32 * g + 16], w_in[hf + 16 * g:hf + 16 * g + 16])      # value = x2 = rows [Hf, 2 Hf)
        assert torch.equal(pw[32 * g + 16:32 * g + 32], w_in[16 * g:16 * g + 16])            # gate = x1 = rows [0, Hf)
        assert torch.equal(pb[32 * g:32 * g + 16], b_in[hf + 16 * g:hf + 16 * g + 16])
        assert torch.equal(pb[32 * g + 16:32 * g + 32], b_in[16 * g:16 * g + 16])
    # what the epilogue computes on the packed rows is what Dinov2SwiGLUFFN computes on the module's
    # (every output element as its own 192-term sum: a BLAS product may sum a row of W in an order that depends on where the row sits in the
    # matrix -- MKL does on some CPUs -- and the comparison below is bit for bit between two row orders)
    x = torch.randn(5, 192, dtype=torch.float64)
    lin = lambda w, b: (x[:, None, :] * w.double()[None]).sum(-1) + b.double()
    x1, x2 = lin(w_in, b_in).chunk(2, -1)
    acc = lin(pw, pb).view(5, hf // 16, 2, 16)
    assert torch.equal(acc[:, :, 0].reshape(5, hf) * torch.nn.functional.silu(acc[:, :, 1].reshape(5, hf)), torch.nn.functional.silu(x1) * x2)


def test_layerscale_fold_against_float64_product():
    for cfg in (SMALL, dict(SMALL, use_swiglu_ffn=False)):
        sd = _sd(cfg)
        a = _enc(sd, cfg, compute="fp32")
        assert a.swiglu == cfg["use_swiglu_ffn"] and a.dff == (512 if a.swiglu else 768)
        for i, Lw in enumerate(a.layers):
            p = f"encoder.layer.{i}."
            out = "mlp.weights_out." if a.swiglu else "mlp.fc2."
            for lam, lin, w, b in (("layer_scale1.lambda1", "attention.output.dense.", Lw["o"], Lw["o_b"]), ("layer_scale2.lambda1", out, Lw["fc2"], Lw["fc2_b"])):
                l64 = sd[p + lam].double()
                assert torch.equal(w, (l64[:, None] * sd[p + lin + "weight"].double()).float())
                assert torch.equal(b, (l64 * sd[p + lin + "bias"].double()).float())
        if not a.swiglu:
            assert torch.equal(a.layers[0]["fc1"], sd["encoder.layer.0.mlp.fc1.weight"])
    # split planes are taken from the folded float32 weight, not folded per plane
    from v2a_amd import _lib as L
    s = _enc(_sd(), compute="bf16x3")
    assert torch.equal(s.layers[0]["o"], L.split_planes(_enc(_sd(), compute="fp32").layers[0]["o"]))


@pytest.mark.parametrize("crop", [56, 70, 28, 112])
def test_interpolated_position_table_equals_the_library_call(crop):
    from transformers import Dinov2Config
    from transformers.models.dinov2.modeling_dinov2 import Dinov2Embeddings
    from v2a_amd.dinov2 import interpolate_positions
    sd = _sd()
    emb = Dinov2Embeddings(Dinov2Config(**SMALL))
    emb.load_state_dict({k[len("embeddings."):]: v for k, v in sd.items() if k.startswith("embeddings.")})
    g = crop // 14
    with torch.no_grad():
        want = emb.interpolate_pos_encoding(torch.zeros(1, 1 + g * g, 192), crop, crop)[0]
    got = interpolate_positions(sd["embeddings.position_embeddings"], g)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    if crop == 56:       # the encoder's rows: that table plus the patch projection's bias on the patch rows
        a = _enc(sd, compute="fp32")
        assert torch.equal(a.pos[0], want[0])
        assert torch.equal(a.pos[1:], (want[1:].double() + sd["embeddings.patch_embeddings.projection.bias"].double()).float())


@pytest.mark.parametrize("name", ["small", "wide"])
def test_resize_then_crop_tables_equal_the_processor_crops(name):
    from v2a_amd.clip import ResizePlan
    from v2a_amd.synth import synthetic_video_frames
    z = np.load(os.path.join(GOLDEN, f"dinov2_{name}.npz"))
    meta = json.loads(str(z["meta"]))
    seen = 0
    for cname, case in meta["cases"].items():
        for cl, n, h, w, seed in case["clips"]:
            key = f"{cname}_{cl}"
            fr = synthetic_video_frames(n, h, w, seed)
            assert [hashlib.md5(np.ascontiguousarray(f).tobytes()).hexdigest() for f in fr] == list(z[key + "_frames_md5"]), key
            rp = ResizePlan(h, w, case["crop"], case["resize"])
            assert rp.resize == case["resize"] and min(rp.out_hw) == case["resize"]
            got = rp.resize_numpy(fr[0])
            assert hashlib.md5(np.ascontiguousarray(got).tobytes()).hexdigest() == z[key + "_crop_md5"][0], key
            assert np.array_equal(got.reshape(-1)[z[key + "_crop_idx"]], z[key + "_crop_vals"][0])
            seen += 1
    assert seen >= 5


def test_resize_plan_default_is_unchanged_and_a_smaller_resize_is_refused():
    from v2a_amd.clip import ResizePlan
    a, b = ResizePlan(360, 640, 224), ResizePlan(360, 640, 224, 224)
    assert a.out_hw == b.out_hw and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("hb", "hk", "vb", "vk")) and (a.y0, a.rows) == (b.y0, b.rows)
    c = ResizePlan(360, 640, 224, 256)
    assert c.out_hw == (256, 455) and (c.top, c.left) == (16, 115)
    with pytest.raises(ValueError):
        ResizePlan(360, 640, 224, 200)


def test_normalize_table_matches_the_bit_processor():
    from transformers import BitImageProcessor
    from v2a_amd.clip import normalize_table
    from v2a_amd.dinov2 import IMAGENET_MEAN, IMAGENET_STD
    img = np.tile(np.arange(256, dtype=np.uint8)[None, :, None], (16, 1, 3))
    pv = BitImageProcessor(do_resize=False, do_center_crop=False, image_mean=list(IMAGENET_MEAN), image_std=list(IMAGENET_STD))(
        images=[img], return_tensors="np")["pixel_values"][0]
    lut = normalize_table(IMAGENET_MEAN, IMAGENET_STD)
    assert np.array_equal(pv.astype(np.float32), lut[np.arange(3)[:, None, None], img.transpose(2, 0, 1)])


def test_config_refusals(tmp_path):
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    sd = _sd()
    with pytest.raises(ValueError, match="64-wide"):
        _enc(sd, dict(SMALL, num_attention_heads=2))                 # 96-wide heads
    with pytest.raises(ValueError, match="64-wide"):
        _enc(sd, dict(SMALL, num_attention_heads=6))                 # 32-wide heads
    with pytest.raises(ValueError):
        _enc(sd, compute="bf16")
    with pytest.raises(ValueError):
        _enc(sd, chunk=0)
    with pytest.raises(ValueError):
        _enc(sd, crop=60)                                             # not a multiple of the patch size
    # from_pretrained: the preprocessor's sizes are read, a resample other than BICUBIC is refused
    d = tmp_path / "dinov2"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(SMALL, model_type="dinov2")))
    torch.save(sd, str(d / "pytorch_model.bin"))
    pc = dict(size={"shortest_edge": 64}, crop_size={"height": 56, "width": 56}, resample=3, image_mean=[0.5, 0.4, 0.3], image_std=[0.2, 0.3, 0.4])
    (d / "preprocessor_config.json").write_text(json.dumps(pc))
    e = DINOv2ImageEncoder.from_pretrained(str(d), "cpu", compute="fp32")
    assert (e.resize, e.S, e.T) == (64, 56, 17) and e.cfg["num_attention_heads"] == 3
    from v2a_amd.clip import normalize_table
    assert np.array_equal(e.lut.numpy(), normalize_table((0.5, 0.4, 0.3), (0.2, 0.3, 0.4)))
    (d / "preprocessor_config.json").write_text(json.dumps(dict(pc, resample=2)))
    with pytest.raises(NotImplementedError, match="BICUBIC"):
        DINOv2ImageEncoder.from_pretrained(str(d), "cpu")


def _small_e2tts(dim_text=192, **kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=dim_text, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_e2tts_wiring_under_dinov2():
    import v2a_amd
    from v2a_amd.dinov2 import DINOv2ImageEncoder
    assert v2a_amd.DINOv2ImageEncoder is DINOv2ImageEncoder and "DINOv2ImageEncoder" in v2a_amd.__all__
    sd = _sd()
    m = _small_e2tts(video_encoder="dinov2")
    enc = m.load_image_encoder(sd, config=SMALL, compute="fp32", **RUN)
    assert isinstance(enc, DINOv2ImageEncoder) and m.load_image_encoder(enc) is enc
    assert m.load_image_encoder({"image_encoder." + k: v for k, v in sd.items()}, config=SMALL, **RUN).d == 192
    with pytest.raises(TypeError):
        m.load_image_encoder(3)
    with pytest.raises(ValueError, match="dim_text"):
        _small_e2tts(dim_text=128, video_encoder="dinov2").load_image_encoder(sd, config=SMALL, **RUN)
    # the other choices of the reference are still refused, and clip_vit does not take a DINOv2 encoder's weights for CLIP's
    for other in ("clip_vit2", "clip_convnext", "mixed"):
        with pytest.raises(NotImplementedError):
            _small_e2tts(video_encoder=other).load_image_encoder(sd, config=SMALL)
    with pytest.raises(KeyError):
        _small_e2tts().load_image_encoder(sd)
    bare = _small_e2tts(video_encoder="dinov2")
    with pytest.raises(RuntimeError, match="load_image_encoder"):
        bare.sample(torch.zeros(1, 8, 16), video_frames=[(np.zeros((2, 8, 8, 3), np.uint8), 1.0)])


def test_cli_video_encoder_argument_and_cache_name(tmp_path):
    from v2a_amd import cli
    from v2a_amd.features import load_clip_cache
    base = ["ck", "0", "scp", "0", "1", "out"]
    assert cli.build_parser().parse_args(base).video_encoder == "clip_vit"
    assert cli.build_parser().parse_args(base + ["--video-encoder", "dinov2", "--clip", "/m/dinov2-giant"]).video_encoder == "dinov2"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--video-encoder", "clip_vit2"])
    vp = str(tmp_path / "v.mp4")
    np.savez(str(tmp_path / "v.t5.npz"), np.zeros((3, 8), np.float32))
    enc = lambda path: (torch.arange(12, dtype=torch.float32).reshape(4, 3), 2.0)
    reqs = cli.build_requests([(vp, "cap")], False, 30, clip_encode=enc, video_encoder="dinov2")
    emb, dur = load_clip_cache(str(tmp_path / "v.generated.dinov2.npz"))
    assert dur == 2.0 and emb.shape == (4, 3) and reqs[0].clip_embed.shape == (30, 3)
    assert not os.path.exists(str(tmp_path / "v.generated.npz"))


def test_header_and_binding_declare_swiglu():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    assert "V2A_EPI_SWIGLU = 7" in h and _lib.EPI_SWIGLU == 7 and _lib._EPI_NAMES[7] == "swiglu"
    assert _lib.ABI_VERSION == 9 and "v2a_abi_version" in _lib.EXPORTS


def test_swiglu_instantiations_have_no_scratch():
    """Every v2a_gemm kernel built with the SWIGLU epilogue (template argument 7): the exact-fp32 kernel's two tile shapes, the six
    split ring shapes and the split 8-phase kernel, each with fp32 and plane output -- no private segment, no spills."""
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    found = []
    for src in ("gemm", "gemm_8phase"):
        paths = glob.glob(os.path.join(build, f"{src}-hip-amdgcn-amd-amdhsa-gfx950.s"))
        assert paths, f"no device assembly for {src}.hip: csrc/build.sh must compile it with -save-temps=obj"
        for b in open(paths[0]).read().split("- .agpr_count:")[1:]:
            n = re.search(r"\.name:\s+(\S+)", b).group(1)
            if not re.search(r"gemm_(bf16_dma_|bf16_8ph_)?kernelI(fLb0E)?Li7E", n):
                continue
            found.append(n)
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
    assert len(found) == 2 + 2 * 6 + 2 * 2, found          # 8-phase: staggered and lock-step forms
