"""CPU: the host half of the CLIP image encoder (clip.py) -- Pillow's integer BICUBIC resample restated from the module's own
coefficient tables, the processor's normalise table, key mapping and config refusals, the E2TTS / CLI wiring, and the device
assembly of csrc/clip.hip (no scratch)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(hidden_size=208, intermediate_size=832, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
             projection_dim=128, layer_norm_eps=1e-5, hidden_act="gelu", num_channels=3)


def _pil_crop(img, S):
    from PIL import Image
    from v2a_amd.clip import ResizePlan
    rp = ResizePlan(img.shape[0], img.shape[1], S)
    oh, ow = rp.out_hw
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC, reducing_gap=None))
    return rp, ref[rp.top:rp.top + S, rp.left:rp.left + S]


@pytest.mark.parametrize("hw", [(224, 224), (250, 300), (360, 640), (640, 360), (448, 700), (900, 1344), (1344, 900), (150, 200),
                                (97, 50), (227, 301), (1350, 1500)])
def test_integer_resize_is_bit_equal_to_pillow(hw):
    """Downscale 1x .. 6x, upscale, both orientations: the two integer passes over the host tables equal PIL.Image.resize(BICUBIC,
    reducing_gap=None) followed by the centre crop, byte for byte."""
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    smooth = np.cumsum(rng.normal(0, 6, hw + (3,)), axis=1)
    img = np.clip(128 + smooth - smooth.mean() + rng.normal(0, 30, hw + (3,)), 0, 255).astype(np.uint8)
    for S in (224, 56):
        rp, ref = _pil_crop(img, S)
        assert np.array_equal(rp.resize_numpy(img), ref), (hw, S)
        # the tables stay inside the image: what the kernels read
        assert (rp.hb[:, 0] + rp.hb[:, 1] <= hw[1]).all() and (rp.vb[:, 0] + rp.vb[:, 1] <= rp.rows).all()


def test_resize_output_size_matches_transformers():
    from transformers.image_transforms import get_resize_output_image_size
    from v2a_amd.clip import resize_output_size
    for h, w in [(360, 640), (640, 360), (150, 200), (227, 301), (224, 224), (97, 50)]:
        want = get_resize_output_image_size(np.zeros((h, w, 3), np.uint8), size=224, default_to_square=False)
        assert resize_output_size(h, w, 224) == tuple(want), (h, w)


def test_normalize_table_matches_processor():
    from transformers import CLIPImageProcessor
    from v2a_amd.clip import normalize_table
    img = np.tile(np.arange(256, dtype=np.uint8)[None, :, None], (224, 1, 3))
    img = np.concatenate([img, img[:, :-32]], 1)[:, :224]                       # every byte value in every channel, 224 x 224
    pv = CLIPImageProcessor(do_resize=False, do_center_crop=False)(images=[img], return_tensors="np")["pixel_values"][0]
    lut = normalize_table()
    want = lut[np.arange(3)[:, None, None], img.transpose(2, 0, 1)]
    assert np.array_equal(pv.astype(np.float32), want)


def test_key_mapping_and_config_refusals():
    from v2a_amd.clip import CLIPImageEncoder
    from v2a_amd.synth import random_clip_vision_state_dict
    sd = random_clip_vision_state_dict(SMALL, 3)
    a = CLIPImageEncoder(sd, "cpu", config=SMALL, compute="fp32")
    b = CLIPImageEncoder({"image_encoder." + k: v for k, v in sd.items()}, "cpu", config=SMALL, compute="fp32")
    assert a.cfg == b.cfg and a.cfg["num_hidden_layers"] == 2 and a.T == 17 and a.dh == 104
    assert torch.equal(a.layers[1]["qkv"][:, :208], torch.cat([sd[f"vision_model.encoder.layers.1.self_attn.{n}_proj.weight"] for n in "qkv"], 0))
    assert torch.equal(a.layers[1]["qkv"][:, 208:], torch.zeros(624, 48))        # K zero-padded to 256
    assert torch.equal(a.patch_w[:, :588], sd["vision_model.embeddings.patch_embedding.weight"].reshape(208, 588))
    split = CLIPImageEncoder(sd, "cpu", config=SMALL, compute="bf16x3")
    w = split.layers[0]["fc2"]
    assert w.dtype == torch.bfloat16 and w.shape == (208, 2 * 832)
    assert torch.allclose(w[:, :832].float() + w[:, 832:].float(), sd["vision_model.encoder.layers.0.mlp.fc2.weight"], rtol=0, atol=1e-6)
    for act in ("quick_gelu", "gelu_new", "relu"):
        with pytest.raises(NotImplementedError):
            CLIPImageEncoder(sd, "cpu", config=dict(SMALL, hidden_act=act))
    with pytest.raises(ValueError):
        CLIPImageEncoder(sd, "cpu", config=SMALL, compute="bf16")
    with pytest.raises(ValueError):
        CLIPImageEncoder(sd, "cpu", config=SMALL, chunk=0)


def test_seeded_weights_are_reproducible_and_exercise_every_term():
    from v2a_amd.synth import random_clip_vision_state_dict
    a, b = random_clip_vision_state_dict(SMALL, 5), random_clip_vision_state_dict(SMALL, 5)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(a[k].abs().min() > 0 or a[k].abs().max() > 0.01 for k in a if k.endswith("bias"))
    assert all((a[k] - 1).abs().max() > 0.01 for k in a if "norm" in k and k.endswith("weight"))
    o = random_clip_vision_state_dict(SMALL, 5, outlier=30.0)
    r = o["vision_model.encoder.layers.0.mlp.fc2.weight"].abs().amax(1) / a["vision_model.encoder.layers.0.mlp.fc2.weight"].abs().amax(1)
    assert int((r > 10).sum()) == 4


def _small_e2tts(**kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=128, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_e2tts_image_encoder_wiring_refusals(tmp_path):
    from v2a_amd.clip import CLIPImageEncoder
    from v2a_amd.synth import random_clip_vision_state_dict
    sd = random_clip_vision_state_dict(SMALL, 3)
    with pytest.raises(NotImplementedError):
        _small_e2tts(video_encoder="clip_vit2").load_image_encoder(sd, config=SMALL)
    m = _small_e2tts()
    enc = m.load_image_encoder(sd, config=SMALL, compute="fp32")
    assert isinstance(enc, CLIPImageEncoder) and m.load_image_encoder(enc) is enc
    with pytest.raises(TypeError):
        m.load_image_encoder(3)
    # the checkpoint loader still reports image_encoder.* as unexpected
    res = _small_e2tts().load_state_dict({"image_encoder." + k: v for k, v in list(sd.items())[:3]}, strict=False)
    assert res.unexpected_keys and all(k.startswith("image_encoder.") for k in res.unexpected_keys)
    # no encoder: video_frames is refused, and the missing-cache error of video_paths is unchanged
    bare = _small_e2tts()
    with pytest.raises(RuntimeError, match="load_image_encoder"):
        bare.sample(torch.zeros(1, 8, 16), video_frames=[(np.zeros((2, 8, 8, 3), np.uint8), 1.0)])
    with pytest.raises(FileNotFoundError):
        bare.sample(torch.zeros(1, 8, 16), video_paths=[str(tmp_path / "a.mp4")])


def test_cli_clip_argument_and_missing_cache(tmp_path):
    from v2a_amd import cli
    from v2a_amd.features import load_clip_cache
    a = cli.build_parser().parse_args(["ck", "0", "scp", "0", "1", "out", "--clip", "/models/image_encoder"])
    assert a.clip == "/models/image_encoder"
    assert cli.build_parser().parse_args(["ck", "0", "scp", "0", "1", "out"]).clip is None
    vp = str(tmp_path / "v.mp4")
    np.savez(str(tmp_path / "v.t5.npz"), np.zeros((3, 8), np.float32))
    with pytest.raises(FileNotFoundError, match="--clip"):
        cli.build_requests([(vp, "cap")], False, 30)
    calls = []

    def enc(path):
        calls.append(path)
        return torch.arange(12, dtype=torch.float32).reshape(4, 3), 2.0
    reqs = cli.build_requests([(vp, "cap")], False, 30, clip_encode=enc)
    emb, dur = load_clip_cache(str(tmp_path / "v.generated.npz"))
    assert calls == [vp] and dur == 2.0 and emb.shape == (4, 3) and reqs[0].clip_embed.shape == (30, 3)
    cli.build_requests([(vp, "cap")], False, 30, clip_encode=enc)             # the cache wins now
    assert calls == [vp]


def test_clip_device_assembly_has_no_scratch():
    """The rule of test_isa_guard.py (whose source list is fixed) for csrc/clip.hip."""
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    paths = glob.glob(os.path.join(build, "clip-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert paths, "no device assembly for clip.hip: csrc/build.sh must compile it with -save-temps=obj"
    text = open(paths[0]).read()
    blocks = text.split("- .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert sum("clip_" in n for n in names) == 5, names
    for b, n in zip(blocks, names):
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n


def test_header_declares_clip_entries_and_struct_mirror():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ("v2a_clip_resize_h", "v2a_clip_resize_v", "v2a_clip_embed_init", "v2a_clip_layernorm", "v2a_clip_attention"):
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS
    assert "V2A_EPI_GELU = 6" in h and _lib.EPI_GELU == 6
    fields = re.search(r"typedef struct v2a_clip_attn_args \{(.*?)\} v2a_clip_attn_args;", h, re.S).group(1)
    assert [f for f, _ in _lib.ClipAttnArgs._fields_] == re.findall(r"\b(\w+)[,;]", re.sub(r"/\*.*?\*/", "", fields).replace("*", " "))
