"""CPU: host side of the FLAN-T5 prompt encoder (v2a_amd.T5Encoder) -- bucket table, key mapping, config inference, weight
packing, argument checks, the E2TTS prompt path with a stubbed encoder, the CLI switch, the new C-ABI symbols and the fixture
generator."""
import ctypes
import glob
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(vocab_size=64, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, relative_attention_num_buckets=32,
            relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def _sd(cfg=TINY, seed=0):
    from v2a_amd.synth import random_t5_encoder_state_dict
    return random_t5_encoder_state_dict(cfg, seed)


def test_bucket_table_matches_transformers_every_length():
    T5Attention = pytest.importorskip("transformers.models.t5.modeling_t5").T5Attention
    from v2a_amd.t5 import relative_position_bucket_table
    for n in range(1, 513):
        pos = torch.arange(n, dtype=torch.long)
        ref = T5Attention._relative_position_bucket(pos[None, :] - pos[:, None], bidirectional=True, num_buckets=32, max_distance=128)
        tab = relative_position_bucket_table(n, 32, 128)
        got = tab[(pos[None, :] - pos[:, None]) + n - 1]
        assert torch.equal(got, ref), n


def test_key_mapping_and_config_inference():
    from v2a_amd.t5 import T5Encoder, infer_config
    sd = _sd()
    cfg = infer_config(sd)
    assert {k: cfg[k] for k in TINY} == TINY
    enc = T5Encoder(sd, "cpu")
    assert len(enc.layers) == 2 and enc.inner == 128 and enc.cfg["d_ff"] == 256
    # reference checkpoint layout: text_encoder2.* next to the sampler's own keys
    ck = {"text_encoder2." + k: v for k, v in sd.items()}
    ck["transformer.final_norm.g"] = torch.ones(4)
    enc2 = T5Encoder(ck, "cpu")
    assert torch.equal(enc2.layers[1]["wo"], enc.layers[1]["wo"]) and torch.equal(enc2.embed, enc.embed)
    assert torch.equal(T5Encoder({"model_state_dict": ck}, "cpu").final_ln, enc.final_ln)
    # tied embedding: only one of shared / embed_tokens present, either works
    for drop in ("shared.weight", "encoder.embed_tokens.weight"):
        one = {k: v for k, v in sd.items() if k != drop}
        assert torch.equal(T5Encoder(one, "cpu").embed, sd["shared.weight"])
    # q | k | v fused in that order
    P = "encoder.block.1.layer.0.SelfAttention."
    assert torch.equal(enc.layers[1]["qkv"], torch.cat([sd[P + "q.weight"], sd[P + "k.weight"], sd[P + "v.weight"]]))
    with pytest.raises(KeyError):
        T5Encoder({k: v for k, v in sd.items() if "shared" not in k and "embed_tokens" not in k}, "cpu")


def test_geglu_tanh_packing_order():
    from v2a_amd.t5 import pack_geglu
    rs = np.random.RandomState(0)
    wi0, wi1 = rs.standard_normal((64, 8)).astype(np.float32), rs.standard_normal((64, 8)).astype(np.float32)
    got = pack_geglu(torch.from_numpy(wi0), torch.from_numpy(wi1)).numpy()
    ref = np.zeros((128, 8), np.float32)
    for g in range(4):                                   # per 16 outputs: 16 value rows (wi_1), then 16 gate rows (wi_0)
        ref[32 * g:32 * g + 16] = wi1[16 * g:16 * g + 16]
        ref[32 * g + 16:32 * g + 32] = wi0[16 * g:16 * g + 16]
    assert np.array_equal(got, ref)


def test_argument_errors():
    from v2a_amd.t5 import T5Encoder
    enc = T5Encoder(_sd(), "cpu")
    ids = torch.ones(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="out of range"):
        enc.encode_ids(torch.tensor([[3, 64]]), torch.ones(1, 2))
    with pytest.raises(ValueError, match="out of range"):
        enc.encode_ids(torch.tensor([[-1, 3]]), None)
    with pytest.raises(ValueError, match="no valid key"):
        enc.encode_ids(ids, torch.tensor([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0]]))
    with pytest.raises(ValueError, match="512"):
        enc.encode_ids(torch.ones(1, 513, dtype=torch.long), None)
    with pytest.raises(ValueError, match="does not match"):
        enc.encode_ids(ids, torch.ones(2, 4))
    cfg = dict(TINY, d_kv=32, num_heads=4)
    with pytest.raises(ValueError, match="d_kv"):
        T5Encoder(_sd(cfg), "cpu")


class _StubTok:
    """Whitespace tokenizer with a fixed vocabulary: right padding with 0, EOS 1, like the T5 tokenizer's output format."""
    model_max_length = 512

    def __init__(self):
        self.calls = []

    def __call__(self, prompts, max_length, padding, truncation, return_tensors):
        assert padding is True and truncation is True and return_tensors == "pt"
        self.calls.append(list(prompts))
        rows = [[2 + (sum(map(ord, w)) % 60) for w in p.split()][:max_length - 1] + [1] for p in prompts]
        n = max(map(len, rows))
        ids = torch.tensor([r + [0] * (n - len(r)) for r in rows])
        return dict(input_ids=ids, attention_mask=(torch.arange(n)[None] < torch.tensor([len(r) for r in rows])[:, None]).long())


def _e2tts(**kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", device="cpu", **kw)


def test_prompt_path_substitutes_video_drop_prompt_and_respects_text_encoder_fn():
    from v2a_amd.t5 import T5Encoder
    tok = _StubTok()
    enc = T5Encoder(_sd(), "cpu", tokenizer=tok)
    seen = []

    def fake_encode(ids, am):
        seen.append((ids.clone(), torch.as_tensor(am).clone()))
        return torch.zeros(ids.shape[0], ids.shape[1], 128), torch.as_tensor(am).bool()
    enc.encode_ids = fake_encode
    m = _e2tts()
    with pytest.raises(NotImplementedError, match="FLAN-T5"):
        m._get_context(["a dog barks"], None, None, 1)
    assert m.load_text_encoder(enc) is enc
    prompts = ["a dog barks loudly", "rain", "piano music playing softly here"]
    ctx, cm = m._get_context(prompts, None, None, 3, [False, True, False])
    assert tok.calls == [["a dog barks loudly", "the sound of X X", "piano music playing softly here"]]
    assert prompts[1] == "rain"                                       # the caller's list is left alone
    assert ctx.shape == (3, 6, 128) and cm.sum(1).tolist() == [5, 6, 6]
    ids, _ = seen[-1]
    assert ids[1, :5].tolist() == tok(["the sound of X X"], 512, True, True, "pt")["input_ids"][0, :5].tolist()
    m._get_context(prompts, None, None, 3)                            # no drop flags: the prompts as given
    assert tok.calls[-1] == prompts
    # a state dict works as the source too, and text_encoder_fn still comes first
    fn_calls = []
    m2 = _e2tts(text_encoder_fn=lambda p: (fn_calls.append(p) or torch.ones(len(p), 2, 128), torch.ones(len(p), 2, dtype=torch.bool)))
    m2.load_text_encoder({"text_encoder2." + k: v for k, v in _sd().items()}, tokenizer=tok)
    n_tok = len(tok.calls)
    ctx2, _ = m2._get_context(["x y"], None, None, 1, [True])
    assert fn_calls == [["x y"]] and len(tok.calls) == n_tok and float(ctx2.sum()) == 256.0
    with pytest.raises(TypeError):
        m.load_text_encoder(3.5)


def test_load_state_dict_unchanged_by_text_encoder_keys():
    m = _e2tts()
    res = m.load_state_dict({"text_encoder2." + k: v for k, v in _sd().items()}, strict=False)
    assert all(k.startswith("text_encoder2.") for k in res.unexpected_keys) and len(res.unexpected_keys) > 0
    assert m._t5 is None


def test_cli_t5_engine_switch():
    from v2a_amd import cli
    base = ["ck.pt", "0", "list.scp", "0", "1", "out"]
    assert cli.build_parser().parse_args(base).t5_engine == "torch"
    assert cli.build_parser().parse_args(base + ["--t5", "d", "--t5-engine", "hip"]).t5_engine == "hip"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--t5-engine", "cuda"])


def test_new_symbols_exported_and_validated():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for s in ("v2a_t5_rmsnorm", "v2a_t5_attention", "v2a_gemm_skinny_f32"):
        assert s in _lib.EXPORTS and hasattr(L, s)
    g = _lib.GemmArgs()
    g.nseg, g.M, g.N, g.compute_dtype, g.a_dtype, g.out_dtype = 1, 64, 64, 0, 0, 0
    g.a[0], g.lda[0], g.ka[0], g.w, g.ldw, g.out, g.ldo = 4096, 64, 64, 8192, 64, 12288, 64
    g.epilogue = _lib.EPI_GEGLU_TANH
    assert L.v2a_gemm(ctypes.byref(g), None) == -1                    # v2a_gemm keeps rejecting epilogue 5
    g.epilogue = _lib.EPI_SIGMOID
    assert L.v2a_gemm_skinny_f32(ctypes.byref(g), None) == -1 and b"epilogue" in L.v2a_last_error()
    g.epilogue, g.ka[0] = _lib.EPI_STORE, 48
    assert L.v2a_gemm_skinny_f32(ctypes.byref(g), None) == -1 and b"K %" in L.v2a_last_error()
    g.ka[0], g.M = 64, 16 * 512 + 1
    assert L.v2a_gemm_skinny_f32(ctypes.byref(g), None) == -1
    a = _lib.T5AttnArgs()
    a.q = a.k = a.v = a.out = a.bias = a.key_mask = 4096
    a.B, a.H, a.N, a.d_kv = 1, 16, 8, 32
    assert L.v2a_t5_attention(ctypes.byref(a), None) == -1 and b"d_kv" in L.v2a_last_error()
    a.d_kv, a.N = 64, 513
    assert L.v2a_t5_attention(ctypes.byref(a), None) == -1 and b"N <= 512" in L.v2a_last_error()
    assert L.v2a_t5_rmsnorm(None, 0, None, 0, None, 0, None, 0, 1, 64, None, 1e-6, None) == -1


def test_header_declares_t5_entries_and_struct_mirror():
    src = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    assert re.search(r"V2A_EPI_GEGLU_TANH\s*=\s*5", src)
    body = re.search(r"typedef struct v2a_t5_attn_args \{(.*?)\} v2a_t5_attn_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*$", p.strip())[0] for d in body.split(";") for p in d.split(",") if p.strip()]
    from v2a_amd import _lib
    assert names == [f[0] for f in _lib.T5AttnArgs._fields_]


def test_t5_listing_has_no_scratch():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    path = glob.glob(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build", "t5-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert path, "no device assembly of t5.hip"
    text = open(path[0]).read()
    blocks = text.split("- .agpr_count:")[1:]
    assert len(blocks) >= 3
    for blk in blocks:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, name


def test_regenerated_small_fixture_matches_committed():
    pytest.importorskip("transformers")
    spec = importlib.util.spec_from_file_location("make_golden_t5", os.path.join(ROOT, "scripts", "make_golden_t5.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new = mod.run_case("small")
    old = np.load(os.path.join(GOLDEN, "t5_small.npz"))
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        if k == "meta":
            a, b = __import__("json").loads(str(old[k])), __import__("json").loads(new[k])
            a.pop("transformers"), b.pop("transformers")
            assert a == b
        elif old[k].dtype.kind == "i":
            assert np.array_equal(old[k], new[k]), k
        else:
            np.testing.assert_allclose(new[k], old[k], rtol=1e-6, atol=1e-6, err_msg=k)
