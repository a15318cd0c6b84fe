"""CPU: host side of the Encodec quantizer (v2a_amd.EncodecQuantizer) -- the C-ABI symbols, both key layouts, the bandwidth rule,
the plain-torch restatement against the float64 vectors of the library's own quantizer (tests/golden/encodec_rvq.npz, made by
scripts/make_golden_encodec_rvq.py), the refusals, the CLI flag and the device assembly of the new kernels."""
import glob
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from v2a_amd.encodec import (EncodecQuantizer, num_quantizers_for_bandwidth, quantizer_codebooks,  # fails at import without the feature
                             rvq_decode_torch, rvq_encode_torch)
from v2a_amd.synth import random_encodec_quantizer_state_dict, synthetic_encodec_latents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "encodec_rvq.npz")
CASES = [f"{fam}_{b}x{t}" for fam in ("structured", "gaussian") for b, t in ((2, 750), (3, 17), (1, 1))]
BANDWIDTH_STAGES = ((1.5, 2), (3.0, 4), (6.0, 8), (12.0, 16), (24.0, 32))


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD, allow_pickle=False))
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def codebooks(gold):
    cb = quantizer_codebooks(random_encodec_quantizer_state_dict(gold["meta"]["param_seed"]))
    assert hashlib.md5(cb.numpy().tobytes()).hexdigest() == gold["meta"]["codebooks_md5"]
    return cb


def latents(gold, codebooks, name):
    """The case's input, regenerated from its seed and checked against the md5 the fixture recorded."""
    fam, shape = name.split("_")
    b, t = (int(v) for v in shape.split("x"))
    c = gold["meta"]["cases"][name]
    x = synthetic_encodec_latents(codebooks, b, t, c["seed"], structured=fam == "structured")
    assert x.shape == (b, 128, t) and hashlib.md5(x.numpy().tobytes()).hexdigest() == c["md5"], name
    return x


def test_new_symbols_are_declared_exported_and_check_arguments():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ("v2a_encodec_rvq_encode", "v2a_encodec_rvq_decode"):
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS
    assert "EncodecEuclideanCodebook.quantize" in h and "EncodecResidualVectorQuantizer.encode" in h
    assert "EncodecResidualVectorQuantizer.decode" in h
    assert _lib.ABI_VERSION == 9
    L = _lib.lib()
    enc = lambda x=4096, cb=4096, S=32, Kc=1024, D=128, n_q=32, B=1, T=5, st=(640, 1, 5): L.v2a_encodec_rvq_encode(
        x, *st, B, T, cb, 8192, S, Kc, D, n_q, 16384, None)
    assert enc(x=None) == -1 and b"null" in L.v2a_last_error()
    assert enc(D=64) == -1 and b"D=64" in L.v2a_last_error()
    assert enc(Kc=1000) == -1 and b"Kc=1000" in L.v2a_last_error()
    assert enc(n_q=33) == -1 and b"n_q=33" in L.v2a_last_error()
    assert enc(T=0) == -1 and b"T=0" in L.v2a_last_error()
    assert enc(st=(640, -1, 5)) == -1 and b"stride" in L.v2a_last_error()
    assert enc(cb=4100) == -1 and b"alignment" in L.v2a_last_error()
    dec = lambda codes=4096, S=32, Kc=1024, D=128, n_q=32, B=1, T=5, out=8192: L.v2a_encodec_rvq_decode(
        codes, n_q, B, T, 16384, S, Kc, D, out, 640, 1, 5, None)
    assert dec(codes=None) == -1 and b"null" in L.v2a_last_error()
    assert dec(D=96) == -1 and b"D=96" in L.v2a_last_error()
    assert dec(n_q=0) == -1 and b"n_q=0" in L.v2a_last_error()
    assert dec(codes=4100) == -1 and b"alignment" in L.v2a_last_error()


def test_rvq_device_assembly_has_no_scratch():
    """The rule of test_clip_host.py::test_clip_device_assembly_has_no_scratch for csrc/encodec_rvq.hip."""
    from v2a_amd import _lib
    _lib.build(verbose=False)
    build = os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build")
    paths = glob.glob(os.path.join(build, "encodec_rvq-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert paths, "no device assembly for encodec_rvq.hip: csrc/build.sh must compile it with -save-temps=obj"
    text = open(paths[0]).read()
    blocks = text.split("- .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert sum("rvq_encode" in n or "rvq_decode" in n for n in names) == 2, names
    for b, n in zip(blocks, names):
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
    assert "v_mfma_f32_16x16x4_f32" in text or "v_mfma_f32_16x16x4f32" in text      # the exact-fp32 matrix instruction, not a bf16 one


def test_both_key_layouts_load_to_identical_codebooks():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    sd = random_encodec_quantizer_state_dict(3)
    assert torch.equal(random_encodec_quantizer_state_dict(3)["layers.31.codebook.embed"], sd["layers.31.codebook.embed"])      # seeded
    own = EncodecQuantizer(sd, "cpu")
    model = {"quantizer." + k: v for k, v in sd.items()}
    model["decoder.layers.0.conv.bias"] = torch.zeros(3)            # the rest of an EncodecModel state dict is ignored
    model["encoder.layers.0.conv.bias"] = torch.zeros(3)
    full = EncodecQuantizer(model, "cpu")
    bare = EncodecQuantizer({k: v for k, v in sd.items() if k.endswith(".embed")}, "cpu")       # training statistics are not needed
    for q in (own, full, bare):
        assert (q.num_quantizers, q.codebook_size, q.dim) == (32, 1024, 128)
        assert torch.equal(q.codebooks, own.codebooks) and torch.equal(q.norms, own.norms)
    assert torch.equal(own.codebooks[7], sd["layers.7.codebook.embed"])
    torch.testing.assert_close(own.norms, own.codebooks.pow(2).sum(-1), rtol=1e-6, atol=0)
    # scale falls by stage as 0.85^s
    rms = own.codebooks.double().pow(2).mean((1, 2)).sqrt()
    torch.testing.assert_close(rms, 0.85 ** torch.arange(32, dtype=torch.float64), rtol=0.02, atol=0)
    with pytest.raises(KeyError, match="codebook.embed"):
        EncodecQuantizer({"decoder.layers.0.conv.bias": torch.zeros(3)}, "cpu")
    with pytest.raises(ValueError, match="multiple of 512"):
        EncodecQuantizer(random_encodec_quantizer_state_dict(1, num_quantizers=2, codebook_size=100), "cpu")
    with pytest.raises(ValueError, match="dimension 128"):
        EncodecQuantizer(random_encodec_quantizer_state_dict(1, num_quantizers=2, codebook_size=512, dim=64), "cpu")


def test_generated_state_dict_loads_strictly_into_the_library():
    tf = pytest.importorskip("transformers")
    from transformers.models.encodec.modeling_encodec import EncodecResidualVectorQuantizer
    q = EncodecResidualVectorQuantizer(tf.EncodecConfig(target_bandwidths=[1.5, 3.0, 6.0, 12.0, 24.0]))
    res = q.load_state_dict(random_encodec_quantizer_state_dict(3), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_bandwidth_to_stages_table():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    q = EncodecQuantizer(random_encodec_quantizer_state_dict(1), "cpu")
    for bw, n in BANDWIDTH_STAGES:
        assert q.num_quantizers_for_bandwidth(bw) == n == num_quantizers_for_bandwidth(bw, 1024, 32)
    assert q.num_quantizers_for_bandwidth(None) == q.num_quantizers_for_bandwidth(0) == q.num_quantizers_for_bandwidth(0.0) == 32
    assert q.num_quantizers_for_bandwidth(0.1) == 1 and q.num_quantizers_for_bandwidth(48.0) == 32       # at least one, at most all
    tf = pytest.importorskip("transformers")
    from transformers.models.encodec.modeling_encodec import EncodecResidualVectorQuantizer
    lib = EncodecResidualVectorQuantizer(tf.EncodecConfig(target_bandwidths=[1.5, 3.0, 6.0, 12.0, 24.0]))
    for bw in (None, 0.0, 0.1, 1.5, 3.0, 6.0, 12.0, 24.0):
        assert lib.get_num_quantizers_for_bandwidth(bw) == q.num_quantizers_for_bandwidth(bw), bw


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_reproduces_the_library_vectors(gold, codebooks, name):
    """float64: every fixture code exactly, the stored decode values to 1e-12, the stored residual norms likewise."""
    x = latents(gold, codebooks, name).double()
    cb = codebooks.double()
    want = torch.from_numpy(gold[name + "_codes"].astype(np.int64))
    codes = rvq_encode_torch(cb, x)
    assert codes.dtype == torch.int64 and codes.shape == want.shape == (32,) + (x.shape[0], x.shape[2])
    assert torch.equal(codes, want)
    dec = rvq_decode_torch(cb, want, torch.float64)
    ii = gold[name + "_dec_idx"]
    assert float(np.abs(dec.numpy()[tuple(ii.T)] - gold[name + "_dec_val"]).max()) <= 1e-12
    assert float(np.abs((x - dec).norm(dim=1).numpy() - gold[name + "_resid_norm"]).max()) <= 1e-12
    # the first n rows of the 24 kbps codes are the codes at the bandwidth that has n stages
    for bw, n in BANDWIDTH_STAGES[:3]:
        assert torch.equal(rvq_encode_torch(cb, x, num_quantizers_for_bandwidth(bw, 1024, 32)), want[:n])


def test_lower_bandwidths_are_prefixes_in_the_library_too(gold, codebooks):
    tf = pytest.importorskip("transformers")
    from transformers.models.encodec.modeling_encodec import EncodecResidualVectorQuantizer
    q = EncodecResidualVectorQuantizer(tf.EncodecConfig(target_bandwidths=[1.5, 3.0, 6.0, 12.0, 24.0])).eval()
    q.load_state_dict(random_encodec_quantizer_state_dict(gold["meta"]["param_seed"]), strict=True)
    q = q.double()
    name = "gaussian_3x17"
    x = latents(gold, codebooks, name).double()
    want = torch.from_numpy(gold[name + "_codes"].astype(np.int64))
    with torch.no_grad():
        for bw, n in BANDWIDTH_STAGES:
            got = q.encode(x, bw)
            assert got.shape[0] == n and torch.equal(got, want[:n]), bw
        torch.testing.assert_close(q.decode(want[:8]), rvq_decode_torch(codebooks.double(), want[:8], torch.float64), rtol=0, atol=1e-12)


def test_refusals_come_before_any_launch():
    from v2a_amd import _lib
    _lib.build(verbose=False)
    q = EncodecQuantizer(random_encodec_quantizer_state_dict(1, num_quantizers=4), "cpu")
    with pytest.raises(ValueError, match=r"\(b, 128, t\)"):
        q.encode(torch.zeros(2, 64, 128))                           # channel axis is not the codebook dimension
    with pytest.raises(ValueError, match=r"\(b, t, 128\)"):
        q.encode(torch.zeros(2, 128, 64), channels_last=True)
    with pytest.raises(ValueError, match=r"\(b, 128, t\)"):
        q.encode(torch.zeros(128, 9))
    with pytest.raises(ValueError, match="float"):
        q.encode(torch.zeros(2, 128, 9, dtype=torch.int64))
    ok = torch.zeros(4, 2, 9, dtype=torch.int64)
    for bad in (-1, 1024):
        c = ok.clone()
        c[3, 1, 8] = bad
        with pytest.raises(ValueError, match=r"outside \[0, 1024\)"):
            q.decode(c)
    with pytest.raises(ValueError, match="5 stages"):
        q.decode(torch.zeros(5, 2, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer"):
        q.decode(torch.zeros(4, 2, 9))


def _small_model(**kw):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4,
                                          max_seq_len=256, if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=128, if_cond_proj_in=True, device="cpu", **kw)


class _Dim64(EncodecQuantizer):
    dim = 64


def test_integer_cond_without_a_quantizer_is_refused():
    import v2a_amd
    assert v2a_amd.EncodecQuantizer is EncodecQuantizer and "EncodecQuantizer" in v2a_amd.__all__
    m = _small_model()
    with pytest.raises(NotImplementedError, match="load_audio_quantizer"):
        m.sample(torch.zeros(2, 8, 12, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="load_audio_quantizer"):
        m.latents_to_codes(torch.zeros(2, 12, 128), 6.0)
    with pytest.raises(TypeError):
        m.load_audio_quantizer("facebook/encodec_24khz")
    with pytest.raises(ValueError, match="128 latent channels"):
        m.load_audio_quantizer(_Dim64.__new__(_Dim64))                # a quantizer of another width than the model's latents


def test_cli_codes_flag():
    from v2a_amd import cli
    p = cli.build_parser()
    base = ["ck", "0", "scp", "0", "1", "out"]
    assert p.parse_args(base).codes is None
    for bw in (1.5, 3, 6, 12, 24):
        assert p.parse_args(base + ["--encodec", "e.pt", "--codes", str(bw)]).codes == float(bw)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--encodec", "e.pt", "--codes", "5"])   # not a bandwidth of the codec
    with pytest.raises(SystemExit):
        cli.main(base + ["--codes", "6"])                            # needs --encodec
