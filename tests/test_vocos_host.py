"""CPU: host side of the Vocos vocoder (v2a_amd.Vocos, csrc/vocos.hip) -- shape inference, every refusal of the class, from_pretrained on a
local directory, E2TTS.load_vocoder, the host tables, the header and binding of the new entry points and their argument checks, which
answer V2A_ERR_ARG before any HIP call."""
import os
import re

import pytest
import torch

import vocos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("v2a_vocos_stage_in", "v2a_vocos_dwconv_ln", "v2a_vocos_gelu", "v2a_vocos_scale_residual", "v2a_vocos_spectrum", "v2a_vocos_overlap_add")


@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _sd(C=10, dim=64, hidden=192, depth=2, n_fft=64, seed=0):
    return R.VocosRef(C, dim, hidden, depth, n_fft, n_fft // 4, seed=seed).state_dict()


def test_header_declares_the_entries_with_the_lines_they_replace():
    from v2a_amd import _lib
    h = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    for name in ENTRIES:
        assert re.search(r"int %s\(" % name, h) and name in _lib.EXPORTS, name
    assert "e2_tts_crossatt.py:1324" in h and "x3:2275-2287" in h and h.count("Replaces:") >= 6
    assert _lib.ABI_VERSION == 9
    from v2a_amd import vocos
    assert "#define V2A_VOCOS_MAX_DIM %d" % vocos.MAX_DIM in h and "#define V2A_VOCOS_MAX_FFT %d" % vocos.MAX_FFT in h


def test_shapes_are_read_from_the_state_dict():
    from v2a_amd import Vocos
    v = Vocos(_sd(), device="cpu")
    assert (v.C, v.dim, v.hidden, v.depth, v.n_fft, v.hop) == (10, 64, 192, 2, 64, 16)
    assert (v.c_pad, v.n_logits, v.k_spec, v.n_bins) == (16, 68, 80, 33)
    v = Vocos(_sd(20, 96, 160, 3, 128), device="cpu", hop_length=24)
    assert (v.C, v.dim, v.hidden, v.depth, v.n_fft, v.hop) == (20, 96, 160, 3, 128, 24)
    sd = _sd()
    sd["feature_extractor.mel_spec.spectrogram.window"] = torch.zeros(64)           # ignored
    assert Vocos(sd, device="cpu").depth == 2
    with pytest.raises(TypeError):
        Vocos([1, 2])


def test_host_tables():
    from v2a_amd import Vocos, istft_basis
    v = Vocos(_sd(), device="cpu")
    basis, wsq = v.host_tables()
    assert basis.shape == (64, 80) and basis.dtype == torch.float32 and wsq.shape == (64,) and wsq.dtype == torch.float32
    assert torch.equal(basis[:, :66], istft_basis(64).float()) and bool((basis[:, 66:] == 0).all())
    assert torch.equal(wsq, torch.hann_window(64, periodic=True, dtype=torch.float64).pow(2).float())


def test_constructor_refusals():
    from v2a_amd import Vocos
    sd = _sd()
    sd["backbone.convnext.0.norm.scale.weight"] = torch.zeros(4, 64)
    with pytest.raises(NotImplementedError, match="adaptive-norm"):
        Vocos(sd, device="cpu")
    for key in ("backbone.embed.weight", "head.out.weight", "backbone.convnext.0.pwconv1.weight", "backbone.convnext.1.gamma", "backbone.norm.bias",
                "backbone.final_layer_norm.weight", "head.out.bias", "backbone.convnext.1.dwconv.weight"):
        sd = _sd()
        del sd[key]
        with pytest.raises(ValueError, match=re.escape(key)):
            Vocos(sd, device="cpu")
    for key, shape in (("backbone.convnext.1.pwconv2.weight", (64, 191)), ("backbone.embed.bias", (63,)), ("backbone.convnext.0.dwconv.weight", (64, 1, 5)),
                       ("head.out.bias", (64,)), ("backbone.embed.weight", (64, 10, 5)), ("head.out.weight", (66,))):
        sd = _sd()
        sd[key] = torch.zeros(shape)
        with pytest.raises(ValueError, match=re.escape(key)):
            Vocos(sd, device="cpu")
    with pytest.raises(ValueError, match="multiples of 16"):
        Vocos(_sd(dim=72), device="cpu")
    with pytest.raises(ValueError, match="multiples of 16"):
        Vocos(_sd(hidden=200), device="cpu")
    with pytest.raises(ValueError, match="n_fft"):
        Vocos(_sd(n_fft=62), device="cpu")
    for hop in (0, -4, 65):
        with pytest.raises(ValueError, match="hop_length"):
            Vocos(_sd(), device="cpu", hop_length=hop)
    with pytest.raises(ValueError, match="envelope"):                              # hop = n_fft: the Hann window is zero where two frames meet
        Vocos(_sd(), device="cpu", hop_length=64)
    Vocos(_sd(), device="cpu", hop_length=63)                                       # torch.istft accepts it as well
    S = torch.randn(1, 33, 4, dtype=torch.complex128)
    torch.istft(S, 64, 63, 64, torch.hann_window(64, periodic=True, dtype=torch.float64), center=True)


def test_from_pretrained_reads_a_local_directory(tmp_path):
    import yaml
    from v2a_amd import Vocos
    sd = _sd()
    cfg = dict(feature_extractor=dict(class_path="vocos.feature_extractors.MelSpectrogramFeatures",
                                      init_args=dict(sample_rate=24000, n_fft=64, hop_length=32, n_mels=10, padding="center")),
               backbone=dict(class_path="vocos.models.VocosBackbone", init_args=dict(input_channels=10, dim=64, intermediate_dim=192, num_layers=2)),
               head=dict(class_path="vocos.heads.ISTFTHead", init_args=dict(dim=64, n_fft=64, hop_length=32, padding="center")))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / "pytorch_model.bin")
    v = Vocos.from_pretrained(tmp_path, device="cpu")
    assert (v.C, v.dim, v.hidden, v.depth, v.n_fft, v.hop) == (10, 64, 192, 2, 64, 32)
    assert Vocos.from_pretrained(str(tmp_path), device="cpu").hop == 32
    cfg["head"]["init_args"]["padding"] = "same"
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(NotImplementedError, match="padding"):
        Vocos.from_pretrained(tmp_path, device="cpu")
    cfg["head"]["init_args"].update(padding="center", n_fft=128)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="n_fft"):
        Vocos.from_pretrained(tmp_path, device="cpu")
    for missing in ("charactr/vocos-mel-24khz", str(tmp_path / "nothing")):         # a hub name is not a local directory: nothing is fetched
        with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
            Vocos.from_pretrained(missing, device="cpu")


def test_load_vocoder_type_and_shape_errors(tmp_path):
    import v2a_amd
    from v2a_amd import MelSpec, Vocos
    tk = dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=64, if_text_modules=True,
              if_cross_attn=True, if_audio_conv=True, if_text_conv=True)
    m = v2a_amd.E2TTS(transformer=tk, num_channels=10, sampling_rate=24000, device="cpu")
    assert m.vocos is None
    v = Vocos(_sd(), device="cpu")
    assert m.load_vocoder(v) is v and m.vocos is v
    assert isinstance(m.load_vocoder(_sd()), Vocos) and m.vocos.hop == 16
    assert m.load_vocoder(_sd(), hop_length=32).hop == 32
    with pytest.raises(TypeError, match="load_vocoder"):
        m.load_vocoder(3)
    with pytest.raises(TypeError, match="keywords"):
        m.load_vocoder(v, hop_length=16)
    with pytest.raises(FileNotFoundError):
        m.load_vocoder(str(tmp_path / "nothing"))
    with pytest.raises(ValueError, match="num_channels=10"):
        m.load_vocoder(_sd(C=12))
    assert m.vocos.hop == 32                                                       # a refused vocoder leaves the loaded one
    m.load_mel_spec(MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=10, device="cpu"))
    assert m.load_vocoder(_sd()).hop == 16
    with pytest.raises(ValueError, match="hop"):
        m.load_vocoder(_sd(), hop_length=32)
    m2 = v2a_amd.E2TTS(transformer=tk, num_channels=10, device="cpu")                # no sampling_rate: no rate to contradict
    m2.load_mel_spec(MelSpec(filter_length=64, hop_length=16, win_length=64, n_mel_channels=10, device="cpu"))
    assert m2.load_vocoder(_sd(), hop_length=32).hop == 32


def test_decode_refuses_shapes_before_any_launch():
    from v2a_amd import Vocos
    v = Vocos(_sd(), device="cpu")
    for bad, match in ((torch.zeros(1, 10, 1), "at least 2 frames"), (torch.zeros(1, 9, 5), "features are"), (torch.zeros(1, 1, 10, 5), "features are"),
                       (torch.zeros(10), "features are"), (torch.zeros(1, 10, 5, dtype=torch.int64), "floating point")):
        with pytest.raises(ValueError, match=match):
            v.decode(bad)
    for lens in ((1,), (6,), (2, 2)):
        with pytest.raises(ValueError, match="lens"):
            v.decode(torch.zeros(1, 10, 5), lens=lens)


def test_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    A = 4096                                                                       # an aligned, non-null address: nothing is read before the checks pass
    ok_stage = dict(x=A, xbs=50, xcs=5, B=1, C=10, T=5, lens=None, out=2 * A, c_pad=16)
    stage = lambda **k: lib.v2a_vocos_stage_in(*[{**ok_stage, **k}[n] for n in ("x", "xbs", "xcs", "B", "C", "T", "lens", "out", "c_pad")], None)
    for k, word in ((dict(x=None), b"null"), (dict(out=A), b"aliased"), (dict(c_pad=12), b"c_pad"), (dict(c_pad=8), b"c_pad"), (dict(T=0), b"T=0"),
                    (dict(B=0), b"B=0"), (dict(B=70000), b"B=70000"), (dict(xcs=4), b"x_chan_stride"), (dict(xbs=49), b"x_batch_stride"),
                    (dict(out=2 * A + 4), b"alignment"), (dict(lens=2), b"alignment")):
        assert stage(**k) == -1 and word in lib.v2a_last_error(), k
    ok_dw = dict(x=A, ldx=64, wt=2 * A, bias=3 * A, gamma=4 * A, beta=5 * A, eps=1e-6, B=1, T=5, rpc=11, d=64, lens=None, y=6 * A, ldy=64)
    dw = lambda **k: lib.v2a_vocos_dwconv_ln(*[{**ok_dw, **k}[n] for n in ("x", "ldx", "wt", "bias", "gamma", "beta", "eps", "B", "T", "rpc", "d", "lens", "y",
                                                                               "ldy")], None)
    for k, word in ((dict(wt=None), b"null"), (dict(y=A), b"aliased"), (dict(d=72), b"d=72"), (dict(d=8), b"d=8"), (dict(d=2064), b"d=2064"),
                    (dict(rpc=4), b"rows_per_clip"), (dict(ldx=60), b"ldx"), (dict(ldy=66), b"ldy"), (dict(eps=0.0), b"eps"), (dict(T=0), b"T=0"),
                    (dict(bias=3 * A + 4), b"alignment")):
        assert dw(**k) == -1 and word in lib.v2a_last_error(), k
    assert lib.v2a_vocos_gelu(None, 64, 4, 64, None) == -1 and b"null" in lib.v2a_last_error()
    for args, word in (((A, 64, 0, 64), b"rows=0"), ((A, 64, 4, 66), b"n=66"), ((A, 60, 4, 64), b"ldx"), ((A + 4, 64, 4, 64), b"alignment")):
        assert lib.v2a_vocos_gelu(*args, None) == -1 and word in lib.v2a_last_error(), args
    ok_sr = dict(p=A, ldp=64, gamma=2 * A, resid=3 * A, ldr=64, out=4 * A, ldo=64, rows=4, n=64)
    sr = lambda **k: lib.v2a_vocos_scale_residual(*[{**ok_sr, **k}[n] for n in ("p", "ldp", "gamma", "resid", "ldr", "out", "ldo", "rows", "n")], None)
    for k, word in ((dict(gamma=None), b"null"), (dict(out=A), b"aliased"), (dict(n=6), b"n=6"), (dict(ldr=32), b"ldr"), (dict(rows=0), b"rows=0"),
                    (dict(resid=3 * A + 8), b"alignment")):
        assert sr(**k) == -1 and word in lib.v2a_last_error(), k
    ok_sp = dict(logits=A, ldl=68, rows=4, n_fft=64, spec=2 * A, lds=80)
    sp = lambda **k: lib.v2a_vocos_spectrum(*[{**ok_sp, **k}[n] for n in ("logits", "ldl", "rows", "n_fft", "spec", "lds")], None)
    for k, word in ((dict(spec=None), b"null"), (dict(spec=A), b"aliased"), (dict(n_fft=62), b"n_fft=62"), (dict(n_fft=8192), b"n_fft=8192"),
                    (dict(ldl=65), b"ld_logits"), (dict(lds=64), b"ld_spec"), (dict(lds=81), b"ld_spec"), (dict(rows=0), b"rows=0"),
                    (dict(spec=2 * A + 4), b"alignment")):
        assert sp(**k) == -1 and word in lib.v2a_last_error(), k
    ok_oa = dict(frames=A, ldf=64, rpc=11, wsq=2 * A, B=1, T=5, n_fft=64, hop=16, lens=None, out=3 * A, obs=64)
    oa = lambda **k: lib.v2a_vocos_overlap_add(*[{**ok_oa, **k}[n] for n in ("frames", "ldf", "rpc", "wsq", "B", "T", "n_fft", "hop", "lens", "out", "obs")],
                                               None)
    for k, word in ((dict(wsq=None), b"null"), (dict(out=A), b"aliased"), (dict(T=1), b"T=1"), (dict(hop=0), b"hop=0"), (dict(hop=65), b"hop=65"),
                    (dict(n_fft=66), b"n_fft=66"), (dict(ldf=60), b"ld_frames"), (dict(rpc=4), b"rows_per_clip"), (dict(obs=63), b"out_batch_stride"),
                    (dict(out=3 * A + 2), b"alignment")):
        assert oa(**k) == -1 and word in lib.v2a_last_error(), k


def test_cli_takes_vocos_or_encodec_as_the_vocoder(capsys):
    from v2a_amd import cli
    args = ["ckpt", "0", "scp", "0", "1", "out"]
    a = cli.build_parser().parse_args(args + ["--vocos", "dir"])
    assert a.vocos == "dir" and a.encodec is None
    assert cli.build_parser().parse_args(args).vocos is None
    with pytest.raises(SystemExit):
        cli.main(args + ["--vocos", "dir", "--encodec", "state.pt"])
    assert "exclusive" in capsys.readouterr().err
