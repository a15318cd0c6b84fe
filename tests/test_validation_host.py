"""CPU: the host side of `E2TTS.forward(val=True)`, the reference's validation pass (x3:2307-2588, `x3` =
src/e2_tts_pytorch/e2_tts_crossatt3.py): the fixed span, the refusals, the return type, the MIDI ground-truth loader, and the
argument checks of the three C-ABI entry points behind it."""
import inspect

import numpy as np
import pytest
import torch

import v2a_amd
from v2a_amd import cli

SMALL = dict(dim=128, dim_text=192, dim_frames=64, depth=4, heads=2, frames_heads=1, num_registers=4, max_seq_len=256)
B, N, LENS, TIMES = 3, 40, [40, 33, 21], [0.1, 0.37, 0.8]          # shared with tests/test_validation_gpu.py


def _model(**kw):
    return v2a_amd.E2TTS(transformer=dict(if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True, **SMALL),
                         num_channels=16, **kw)


def _reference_span(seq_len, frac_lengths, max_length):
    """x3:307-337 with val=True, op for op in plain torch (einx comparisons written as broadcasts), and `&= mask` of x3:2361-2362."""
    lengths = (frac_lengths * seq_len).long()
    max_start = seq_len - lengths
    rand = torch.tensor([0.5] * frac_lengths.shape[0]).float()
    start = (max_start * rand).long().clamp(min=0)
    end = start + lengths
    seq = torch.arange(seq_len.max().item()).long()
    out = (seq[None, :] >= start[:, None]) & (seq[None, :] < end[:, None])
    out = torch.nn.functional.pad(out, (0, max_length - out.shape[-1]), value=False)
    return out & (torch.arange(max_length)[None, :] < seq_len[:, None])


def test_val_span_mask_is_85_percent_centred():
    lens = torch.tensor(LENS)
    span = v2a_amd.val_span_mask(lens, N)
    assert span.shape == (B, N) and span.dtype == torch.bool
    for row, (lo, hi) in zip(span, ((3, 37), (2, 30), (2, 19))):       # float32 0.85 * 40, 33, 21 -> 34, 28, 17 frames
        want = torch.zeros(N, dtype=torch.bool)
        want[lo:hi] = True
        assert torch.equal(row, want), (lo, hi, row.nonzero().flatten().tolist())
    frac = torch.tensor([(0.7 + 1.0) / 2.0] * B).float()
    assert torch.equal(span, _reference_span(lens, frac, N))
    for lens in ([1, 2, 3], [7, 40, 39], [0, 5, 6]):                     # short clips, and an empty one: its span is empty
        lens = torch.tensor(lens)
        assert torch.equal(v2a_amd.val_span_mask(lens, N), _reference_span(lens, torch.tensor([0.85] * 3).float(), N))
    assert not v2a_amd.val_span_mask(torch.tensor([0, 5, 6]), N)[0].any()


def test_forward_exists_with_the_reference_signature():
    sig = inspect.signature(v2a_amd.E2TTS.forward)
    names = list(sig.parameters)
    assert names[:2] == ["self", "inp"]
    for k in ("text", "times", "lens", "velocity_consistency_model", "prompt", "video_drop_prompt", "audio_drop_prompt", "val",
              "video_paths", "frames", "midis", "x0", "text_embed", "context", "context_mask", "frames_embed"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig.parameters["val"].default is False and sig.parameters["times"].default is None


def test_return_types_carry_the_reference_field_names():
    assert v2a_amd.E2TTSReturn._fields == ("loss", "cond", "pred_flow", "pred_data", "loss_breakdown")          # x3:134
    assert v2a_amd.E2TTSReturn.__name__ == "E2TTS"
    assert v2a_amd.LossBreakdown._fields == ("flow", "velocity_consistency", "a", "b")                           # x3:132
    assert v2a_amd.LossBreakdown.__name__ == "LossBreakdown"


def test_refusals_come_before_any_gpu_work():
    x = torch.zeros(B, N, 16)
    m = _model(if_cond_proj_in=False, audiocond_drop_prob=1.1)
    with pytest.raises(NotImplementedError, match="val=False"):
        m.forward(x, text=torch.zeros(B, N, 192))
    with pytest.raises(NotImplementedError, match="val=False"):
        m(x, text=torch.zeros(B, N, 192), val=False)
    with pytest.raises(NotImplementedError, match="velocity_consistency_model"):
        m.forward(x, val=True, velocity_consistency_model=m)
    snr = _model(if_cond_proj_in=True, audiocond_drop_prob=0.3, audiocond_snr=(5.0, 10.0))
    with pytest.raises(NotImplementedError, match="audiocond_snr"):
        snr.forward(x, val=True, text=torch.zeros(B, N, 192))
    with pytest.raises(NotImplementedError, match="concat_cond"):
        _model(concat_cond=True)


def test_load_midi_ground_truth_pads_and_cuts(tmp_path):
    g = np.random.default_rng(3)
    vids = [str(tmp_path / f"p{i}.mp4") for i in range(3)]
    rolls = [g.random((25, 88)), g.random((40, 88)), g.random((61, 88))]
    for v, r in zip(vids, rolls):
        np.save(v.replace(".mp4", ".3.npy"), r)                         # float64 on disk, as a MIDI export leaves it
    got = v2a_amd.load_midi_ground_truth([vids[0], None, (vids[1], 0, 12000), vids[2]], 40)
    assert got.shape == (3, 40, v2a_amd.NOTES) and got.dtype == torch.float32
    assert torch.equal(got[0, :25], torch.from_numpy(rolls[0].astype(np.float32))[:, 15:66]) and float(got[0, 25:].abs().max()) == 0
    assert torch.equal(got[1], torch.from_numpy(rolls[1].astype(np.float32))[:, 15:66])
    assert torch.equal(got[2], torch.from_numpy(rolls[2].astype(np.float32))[:40, 15:66])
    assert v2a_amd.load_midi_ground_truth([None, None], 40) is None
    with pytest.raises(FileNotFoundError):
        v2a_amd.load_midi_ground_truth([str(tmp_path / "missing.mp4")], 40)


def test_entry_points_validate_arguments_on_cpu():
    from v2a_amd import _lib
    L = _lib.lib()
    for name in ("v2a_cfm_interp", "v2a_masked_sqerr", "v2a_roll_metrics"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.v2a_cfm_interp(None, 16, 16, None, 16, 16, None, 1, 1, 16, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_cfm_interp(16, 16, 16, None, 16, 16, None, 1, 1, 6, None) == -1 and b"multiple of 4" in L.v2a_last_error()
    assert L.v2a_cfm_interp(16, 24, 16, None, 16, 16, None, 1, 1, 16, None) == -1 and b"alignment" in L.v2a_last_error()
    assert L.v2a_masked_sqerr(16, 16, 16, 1, 1, 16, None, 16, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_masked_sqerr(16, 16, 16, 0, 1, 16, 16, 16, None) == -1 and b"B=0" in L.v2a_last_error()
    assert L.v2a_roll_metrics(16, 16, None, 1, 1, 51, 16, 16, None) == -1 and b"null" in L.v2a_last_error()
    assert L.v2a_roll_metrics(16, 16, 16, 1, 1, 51, 16, 12, None) == -1 and b"alignment" in L.v2a_last_error()
    assert _lib.LOSS_MAX_PARTS == 256
    assert L.v2a_abi_version() == 9                                       # additive exports


def test_cli_has_validate():
    a = cli.build_parser().parse_args(["ck.pt", "0", "list.scp", "0", "3", "out", "--validate", "--piano"])
    assert a.validate and a.piano
    assert cli.build_parser().parse_args(["ck.pt", "0", "list.scp", "0", "3", "out"]).validate is False
