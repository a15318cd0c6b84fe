"""GPU: the note extraction kernel (csrc/midi_notes.hip: v2a_roll_notes) through `v2a_amd.midi.roll_to_notes`, and what is built on
it (`E2TTS.midi_to_notes`, `E2TTS.frames_to_notes`).

Everything here is integer work, so every comparison is exact: `onset`, `counts`, `totals` and `notes` equal the numpy restatement of
tests/test_midi_notes_host.py (np.diff on the zero-prefixed roll), which that file holds to the reference's own `process_midi` /
`process_roll` / `GetNote` on the fixture.  Shapes: T at the ballot-word (64) and tile (256) boundaries and the two clip lengths of
the piano configurations (750, 2250), keys 51 / 88 / 128, three clips with ragged lengths (zero and full among them), bytes and fp32
with a threshold, a (b, K, t) view read in place, the worst-case alternating roll, notes across word and tile boundaries, a buffer
smaller than the notes."""
import numpy as np
import pytest
import torch

from test_midi_notes_host import load_cases, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256


@pytest.fixture(scope="module")
def L():
    from v2a_amd import _lib
    _lib.lib()
    assert _lib.ROLL_NOTES_TILE == TILE
    return _lib


def seeded_roll(b, t, keys, seed):
    """Held notes of 1..40 frames with gaps of 1..30, one key on throughout, one alternating every frame, one held across every
    multiple of 64 (so notes cross the word and tile boundaries), one empty."""
    rng = np.random.default_rng(seed)
    roll = np.zeros((b, t, keys), np.uint8)
    for i in range(b):
        for k in range(keys):
            f = int(rng.integers(0, 8))
            while f < t:
                d = int(rng.integers(1, 41))
                roll[i, f:f + d, k] = 1
                f += d + int(rng.integers(1, 31))
        roll[i, :, 1] = 1
        roll[i, :, 2] = 0
        roll[i, i % 2::2, 2] = 1
        roll[i, :, 3] = 0
        for edge in range(64, t + 1, 64):
            roll[i, max(0, edge - 2 - i):edge + 1 + i, 3] = 1                     # on at edge - 1 and at edge
        roll[i, :, 4] = 0
    return roll


def raw_launch(L, roll, lens=None, threshold=0.0, cap=None, onset=True):
    """One v2a_roll_notes launch on a device tensor -> (counts, totals, notes buffer, onset) as numpy, the buffer pre-filled with -7."""
    b, t, keys = roll.shape
    cap = keys * ((t + 1) // 2) if cap is None else cap
    counts = torch.full((b, keys), -7, dtype=torch.int32, device=DEV)
    totals = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    notes = torch.full((b, max(cap, 1), 3), -7, dtype=torch.int32, device=DEV)
    on = torch.full((b, keys, t), -7, dtype=torch.int8, device=DEV) if onset else None
    ln = None if lens is None else torch.as_tensor(lens, dtype=torch.int32).to(DEV)
    L.roll_notes(roll, counts, totals, notes if cap else None, strides=roll.stride(), B=b, T=t, keys=keys, cap=cap, threshold=threshold, lens=ln, onset=on)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), totals.cpu().numpy(), notes.cpu().numpy()[:, :cap], None if on is None else on.cpu().numpy()


def check_against_restatement(roll_np, got, lens=None, cap=None):
    counts, totals, notes, onset = got
    for i in range(len(roll_np)):
        o, c, n = restate(roll_np[i], None if lens is None else lens[i])
        assert np.array_equal(counts[i], c), i
        assert totals[i] == len(n), i
        if onset is not None:
            assert np.array_equal(onset[i], o), i
        kept = len(n) if cap is None else min(len(n), cap)
        assert np.array_equal(notes[i, :kept], n[:kept]), i
        assert (notes[i, kept:] == -7).all(), i                                   # rows behind the notes are not written


@pytest.mark.parametrize("keys", [51, 88, 128])
@pytest.mark.parametrize("t", [1, 63, 64, 65, 255, 256, 257, 750, 2250])
def test_bytes_with_ragged_lengths(L, t, keys):
    """B = 3, lens = (full, zero, ragged); then the same clips without lens."""
    roll = seeded_roll(3, t, keys, 100 * t + keys)
    lens = [t, 0, max(1, (2 * t) // 3)]
    dev = torch.from_numpy(roll).to(DEV)
    check_against_restatement(roll, raw_launch(L, dev, lens), lens)
    check_against_restatement(roll, raw_launch(L, dev))
    if t in (64, 257):                                                            # lengths at a word edge and one past a tile
        lens = [min(t, 64), min(t, 256), t - 1]
        check_against_restatement(roll, raw_launch(L, dev, lens), lens)


@pytest.mark.parametrize("keys,t", [(51, 257), (88, 750), (128, 65)])
def test_fp32_with_threshold_and_strided_view(L, keys, t):
    """fp32 on iff > threshold (values exactly at the threshold and NaN are off), and a (b, K, t) tensor read through its transposed
    view -- both element sizes."""
    g = torch.Generator().manual_seed(keys + t)
    p = torch.rand(3, t, keys, generator=g)
    p[0, :, 0] = 0.4                                                              # exactly the threshold: off under >, on under >=
    p[1, ::3, 1] = float("nan")
    lens = [t, t // 2, t]
    want = (p > 0.4).numpy().astype(np.uint8)
    check_against_restatement(want, raw_launch(L, p.to(DEV), lens, threshold=0.4), lens)
    from v2a_amd.midi import ROLL_THRESHOLD_BELOW
    want_ge = (p >= np.float32(0.4)).numpy().astype(np.uint8)
    assert want_ge[0, :, 0].all() and not want[0, :, 0].any()
    check_against_restatement(want_ge, raw_launch(L, p.to(DEV), lens, threshold=ROLL_THRESHOLD_BELOW), lens)
    # (b, K, t) storage, read in place
    kt = p.transpose(1, 2).contiguous().to(DEV)
    view = kt.transpose(1, 2)
    assert view.shape == (3, t, keys) and view.stride() == (keys * t, 1, t)
    check_against_restatement(want, raw_launch(L, view, lens, threshold=0.4), lens)
    bytes_kt = torch.from_numpy(want).transpose(1, 2).contiguous().to(DEV)
    check_against_restatement(want, raw_launch(L, bytes_kt.transpose(1, 2), lens), lens)
    # a batch slice of a larger tensor: the batch stride is not t * keys
    big = torch.from_numpy(np.concatenate([want, want[::-1]], axis=1)).to(DEV)      # (3, 2 t, keys)
    check_against_restatement(want, raw_launch(L, big[:, :t]))


@pytest.mark.parametrize("keys,t", [(128, 257), (88, 64), (51, 1)])
def test_worst_case_alternating_roll_and_a_small_buffer(L, keys, t):
    """Every key alternating from frame 0: keys * ceil(t / 2) notes, the default buffer exactly full.  Then a buffer of fewer rows:
    the first `cap` rows are written, nothing behind them, totals still holds the true count, the call returns 0 and the host
    wrapper raises."""
    from v2a_amd import midi
    roll = np.zeros((2, t, keys), np.uint8)
    roll[0, 0::2] = 1
    roll[1, 1::2] = 1
    dev = torch.from_numpy(roll).to(DEV)
    got = raw_launch(L, dev)
    assert got[1][0] == keys * ((t + 1) // 2) == midi.worst_case_rows(t, keys) and got[1][1] == keys * (t // 2)
    check_against_restatement(roll, got)
    for cap in (0, 1, keys * ((t + 1) // 2) - 1):
        got = raw_launch(L, dev, cap=cap, onset=False)
        check_against_restatement(roll, got, cap=cap)
        with pytest.raises(L.V2AError, match="notes, the buffer"):
            midi.roll_to_notes(dev, cap=cap)
    assert len(midi.roll_to_notes(dev)[0]) == midi.worst_case_rows(t, keys)


def test_roll_to_notes_rows_pitches_and_batch_independence(L):
    """The wrapper's rows (pitch = 21 + note_min + key), its onset matrix, and a clip alone against the same clip in a batch."""
    from v2a_amd import midi
    t, keys = 750, 51
    roll = seeded_roll(3, t, keys, 7)
    lens = [t, 333, 0]
    dev = torch.from_numpy(roll).to(DEV)
    notes, onset = midi.roll_to_notes(dev, lens, note_min=15, return_onset=True)
    assert len(notes) == 3 and onset.shape == (3, keys, t) and onset.dtype == np.int8
    for i in range(3):
        o, c, n = restate(roll[i], lens[i])
        assert notes[i].dtype == np.int32 and np.array_equal(notes[i], n + np.array([36, 0, 0], np.int32))
        assert np.array_equal(onset[i], o)
        alone = midi.roll_to_notes(dev[i:i + 1], lens[i:i + 1], note_min=15)
        assert len(alone) == 1 and np.array_equal(alone[0], notes[i])
        swapped = midi.roll_to_notes(dev.flip(0), lens[::-1], note_min=15)
        assert np.array_equal(swapped[2 - i], notes[i])
    assert len(notes[2]) == 0 and notes[2].shape == (0, 3)
    # a host roll is taken to the device; bool elements are bytes
    host = midi.roll_to_notes(torch.from_numpy(roll).bool(), lens, note_min=15, device=DEV)
    assert all(np.array_equal(a, b) for a, b in zip(host, notes))
    back = midi.notes_to_roll(notes[1], t, 0.04, note_min=15, keys=keys)
    assert np.array_equal(back[:333], roll[1, :333]) and not back[333:].any()


@pytest.fixture(scope="module")
def fixture_cases():
    return load_cases()[1]


def test_fixture_cases(L, fixture_cases):
    """The reference's own onsets and notes: the clip as it is (the kernel's end at T is the reference's appended end), and the
    reference's roll -- placed at its keys of 88, padded to whole 50-frame windows -- whose onset matrix is compared in full."""
    from v2a_amd import midi
    for tag, c in sorted(fixture_cases.items()):
        roll, nm, keys = c["roll"], c["note_min"], c["keys"]
        t, tp = len(roll), c["onset"].shape[1]
        notes, onset = midi.roll_to_notes(torch.from_numpy(roll[None]).to(DEV), note_min=nm, return_onset=True)
        assert np.array_equal(notes[0], c["notes"]), tag
        assert np.array_equal(onset[0][:, :t], c["onset"][nm:nm + keys, :t]), tag
        full = np.zeros((tp, 88), np.uint8)
        full[:t, nm:nm + keys] = roll
        notes, onset = midi.roll_to_notes(torch.from_numpy(full[None]).to(DEV), return_onset=True)
        assert np.array_equal(notes[0], c["notes"]) and np.array_equal(onset[0], c["onset"]), tag
        counts = raw_launch(L, torch.from_numpy(full[None]).to(DEV))[0]
        assert np.array_equal(counts[0], c["counts"]), tag


# ---- E2TTS ---------------------------------------------------------------------------------------------------------------------------
V2R_SEED, R2M_SEED = 3, 3


@pytest.fixture(scope="module", params=[51, 88])
def piano_model(request):
    import v2a_amd
    from v2a_amd.synth import random_roll2midi_state_dict, random_video2roll_state_dict
    keys = request.param
    m = v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                       if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                      num_channels=16, if_cond_proj_in=False, compute_dtype="fp32", frames_compute_dtype="fp32", device=DEV, piano_keys=keys)
    vsd = random_video2roll_state_dict(V2R_SEED) if keys == 51 else random_video2roll_state_dict(V2R_SEED, 88)
    m.load_state_dict({"video2roll_net." + k: v for k, v in vsd.items()}, strict=False)
    m.load_roll2midi({"state_dict_G": random_roll2midi_state_dict(R2M_SEED)})
    return m


def test_frames_to_notes_of_both_sources(piano_model):
    from v2a_amd import midi
    from v2a_amd.synth import synthetic_piano_frames
    m = piano_model
    keys = m.piano.notes
    x = synthetic_piano_frames(2, 7, seed=9)
    lens = [7, 5]
    # source="midi": the kernel on frames_to_midi's own output
    probs, roll = m.frames_to_midi(x)
    assert roll.shape == (2, 7, 51) and roll.dtype == torch.uint8 and roll.is_cuda
    got = m.frames_to_notes(x, source="midi", lens=lens)
    want = midi.roll_to_notes(roll, lens, note_min=15)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(m.midi_to_notes(roll, lens), want))
    for i in range(2):
        assert np.array_equal(want[i], restate(roll[i].cpu().numpy(), lens[i])[2] + np.array([36, 0, 0], np.int32))
    # source="roll": the Video2Roll probabilities >= 0.4 over the model's own keys
    fp = m._video2roll().frame_probs(x)
    assert fp.shape == (2, 7, keys)
    on = (fp.cpu().numpy() >= np.float32(0.4)).astype(np.uint8)
    got = m.frames_to_notes(x, source="roll", lens=lens)
    n_on = 0
    for i in range(2):
        want_i = restate(on[i], lens[i])[2] + np.array([21 + m.piano.note_min, 0, 0], np.int32)
        assert np.array_equal(got[i], want_i)
        n_on += len(want_i)
    print(f"piano_keys={keys}: source=midi {sum(map(len, want))} notes, source=roll {n_on} notes over 2 clips x 7 frames; spf {m.piano_spf:.5f}")
    assert (m.piano.note_min, m.piano_spf) == ((15, 0.04) if keys == 51 else (0, 2.5 * 320 / 24000))
