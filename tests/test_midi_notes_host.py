"""CPU: the host side of the note extraction behind Roll2Midi (v2a_amd.midi, csrc/midi_notes.hip; src/audeo/Midi_synth.py:33-148).

  * `restate`, the vectorised numpy restatement the GPU tests hold the kernel to (np.diff on the zero-prefixed roll), against the
    fixture tests/golden/midi_notes.npz -- onsets and notes produced by the REFERENCE'S OWN `process_midi` / `process_roll` / `GetNote`
    (scripts/make_golden_midi_notes.py), both branches, every case: exact;
  * header, ctypes signature and EXPORTS agree; the ABI version stays 9; bad arguments are refused before any HIP call;
  * `write_midi` -> `read_midi`: every note back, times within half a tick = 0.5 * 60 / (220 * 80) s = 1.70 ms;
  * roll -> notes -> file -> notes -> `notes_to_roll` gives the binarised roll back exactly, at both frame durations (0.04 s and 1/30 s);
  * `read_midi` on a hand-written byte string with running status, a tempo change and a velocity-0 note-off;
  * CLI argument rules of --midi-file; `E2TTS.piano_spf` under both piano configurations."""
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "midi_notes.npz")
HALF_TICK = 0.5 * 60.0 / (220 * 80)          # seconds


def restate(roll, lens=None):
    """roll (t, keys) of 0 / 1 -> (onset (keys, t) int8, counts (keys) int32, notes (n, 3) int32 rows (key, start, end) by key, then
    start).  Frames at or beyond `lens` are off; the diff of the roll between a zero frame in front and one behind gives +1 where a
    key comes on and -1 where it goes off, the one at frame `t` being the end of a key that still sounds."""
    on = (np.asarray(roll) != 0).astype(np.int8)
    t, keys = on.shape
    if lens is not None:
        on[int(lens):] = 0
    d = np.diff(np.concatenate([np.zeros((1, keys), np.int8), on, np.zeros((1, keys), np.int8)]), axis=0)     # (t + 1, keys)
    rows, counts = [], np.zeros(keys, np.int32)
    for k in range(keys):
        start, end = np.flatnonzero(d[:, k] == 1), np.flatnonzero(d[:, k] == -1)
        assert len(start) == len(end)
        counts[k] = len(start)
        rows += [(k, s, e) for s, e in zip(start, end)]
    return d[:t].T.copy(), counts, np.asarray(rows, np.int32).reshape(-1, 3)


def load_cases():
    """{tag: dict(roll (t, keys) uint8, keys, note_min, onset (88, T'), notes (n, 3) by pitch, counts (88))} of the fixture."""
    z = np.load(GOLD, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    out = {}
    for tag, c in meta["cases"].items():
        keys = c["keys"]
        roll = np.unpackbits(z[tag + "_roll"], axis=1)[:, :keys]
        assert roll.shape == (c["t"], keys) and int(z[tag + "_t"]) == c["t"]
        out[tag] = dict(roll=roll, keys=keys, note_min=15 if keys == 51 else 0, onset=z[tag + "_onset"], notes=z[tag + "_notes"], counts=z[tag + "_counts"])
    return meta, out


CASE_TAGS = sorted(json.loads(str(np.load(GOLD, allow_pickle=False)["meta"]))["cases"])


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def test_fixture_covers_the_cases_of_both_branches(cases):
    meta, cs = cases
    assert meta["source"] == "src/audeo/Midi_synth.py" and set(meta["lines"]) == {"process_midi", "process_roll", "GetNote"}
    for branch, keys in (("midi", 51), ("roll", 88)):
        tags = {t.split("_", 1)[1] for t in cs if t.startswith(branch + "_")}
        assert tags == {"sparse237", "sparse50", "t1", "throughout237", "throughout50", "held237", "held100", "alternating237", "alternating50", "empty60"}
        assert len(cs[f"{branch}_alternating50"]["notes"]) == keys * 25                  # the worst case: keys * ceil(t / 2)
        assert len(cs[f"{branch}_empty60"]["notes"]) == 0
        a = cs[f"{branch}_alternating237"]
        assert a["counts"][a["note_min"] + 5] == 119 and a["counts"][a["note_min"] + keys - 2] == 118      # ceil(237 / 2), floor(237 / 2)
    assert os.path.getsize(GOLD) < 1 << 20


@pytest.mark.parametrize("tag", CASE_TAGS)
def test_restatement_equals_the_reference(cases, tag):
    """The restatement on the reference's own roll -- the clip placed at its keys of 88 and padded to whole 50-frame windows, what
    `process_midi` / `process_roll` build -- gives the reference's onset matrix and notes; on the clip itself it gives the same notes
    (the appended end `T` and the offset at the first padded frame are the same frame)."""
    c = cases[1][tag]
    roll, nm, keys = c["roll"], c["note_min"], c["keys"]
    t = len(roll)
    tp = c["onset"].shape[1]
    assert c["onset"].shape[0] == 88 and tp == -(-t // 50) * 50
    full = np.zeros((tp, 88), np.uint8)
    full[:t, nm:nm + keys] = roll
    onset, counts, notes = restate(full)
    assert np.array_equal(onset, c["onset"])
    assert np.array_equal(counts, c["counts"])
    assert np.array_equal(notes + np.array([21, 0, 0], np.int32), c["notes"])
    # the clip alone, and the padded roll under lens = t
    for o2, c2, n2 in (restate(roll), restate(full[:, nm:nm + keys], lens=t)):
        assert np.array_equal(c2, c["counts"][nm:nm + keys])
        assert np.array_equal(n2 + np.array([21 + nm, 0, 0], np.int32), c["notes"])
        assert np.array_equal(o2[:, :t], c["onset"][nm:nm + keys, :t])


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from v2a_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_header_ctypes_and_exports_agree(lib):
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int v2a_roll_notes\((.*?)\);", body, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    kinds = {"const void* roll": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    want = []
    for p in params:
        typ = p.rsplit(" ", 1)[0]
        want.append(C.c_void_p if "*" in p or typ == "v2a_stream_t" else kinds[typ])
    L = lib.lib()
    assert "v2a_roll_notes" in lib.EXPORTS and hasattr(L, "v2a_roll_notes")
    assert list(L.v2a_roll_notes.argtypes) == want and len(want) == 16 and L.v2a_roll_notes.restype is C.c_int
    assert L.v2a_abi_version() == lib.ABI_VERSION == 9
    consts = dict(re.findall(r"#define (V2A_ROLL_NOTES_[A-Z_]+) (\S+)", body))
    assert (int(consts["V2A_ROLL_NOTES_MAX_KEYS"]), int(consts["V2A_ROLL_NOTES_TILE"])) == (lib.ROLL_NOTES_MAX_KEYS, lib.ROLL_NOTES_TILE) == (128, 256)
    assert consts["V2A_ROLL_NOTES_MAX_FRAMES"] == "(1" and lib.ROLL_NOTES_MAX_FRAMES == 1 << 24 and "(1 << 24)" in body
    build = open(os.path.join(ROOT, "video-to-audio-and-piano-rp_amd", "csrc", "build.sh")).read()
    assert build.count("midi_notes") == 2 and "$BUILD/midi_notes.o" in build


def test_entry_point_refuses_bad_arguments_without_a_gpu(lib):
    L = lib.lib()
    ok = dict(roll=64, elem=1, bs=51, fs=51, ks=1, thr=0.0, B=1, T=1, keys=51, lens=None, counts=64, totals=64, notes=64, cap=4, onset=None)

    def call(**kw):
        a = {**ok, **kw}
        return L.v2a_roll_notes(a["roll"], a["elem"], a["bs"], a["fs"], a["ks"], a["thr"], a["B"], a["T"], a["keys"], a["lens"], a["counts"], a["totals"],
                                a["notes"], a["cap"], a["onset"], None)

    for kw, word in ((dict(roll=None), b"null"), (dict(totals=None), b"null"), (dict(elem=2), b"elem_bytes"), (dict(keys=129), b"keys"),
                     (dict(keys=0), b"keys"), (dict(T=0), b"T=0"), (dict(B=0), b"B=0"), (dict(T=(1 << 24) + 1), b"frames"),
                     (dict(cap=-1), b"cap"), (dict(notes=None), b"cap"), (dict(elem=4, roll=66), b"alignment"), (dict(counts=66), b"alignment")):
        assert call(**kw) == -1, kw
        assert word in L.v2a_last_error(), (kw, L.v2a_last_error())


def test_roll_to_notes_checks_its_arguments_on_the_host():
    from v2a_amd import midi
    assert midi.worst_case_rows(237, 51) == 51 * 119 and midi.worst_case_rows(1, 88) == 88
    assert np.float32(midi.ROLL_THRESHOLD_BELOW) < np.float32(0.4) and np.nextafter(np.float32(midi.ROLL_THRESHOLD_BELOW), np.float32(1)) == np.float32(0.4)
    with pytest.raises(ValueError, match="b, t, keys"):
        midi.roll_to_notes(torch.zeros(4, 51, dtype=torch.uint8))
    with pytest.raises(TypeError, match="float32"):
        midi.roll_to_notes(torch.zeros(1, 4, 51, dtype=torch.float64))
    with pytest.raises(ValueError, match="keys=129"):
        midi.roll_to_notes(torch.zeros(1, 4, 129, dtype=torch.uint8))
    assert midi.roll_to_notes(torch.zeros(0, 4, 51, dtype=torch.uint8)) == []
    import v2a_amd
    assert v2a_amd.midi is midi and v2a_amd.roll_to_notes is midi.roll_to_notes and v2a_amd.write_midi is midi.write_midi
    assert v2a_amd.read_midi is midi.read_midi and v2a_amd.notes_to_roll is midi.notes_to_roll


# ---- the MIDI file -----------------------------------------------------------------------------------------------------------------
def _notes_of(c):
    return restate(c["roll"])[2] + np.array([21 + c["note_min"], 0, 0], np.int32)


@pytest.mark.parametrize("spf", [0.04, 1.0 / 30.0])
@pytest.mark.parametrize("tag", ["midi_sparse237", "roll_sparse237", "roll_alternating50", "midi_held100", "midi_t1", "roll_empty60"])
def test_file_round_trip(cases, tmp_path, tag, spf):
    from v2a_amd import midi
    c = cases[1][tag]
    notes = _notes_of(c)
    assert np.array_equal(notes, c["notes"])
    path = str(tmp_path / "clip.mid")
    assert midi.write_midi(path, notes, spf) == len(notes)
    back = midi.read_midi(path)
    assert back.shape == (len(notes), 4) and back.dtype == np.float64
    if len(notes):
        assert np.array_equal(back[:, 0], notes[:, 0]) and (back[:, 3] == 100).all()
        err = max(np.abs(back[:, 1] - notes[:, 1] * spf).max(), np.abs(back[:, 2] - notes[:, 2] * spf).max())
        print(f"{tag} spf={spf:.5f}: {len(notes)} notes, worst time error {err * 1e3:.3f} ms (half a tick: {HALF_TICK * 1e3:.3f} ms)")
        assert err <= HALF_TICK * (1 + 1e-9)
    # roll -> notes -> file -> notes -> roll
    t, keys = c["roll"].shape
    assert np.array_equal(midi.notes_to_roll(back, t, spf, note_min=c["note_min"], keys=keys), c["roll"])
    assert np.array_equal(midi.notes_to_roll(notes, t, spf, note_min=c["note_min"], keys=keys), c["roll"])


def test_written_bytes_are_the_documented_layout(tmp_path):
    """Two notes that touch (one ends where the next starts): header, tempo track and note track byte for byte."""
    from v2a_amd import midi
    path = str(tmp_path / "two.mid")
    midi.write_midi(path, np.array([[60, 0, 25], [60, 25, 50], [64, 25, 26]]), 0.04)
    raw = open(path, "rb").read()
    tick = lambda f: int(np.floor(f * 0.04 * 220 * 80 / 60 + 0.5))
    assert (tick(25), tick(26), tick(50)) == (293, 305, 587)
    want = b"MThd" + struct.pack(">IHHH", 6, 1, 2, 220)
    t0 = b"\x00\xff\x51\x03" + (750000).to_bytes(3, "big") + b"\x00\xff\x58\x04\x04\x02\x18\x08\x00\xff\x2f\x00"
    t1 = (b"\x00\xc0\x00" + b"\x00\x90\x3c\x64" + b"\x82\x25\x80\x3c\x00" + b"\x00\x90\x3c\x64" + b"\x00\x90\x40\x64" + b"\x0c\x80\x40\x00" +
          b"\x82\x1a\x80\x3c\x00" + b"\x00\xff\x2f\x00")
    want += b"MTrk" + struct.pack(">I", len(t0)) + t0 + b"MTrk" + struct.pack(">I", len(t1)) + t1
    assert raw == want
    with pytest.raises(ValueError, match="pitches"):
        midi.write_midi(path, np.array([[128, 0, 1]]), 0.04)
    with pytest.raises(ValueError, match="outside"):
        midi.notes_to_roll(np.array([[35, 0, 1]]), 4, 0.04, note_min=15, keys=51)


def test_read_midi_hand_written_bytes(tmp_path):
    """Format 0, 96 ticks a quarter: running status, a tempo change in the middle, note-on with velocity 0 as note-off, a second
    channel, a controller, a system-exclusive and a text event to be skipped, two overlapping notes of one pitch paired first in
    first out, and a note-on that never ends (dropped)."""
    from v2a_amd import midi
    trk = (b"\x00\xff\x03\x02hi"                     # track name: skipped
           b"\x00\xff\x51\x03\x07\xa1\x20"           # 500 000 us a quarter
           b"\x00\x90\x3c\x50"                       # tick 0: on 60 v80
           b"\x30\x40\x51"                           # tick 48: running status, on 64 v81
           b"\x30\x3c\x00"                           # tick 96: running status, 60 velocity 0 = off
           b"\x00\xb0\x07\x7f"                       # controller: skipped
           b"\x00\xff\x51\x03\x0f\x42\x40"           # tick 96: 1 000 000 us a quarter
           b"\x30\x80\x40\x00"                       # tick 144: off 64
           b"\x00\xf0\x03\x01\x02\xf7"               # system exclusive: skipped
           b"\x00\x91\x30\x10"                       # tick 144: channel 1, on 48 v16
           b"\x81\x40\x30\x11"                       # tick 336 (two-byte delta 192): running status, second on 48 v17
           b"\x30\x81\x30\x00"                       # tick 384: off 48 -> closes the first
           b"\x30\x30\x00"                           # tick 432: running status off 48 -> closes the second
           b"\x00\x90\x47\x40"                       # on 71, never closed
           b"\x00\xff\x2f\x00")
    path = str(tmp_path / "hand.mid")
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 0, 1, 96) + b"MTrk" + struct.pack(">I", len(trk)) + trk)
    sec = lambda tick: tick * 0.5 / 96 if tick <= 96 else 0.5 + (tick - 96) * 1.0 / 96
    want = np.array([[48, sec(144), sec(384), 16], [48, sec(336), sec(432), 17], [60, sec(0), sec(96), 80], [64, sec(48), sec(144), 81]])
    got = midi.read_midi(path)
    assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-12)
    bad = str(tmp_path / "bad.mid")
    with open(bad, "wb") as f:
        f.write(b"RIFF" + b"\x00" * 20)
    with pytest.raises(ValueError, match="header"):
        midi.read_midi(bad)
    with open(bad, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 0, 0xE728))
    with pytest.raises(ValueError, match="SMPTE"):
        midi.read_midi(bad)


def test_read_midi_format_1_tempo_track_applies_to_the_note_track(tmp_path):
    from v2a_amd import midi
    t0 = b"\x00\xff\x51\x03\x0b\x71\xb0" + b"\x83\x5c\xff\x51\x03\x05\xb8\xd8" + b"\x00\xff\x2f\x00"      # 750 000 us, at tick 476: 375 000 us
    t1 = b"\x00\x90\x3c\x64" + b"\x83\x5c\x80\x3c\x00" + b"\x00\x90\x3e\x64" + b"\x81\x5c\x80\x3e\x00" + b"\x00\xff\x2f\x00"
    path = str(tmp_path / "f1.mid")
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 2, 220))
        for t in (t0, t1):
            f.write(b"MTrk" + struct.pack(">I", len(t)) + t)
    a = 476 * 0.75 / 220
    want = np.array([[60, 0.0, a, 100], [62, a, a + 220 * 0.375 / 220, 100]])
    assert np.allclose(midi.read_midi(path), want, rtol=0, atol=1e-12)


# ---- E2TTS and the CLI -------------------------------------------------------------------------------------------------------------
def _model(keys):
    import v2a_amd
    return v2a_amd.E2TTS(transformer=dict(dim=128, dim_text=192, dim_frames=64, depth=2, heads=2, frames_heads=1, num_registers=4, max_seq_len=256,
                                          if_text_modules=True, if_cross_attn=True, if_audio_conv=True, if_text_conv=True),
                         num_channels=16, if_cond_proj_in=False, device="cpu", piano_keys=keys)


def test_piano_spf_of_both_configurations():
    assert _model(51).piano_spf == 0.04 == 3.0 * 320 / 24000
    assert _model(88).piano_spf == 2.5 * 320 / 24000 and abs(_model(88).piano_spf - 1.0 / 30.0) < 1e-15
    m = _model(51)
    with pytest.raises(ValueError, match="source"):
        m.frames_to_notes(torch.zeros(1, 1, 2, 100, 900), source="wave")
    with pytest.raises(NotImplementedError, match="video2roll_net"):
        m.frames_to_notes(torch.zeros(1, 1, 2, 100, 900), source="roll")
    with pytest.raises(NotImplementedError, match="video2roll_net"):
        m.frames_to_notes(torch.zeros(1, 1, 2, 100, 900))
    with pytest.raises(TypeError, match="threshold"):
        m.frames_to_notes(torch.zeros(1, 1, 2, 100, 900), source="roll", threshold=0.5)
    with pytest.raises(ValueError, match="frames_to_midi"):
        m.midi_to_notes(torch.zeros(1, 4, 88, dtype=torch.uint8))


def test_cli_argument_rules(tmp_path):
    from v2a_amd import cli
    base = ["ck.pt", "0", "t.scp", "0", "1", "out"]
    ap = cli.build_parser()
    assert ap.parse_args(base).midi_file is None
    assert ap.parse_args(base + ["--piano", "--midi-file", "roll"]).midi_file == "roll"
    assert ap.parse_args(base + ["--piano", "--roll2midi", "g.tar", "--midi-file", "midi"]).midi_file == "midi"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--piano", "--midi-file", "wave"])
    with pytest.raises(SystemExit):
        cli.main(base + ["--midi-file", "roll"])                                      # without --piano
    with pytest.raises(SystemExit):
        cli.main(base + ["--roll2midi", "g.tar", "--midi-file", "midi"])              # without --piano
    with pytest.raises(SystemExit):
        cli.main(base + ["--piano", "--midi-file", "midi"])                           # without --roll2midi

    class Model:
        piano_spf = 0.04

        def frames_to_midi(self, frames):
            t = frames.shape[2]
            midi = torch.zeros(2, t, 51, dtype=torch.uint8)
            midi[0, 1:3, 0] = 1
            midi[1, 0:, 50] = 1
            return midi.float(), midi

        def midi_to_notes(self, midi):
            from test_midi_notes_host import restate
            return [restate(m.numpy())[2] + np.array([36, 0, 0], np.int32) for m in midi]

    from v2a_amd import midi
    paths = cli.write_midi_rolls(Model(), torch.zeros(2, 1, 4, 100, 900), ["/x/a.mp4", "/y/b.mp4"], str(tmp_path), midi_file=True)
    assert [os.path.basename(p) for p in paths] == ["a.midi.npz", "b.midi.npz", "a.mid", "b.mid"]
    assert np.allclose(midi.read_midi(paths[2]), [[36, 0.04, 0.12, 100]], atol=HALF_TICK) and np.allclose(midi.read_midi(paths[3]), [[86, 0.0, 0.16, 100]], atol=HALF_TICK)
    paths = cli.write_midi_rolls(Model(), torch.zeros(2, 1, 4, 100, 900), ["/x/a.mp4", "/y/b.mp4"], str(tmp_path / "."))
    assert [os.path.basename(p) for p in paths] == ["a.midi.npz", "b.midi.npz"]
