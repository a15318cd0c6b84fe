"""Notes and MIDI files from the piano key rolls: the link of the reference's Audeo chain behind Roll2Midi, src/audeo/Midi_synth.py.

    process_midi / process_roll (Midi_synth.py:33-95)    the roll, binarised, and its onsets / offsets         roll_to_notes
    GetNote (:97-118)                                     per key, the k-th onset paired with the k-th offset   (csrc/midi_notes.hip, one launch)
    generate_midi (:136-148)                              a MIDI object: tempo 80, program 0, velocity 100,     write_midi
                                                          times frame * spf
    pm.fluidsynth (:147)                                  the rendering: stays outside

`roll_to_notes` is the device half: one v2a_roll_notes launch over the batch, one transfer of the totals, one of the used rows.
`write_midi` / `read_midi` are an own Standard MIDI File writer and reader: pretty_midi and mido are not dependencies, and the bytes
written here have not been compared with pretty_midi's.  `notes_to_roll` is the numpy inverse of `roll_to_notes`."""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib as L

LOWEST_PITCH = 21                # MIDI note number of piano key 0 (Midi_synth.py:107-108)
ROLL_THRESHOLD = 0.4             # Video2Roll_inference.py:71-78: a key is on where sigmoid(logit) >= 0.4
# `p >= 0.4f` as the kernel's strict comparison: p > the largest fp32 below 0.4f
ROLL_THRESHOLD_BELOW = float(np.nextafter(np.float32(ROLL_THRESHOLD), np.float32(-1.0)))


def worst_case_rows(t: int, keys: int) -> int:
    """The most notes a (t, keys) roll can hold: every key alternating from frame 0, ceil(t / 2) each."""
    return int(keys) * ((int(t) + 1) // 2)


@torch.no_grad()
def roll_to_notes(roll, lens=None, *, threshold: float = 0.0, note_min: int = 0, return_onset: bool = False, cap=None, device=None):
    """roll (b, t, keys), any strides (a transposed view of a (b, keys, t) tensor is read in place) -> a list of b int32 arrays
    (n_i, 3) of rows (pitch, start_frame, end_frame), pitch = 21 + note_min + key, ordered by pitch, then by start.

    uint8 / int8 / bool elements: on iff != 0.  float32: on iff > threshold.  lens (b): the valid frames of every clip; frames at or
    beyond count as off and a note still sounding there ends at lens[i] (None: t, the reference's `np.append(end, tmp.shape)`).
    cap: rows of the device buffer per clip, by default the worst case keys * ceil(t / 2); a clip with more notes raises.
    return_onset: also the reference's intermediate, `onset.T` (b, keys, t) int8 (+1 onset, -1 offset), as a numpy array.
    A roll that is not on a GPU goes to `device` (default cuda:0) first."""
    if not torch.is_tensor(roll):
        roll = torch.as_tensor(np.asarray(roll))
    if roll.ndim != 3:
        raise ValueError(f"roll_to_notes: a roll is (b, t, keys), got {tuple(roll.shape)}")
    if roll.dtype in (torch.bool, torch.int8):
        roll = roll.view(torch.uint8)
    if roll.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"roll_to_notes: a roll holds uint8 / int8 / bool or float32 elements, got {roll.dtype}")
    b, t, keys = roll.shape
    if b == 0:
        return ([], np.zeros((0, keys, t), np.int8)) if return_onset else []
    if t < 1 or not 1 <= keys <= L.ROLL_NOTES_MAX_KEYS or t > L.ROLL_NOTES_MAX_FRAMES:
        raise ValueError(f"roll_to_notes: t={t} keys={keys} (1 <= keys <= {L.ROLL_NOTES_MAX_KEYS}, 1 <= t <= {L.ROLL_NOTES_MAX_FRAMES})")
    L.lib()                                                          # fail loudly without the HIP library, before any copy
    if not roll.is_cuda:
        roll = roll.to(torch.device("cuda:0") if device is None else device)
    dev = roll.device
    cap = worst_case_rows(t, keys) if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"roll_to_notes: cap={cap}")
    if lens is not None:
        lens = torch.as_tensor(lens).to(dev, torch.int32).contiguous()
        if lens.shape != (b,):
            raise ValueError(f"roll_to_notes: lens is (b,) = ({b},), got {tuple(lens.shape)}")
    counts = torch.empty(b, keys, dtype=torch.int32, device=dev)
    totals = torch.empty(b, dtype=torch.int32, device=dev)
    rows = torch.empty(b, cap, 3, dtype=torch.int32, device=dev) if cap else None
    onset = torch.empty(b, keys, t, dtype=torch.int8, device=dev) if return_onset else None
    with torch.cuda.device(dev):
        L.roll_notes(roll, counts, totals, rows, strides=roll.stride(), B=b, T=t, keys=keys, cap=cap, threshold=threshold, lens=lens, onset=onset)
    n = totals.cpu().numpy()                                         # transfer 1: how many rows every clip has
    if int(n.max()) > cap:
        raise L.V2AError(f"roll_to_notes: clip {int(n.argmax())} holds {int(n.max())} notes, the buffer {cap} rows per clip "
                         f"(the worst case of a ({t}, {keys}) roll is {worst_case_rows(t, keys)})")
    used = rows[:, :int(n.max())].cpu().numpy() if int(n.max()) else np.zeros((b, 0, 3), np.int32)      # transfer 2: the used rows
    out = []
    for i in range(b):
        one = used[i, :n[i]].copy()
        one[:, 0] += LOWEST_PITCH + int(note_min)
        out.append(one)
    return (out, onset.cpu().numpy()) if return_onset else out


def notes_to_roll(notes, t: int, spf: float, *, note_min: int, keys: int) -> np.ndarray:
    """The inverse of `roll_to_notes` on the host: (t, keys) uint8, frame f of key pitch - 21 - note_min on iff
    start_frame <= f < end_frame.  Integer rows (pitch, start_frame, end_frame) are frames as they are; floating rows
    (pitch, start_s, end_s[, velocity]), what `read_midi` returns, are seconds and go to the nearest frame of `spf` seconds."""
    notes = np.asarray(notes)
    roll = np.zeros((int(t), int(keys)), np.uint8)
    if notes.size == 0:
        return roll
    if notes.ndim != 2 or notes.shape[1] < 3:
        raise ValueError(f"notes_to_roll: rows of (pitch, start, end), got {notes.shape}")
    if np.issubdtype(notes.dtype, np.integer):
        start, end = notes[:, 1].astype(np.int64), notes[:, 2].astype(np.int64)
    else:
        start, end = (np.floor(notes[:, c] / float(spf) + 0.5).astype(np.int64) for c in (1, 2))
    key = np.rint(notes[:, 0]).astype(np.int64) - LOWEST_PITCH - int(note_min)
    if key.min() < 0 or key.max() >= keys or start.min() < 0 or end.max() > t:
        raise ValueError(f"notes_to_roll: a note outside the ({t}, {keys}) roll of keys {note_min}..{note_min + keys - 1}")
    for k, s, e in zip(key, start, end):
        roll[s:e, k] = 1
    return roll


# ---- Standard MIDI File writer / reader -------------------------------------------------------------------------------------------
def _vlq(n: int) -> bytes:
    """A variable-length quantity: 7 bits a byte, most significant first, the top bit set on all but the last."""
    if not 0 <= n < 1 << 28:
        raise ValueError(f"a delta time of {n} ticks does not fit a variable-length quantity")
    out = [n & 0x7F]
    while n > 0x7F:
        n >>= 7
        out.append(0x80 | (n & 0x7F))
    return bytes(reversed(out))


def seconds_to_ticks(seconds, resolution: int, tempo: float):
    """floor(seconds * resolution * tempo / 60 + 0.5): the nearest tick of a file with `resolution` ticks a quarter at `tempo` bpm."""
    return np.floor(np.asarray(seconds, np.float64) * resolution * tempo / 60.0 + 0.5).astype(np.int64)


def write_midi(path, notes, spf: float, *, tempo: float = 80.0, velocity: int = 100, program: int = 0, resolution: int = 220) -> int:
    """Rows (pitch, start_frame, end_frame) -> a format-1 Standard MIDI File at `path`; returns the notes written.

    What `generate_midi` (Midi_synth.py:136-148) puts into its PrettyMIDI object: initial tempo 80, one instrument of program 0
    ("Acoustic Grand Piano"), velocity 100, times frame * spf seconds.  Track 0: set_tempo (60e6 / tempo microseconds a quarter), a
    4/4 time signature, end of track.  Track 1: a program change, then note-on (0x90) / note-off (0x80) events on channel 0, every one
    with its status byte (no running status), sorted by tick, offs before ons at equal ticks, then by pitch; end of track.
    division = resolution ticks a quarter; tick = floor(seconds * resolution * tempo / 60 + 0.5)."""
    notes = np.asarray(notes).reshape(-1, 3) if np.asarray(notes).size else np.zeros((0, 3), np.int64)
    pitch = notes[:, 0].astype(np.int64)
    if not (0 < resolution < 1 << 15 and 0 <= program < 128 and 0 < velocity < 128 and tempo > 0):
        raise ValueError(f"write_midi: resolution={resolution} program={program} velocity={velocity} tempo={tempo}")
    if len(notes) and (pitch.min() < 0 or pitch.max() > 127 or notes[:, 1].min() < 0 or (notes[:, 2] < notes[:, 1]).any()):
        raise ValueError("write_midi: pitches are 0..127 and 0 <= start <= end")
    on = seconds_to_ticks(notes[:, 1].astype(np.float64) * float(spf), resolution, tempo)
    off = seconds_to_ticks(notes[:, 2].astype(np.float64) * float(spf), resolution, tempo)
    events = sorted([(int(t), 0, int(p)) for t, p in zip(off, pitch)] + [(int(t), 1, int(p)) for t, p in zip(on, pitch)])
    us = int(round(60e6 / tempo))
    if not 0 < us < 1 << 24:
        raise ValueError(f"write_midi: tempo={tempo}")
    track0 = b"\x00\xff\x51\x03" + us.to_bytes(3, "big") + b"\x00\xff\x58\x04\x04\x02\x18\x08" + b"\x00\xff\x2f\x00"
    body, now = bytearray(b"\x00" + bytes([0xC0, program])), 0
    for tick, is_on, p in events:
        body += _vlq(tick - now) + bytes([0x90 if is_on else 0x80, p, velocity if is_on else 0])
        now = tick
    body += b"\x00\xff\x2f\x00"
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 2, resolution))
        for trk in (track0, bytes(body)):
            f.write(b"MTrk" + struct.pack(">I", len(trk)) + trk)
    return len(notes)


def _parse_track(data: bytes, index: int):
    """(note events [(tick, order, channel, pitch, velocity, is_on)], tempo events [(tick, microseconds)]) of one MTrk body."""
    notes, tempi, pos, tick, status, order = [], [], 0, 0, None, 0
    n = len(data)

    def vlq():
        nonlocal pos
        v = 0
        while True:
            if pos >= n:
                raise ValueError(f"read_midi: track {index} ends inside a variable-length quantity")
            c = data[pos]
            pos += 1
            v = (v << 7) | (c & 0x7F)
            if not c & 0x80:
                return v

    while pos < n:
        tick += vlq()
        if pos >= n:
            raise ValueError(f"read_midi: track {index} ends behind a delta time")
        c = data[pos]
        if c == 0xFF:                                                # meta event: type, length, data
            if pos + 2 > n:
                raise ValueError(f"read_midi: track {index} ends inside a meta event")
            kind = data[pos + 1]
            pos += 2
            ln = vlq()
            if kind == 0x51 and ln == 3 and pos + 3 <= n:
                tempi.append((tick, int.from_bytes(data[pos:pos + 3], "big")))
            pos += ln
            status = None
            if kind == 0x2F:
                break
            continue
        if c in (0xF0, 0xF7):                                        # system exclusive: length, data
            pos += 1
            ln = vlq()
            pos += ln
            status = None
            continue
        if c & 0x80:
            status = c
            pos += 1
        elif status is None:
            raise ValueError(f"read_midi: track {index} has a data byte {c:#x} at {pos} with no running status")
        kind = status & 0xF0
        if kind >= 0xF0:
            raise ValueError(f"read_midi: track {index}: status {status:#x} is no channel message")
        size = 1 if kind in (0xC0, 0xD0) else 2
        if pos + size > n:
            raise ValueError(f"read_midi: track {index} ends inside a channel message")
        if kind in (0x80, 0x90):
            vel = data[pos + 1]
            notes.append((tick, order, status & 0x0F, data[pos], vel, kind == 0x90 and vel > 0))
            order += 1
        pos += size
    return notes, tempi


def read_midi(path) -> np.ndarray:
    """A Standard MIDI File of format 0 or 1 -> (n, 4) float64 rows (pitch, start_s, end_s, velocity), ordered by pitch, then by start.

    Running status, a tempo map (every set_tempo of every track, in tick order; 120 bpm before the first) and note-on with velocity 0
    as note-off are handled; a note-off closes the oldest open note-on of its track, channel and pitch; every other event is
    skipped, and a note-on that is never closed is dropped.  SMPTE time divisions are refused."""
    raw = open(path, "rb").read()
    if raw[:4] != b"MThd" or len(raw) < 14:
        raise ValueError(f"read_midi: {path} does not start with a MIDI header chunk")
    hlen, fmt, ntrk, division = struct.unpack(">IHHH", raw[4:14])
    if fmt not in (0, 1):
        raise ValueError(f"read_midi: format {fmt} (0 and 1 are read)")
    if division & 0x8000 or division == 0:
        raise ValueError("read_midi: an SMPTE or zero time division")
    pos, tracks = 8 + hlen, []
    while pos + 8 <= len(raw) and len(tracks) < ntrk:
        tag, ln = raw[pos:pos + 4], struct.unpack(">I", raw[pos + 4:pos + 8])[0]
        if tag == b"MTrk":
            tracks.append(_parse_track(raw[pos + 8:pos + 8 + ln], len(tracks)))
        pos += 8 + ln
    # tempo map: seconds at the tick of every change
    changes = sorted(t for _, tempi in tracks for t in tempi)
    ticks, secs, us = [0], [0.0], [500000]
    for tick, u in changes:
        if tick == ticks[-1]:
            us[-1] = u
            continue
        secs.append(secs[-1] + (tick - ticks[-1]) * us[-1] * 1e-6 / division)
        ticks.append(tick)
        us.append(u)
    ticks_a, secs_a, us_a = np.asarray(ticks), np.asarray(secs), np.asarray(us, np.float64)

    def seconds(tick):
        i = int(np.searchsorted(ticks_a, tick, side="right")) - 1
        return float(secs_a[i] + (tick - ticks_a[i]) * us_a[i] * 1e-6 / division)

    rows = []
    for trk, (events, _) in enumerate(tracks):
        open_notes: dict = {}
        for tick, _, ch, pitch, vel, is_on in events:
            if is_on:
                open_notes.setdefault((ch, pitch), []).append((tick, vel))
            elif open_notes.get((ch, pitch)):
                t_on, v = open_notes[(ch, pitch)].pop(0)
                rows.append((float(pitch), seconds(t_on), seconds(tick), float(v)))
    out = np.asarray(rows, np.float64).reshape(-1, 4)
    return out[np.lexsort((out[:, 1], out[:, 0]))] if len(out) else out
