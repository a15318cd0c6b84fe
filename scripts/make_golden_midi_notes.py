"""Golden vectors produced by the REFERENCE'S OWN CODE for the note extraction behind Roll2Midi.   *** TEST INFRASTRUCTURE ***

`src/audeo/Midi_synth.py` cannot be imported (pretty_midi, librosa and soundfile are absent, and it sets LD_PRELOAD at import), but the
three methods that turn a roll into notes need numpy and glob alone.  They are taken out of the file's syntax tree AT GENERATION TIME,
bound to a bare object that carries the attributes they read, and run against the real numpy on temporary `<start>-<end>.npz` windows
in the format the reference's inference scripts write (Roll2Midi_inference.py:79 `midi`, Video2Roll_inference.py `roll`).  Nothing of
the reference is copied into this repository: the script reads it when it runs and commits INPUTS and OUTPUTS.

  methods executed as written     lines      branch              pins
  process_midi                    66-95      self.midi = True    51-key windows placed at keys 15..65 of 88, `> 0`, onsets / offsets
  process_roll                    33-64      self.midi = False   88-key windows, `> 0`, onsets / offsets
  GetNote                         97-118     both                k-th onset with k-th offset per key, end = T for a sounding key

Both methods pad every window to 50 frames, so the reference's roll of a t-frame clip has ceil(t / 50) * 50 frames, the tail off.

Per case `<branch>_<name>` the fixture holds: `_roll` the input roll (t, 51 | 88), bits packed along the keys; `_t`; `_onset` the
reference's `onset.T` (88, ceil(t / 50) * 50) int8; `_notes` (n, 3) int32 rows (pitch, start, end) in the order of the reference's
dict (key, then start); `_counts` (88) notes per key.

Usage:  python scripts/make_golden_midi_notes.py <path of the reference checkout>      (writes tests/golden/midi_notes.npz)
"""
from __future__ import annotations

import ast
import glob
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "midi_notes.npz")
METHODS = ["process_roll", "process_midi", "GetNote"]
WINDOW = 50


def reference_methods(path):
    """The three methods of MIDISynth compiled from the reference's own syntax tree, as plain functions of `self`."""
    tree = ast.parse(open(path).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MIDISynth"]
    assert len(cls) == 1, "no class MIDISynth in " + path
    nodes = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in nodes) == sorted(METHODS), [n.name for n in nodes]
    mod = ast.Module(body=nodes, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(np=np, glob=glob, print=lambda *a, **k: None)
    exec(compile(mod, path, "exec"), ns)
    return {n: ns[n] for n in METHODS}, {n.name: (n.lineno, n.end_lineno) for n in nodes}


def run_reference(fns, roll, midi_branch: bool):
    """roll (t, 51 | 88) -> (onset.T (88, T') int8, notes (n, 3) int32, counts (88) int32) by the reference's methods."""
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "clip")
        os.makedirs(folder)
        for s in range(0, len(roll), WINDOW):
            e = min(s + WINDOW, len(roll))
            np.savez(os.path.join(folder, f"{s}-{e}.npz"), **{"midi" if midi_branch else "roll": roll[s:e]})
        # the attributes MIDISynth.__init__ sets (Midi_synth.py:11-31) and the three methods read
        me = types.SimpleNamespace(midi=midi_branch, min_key=15, max_key=65, frame=WINDOW, piano_keys=88,
                                   midi_out_folder=folder, est_roll_folder=folder)
        fns["process_midi" if midi_branch else "process_roll"](me)
        fns["GetNote"](me)
    onset = me.complete_w_Roll2Midi_onset if midi_branch else me.complete_wo_Roll2Midi_onset
    notes = me.w_Roll2Midi_notes if midi_branch else me.wo_Roll2Midi_notes
    assert list(notes) == list(range(21, 21 + 88))
    rows = [(pitch, int(s), int(e)) for pitch, spans in notes.items() for s, e in spans]
    counts = np.array([len(spans) for spans in notes.values()], np.int32)
    assert np.array_equal(onset, onset.astype(np.int8))
    return onset.astype(np.int8), np.asarray(rows, np.int32).reshape(-1, 3), counts


def sparse_roll(t, keys, seed):
    """Seeded held notes: per key, gaps and durations of a few frames to a few dozen; about a tenth of the cells on."""
    rng = np.random.default_rng(seed)
    roll = np.zeros((t, keys), np.uint8)
    for k in range(keys):
        f = int(rng.integers(0, 40))
        while f < t:
            d = int(rng.integers(1, 25))
            if rng.random() < 0.6:
                roll[f:f + d, k] = 1
            f += d + int(rng.integers(1, 60))
    return roll


def cases(keys):
    out = {}
    out["sparse237"] = sparse_roll(237, keys, 1)                      # four full windows plus 37
    out["sparse50"] = sparse_roll(50, keys, 2)                        # one window exactly
    out["t1"] = (np.arange(keys) % 3 == 0).astype(np.uint8)[None]     # one frame
    r = sparse_roll(237, keys, 3)
    r[:, 7] = 1                                                       # a key on throughout
    out["throughout237"] = r
    r = sparse_roll(50, keys, 4)
    r[:, 11] = 1
    out["throughout50"] = r                                           # ... ending with the last window: the appended end
    r = sparse_roll(237, keys, 5)
    r[:, 3] = 0
    r[200:, 3] = 1                                                    # a key held to the last frame, inside a padded window
    out["held237"] = r
    r = sparse_roll(100, keys, 6)
    r[:, keys - 1] = 0
    r[61:, keys - 1] = 1                                              # ... and at the very end of the reference's roll
    out["held100"] = r
    r = np.zeros((237, keys), np.uint8)
    r[0::2, 5] = 1                                                    # a key alternating every frame: ceil(t / 2) notes
    r[1::2, keys - 2] = 1                                             # and one starting off: floor(t / 2)
    out["alternating237"] = r
    r = np.zeros((50, keys), np.uint8)
    r[0::2] = 1                                                       # every key alternating: the worst case, keys * ceil(t / 2)
    out["alternating50"] = r
    out["empty60"] = np.zeros((60, keys), np.uint8)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__.split("Usage:")[1].strip())
    ref = sys.argv[1]
    path = os.path.join(ref, "src", "audeo", "Midi_synth.py")
    fns, where = reference_methods(path)
    out, meta = {}, dict(source="src/audeo/Midi_synth.py", lines=where, numpy=np.__version__, window=WINDOW, cases={})
    for branch, keys in (("midi", 51), ("roll", 88)):
        for name, roll in cases(keys).items():
            onset, notes, counts = run_reference(fns, roll, branch == "midi")
            tag = f"{branch}_{name}"
            out[tag + "_roll"] = np.packbits(roll, axis=1)
            out[tag + "_t"] = np.int32(len(roll))
            out[tag + "_onset"], out[tag + "_notes"], out[tag + "_counts"] = onset, notes, counts
            meta["cases"][tag] = dict(t=len(roll), keys=keys, notes=int(len(notes)))
    out["meta"] = json.dumps(meta)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(meta["cases"]), "cases; methods at", where)
    for tag, c in meta["cases"].items():
        print(f"  {tag}: t={c['t']} keys={c['keys']} notes={c['notes']}")


if __name__ == "__main__":
    main()
