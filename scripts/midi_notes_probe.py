"""Timing of the note extraction behind Roll2Midi (midi.roll_to_notes, csrc/midi_notes.hip) next to the reference's loop.

  python scripts/midi_notes_probe.py [--out FILE]       on a machine with an MI355X

Two rolls: 750 x 51 (a 30 s clip of the 51-key configuration at 25 fps) and 2250 x 88 (75 s of the 88-key one at 30 fps), seeded held
notes.  Per roll, on the same host:
  * the reference's way, restated here: `process_midi`'s per-frame loop of two `np.setdiff1d` over the nonzero keys and `GetNote`'s
    per-key `np.where` (Midi_synth.py:83-118), on the roll already in host memory;
  * the vectorised numpy restatement the tests use (one np.diff over the roll);
  * the device path: the v2a_roll_notes launch alone (device events around back-to-back launches), and `roll_to_notes` as a user
    calls it -- launch, transfer of the totals, transfer of the used rows -- by the host's clock, and the copy of the roll to the
    host that the reference's way would need first, for a roll that was made on the device.
The three results are compared before anything is timed.  No figure here is a pass criterion."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import v2a_amd  # noqa: E402,F401
from v2a_amd import _lib as L  # noqa: E402
from v2a_amd import midi  # noqa: E402

SHAPES = ((750, 51, 15), (2250, 88, 0))


def held_notes(t, keys, seed):
    rng = np.random.default_rng(seed)
    roll = np.zeros((t, keys), np.uint8)
    for k in range(keys):
        f = int(rng.integers(0, 40))
        while f < t:
            d = int(rng.integers(2, 40))
            roll[f:f + d, k] = 1
            f += d + int(rng.integers(1, 60))
    return roll


def reference_loop(roll, note_min):
    """Midi_synth.py:83-118 restated: per frame two setdiff1d, then per key the onsets paired with the offsets."""
    full = np.zeros((len(roll), 88))
    full[:, note_min:note_min + roll.shape[1]] = roll
    full = np.where(full > 0, 1, 0)
    onset, offset = np.zeros(full.shape), np.zeros(full.shape)
    for j in range(full.shape[0]):
        if j != 0:
            onset[j][np.setdiff1d(full[j].nonzero(), full[j - 1].nonzero())] = 1
            offset[j][np.setdiff1d(full[j - 1].nonzero(), full[j].nonzero())] = -1
        else:
            onset[j][full[j].nonzero()] = 1
    onset = (onset + offset).T
    rows = []
    for i in range(onset.shape[0]):
        start, end = np.where(onset[i] == 1)[0], np.where(onset[i] == -1)[0]
        if len(start) != len(end):
            end = np.append(end, onset[i].shape)
        rows += [(21 + i, s, e) for s, e in zip(start, end)]
    return np.asarray(rows, np.int32).reshape(-1, 3)


def vectorised(roll, note_min):
    on = (roll != 0).astype(np.int8)
    d = np.diff(np.concatenate([np.zeros((1, on.shape[1]), np.int8), on, np.zeros((1, on.shape[1]), np.int8)]), axis=0)
    rows = []
    for k in range(on.shape[1]):
        rows += [(21 + note_min + k, s, e) for s, e in zip(np.flatnonzero(d[:, k] == 1), np.flatnonzero(d[:, k] == -1))]
    return np.asarray(rows, np.int32).reshape(-1, 3)


def host_ms(fn, repeats):
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(repeats):
            fn()
        ts.append((time.perf_counter() - t) * 1e3 / repeats)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("midi_notes_probe: no GPU (a timing needs one)")

    def log(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    log(f"device: {torch.cuda.get_device_name(0)}; best of 3 runs of {a.repeats} repeats, all three shown; host loops on the same machine")
    for t, keys, note_min in SHAPES:
        roll = held_notes(t, keys, t + keys)
        dev = torch.from_numpy(roll).cuda()
        want = reference_loop(roll, note_min)
        assert np.array_equal(vectorised(roll, note_min), want)
        assert np.array_equal(midi.roll_to_notes(dev[None], note_min=note_min)[0], want)
        cap = midi.worst_case_rows(t, keys)
        counts = torch.empty(1, keys, dtype=torch.int32, device="cuda")
        totals = torch.empty(1, dtype=torch.int32, device="cuda")
        rows = torch.empty(1, cap, 3, dtype=torch.int32, device="cuda")

        def launch():
            L.roll_notes(dev, counts, totals, rows, strides=dev[None].stride(), B=1, T=t, keys=keys, cap=cap)

        launch()
        torch.cuda.synchronize()
        ev = []
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.repeats):
                launch()
            e.record()
            torch.cuda.synchronize()
            ev.append(s.elapsed_time(e) * 1e3 / a.repeats)

        def whole():
            midi.roll_to_notes(dev[None], note_min=note_min)

        def copy_back():
            dev.cpu()

        whole_ms, copy_ms = host_ms(whole, a.repeats), host_ms(copy_back, a.repeats)
        ref_ms, vec_ms = host_ms(lambda: reference_loop(roll, note_min), 3), host_ms(lambda: vectorised(roll, note_min), 20)
        f = lambda v, unit=1.0: ", ".join(f"{x * unit:.1f}" for x in v)
        log(f"roll {t} x {keys} ({len(want)} notes, worst-case buffer {cap} rows = {cap * 12 / 1e3:.0f} kB):")
        log(f"  reference loop on the host (setdiff1d per frame, where per key)   {min(ref_ms):9.2f} ms   ({f(ref_ms)})")
        log(f"  vectorised numpy restatement on the host                          {min(vec_ms):9.3f} ms   ({f(vec_ms)})")
        log(f"  v2a_roll_notes launch alone, back to back (device events)         {min(ev):9.1f} us   ({f(ev)})")
        log(f"  roll_to_notes: launch + totals + used rows (host clock)           {min(whole_ms) * 1e3:9.1f} us   ({f(whole_ms, 1e3)})")
        log(f"  copy of the roll to the host, which the host loops need first     {min(copy_ms) * 1e3:9.1f} us   ({f(copy_ms, 1e3)})")
        log(f"  -> the launch is {min(ev) / (min(whole_ms) * 1e3) * 100:.0f} % of roll_to_notes (the rest: allocations, two synchronising transfers, numpy); "
            f"roll_to_notes is {min(ref_ms) / min(whole_ms):.0f}x the reference loop and {min(vec_ms) / min(whole_ms):.2f}x the vectorised restatement")


if __name__ == "__main__":
    main()
