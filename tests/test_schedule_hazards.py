"""Cross-stream hazards of DiTEngine.forward(), checked on the CPU.

forward() runs on device="cpu" with labelled fake streams injected through DiTEngine.handoffs and the launch wrappers of `_lib` replaced by
recorders.  Every launch is recorded with its stream and the strided byte ranges it reads (A segments, residual, sums of squares, modulation
tables) and writes (out, shadow planes, sums of squares); every event record and wait is recorded too.  Vector clocks give happens-before;
every pair of launches on DIFFERENT streams that touch overlapping bytes with at least one of them writing must be ordered.

Two evaluations are driven back to back, so the seam between them is checked as well.  The negative control drops the eX wait altogether:
the checker must then name exactly the pairs the wait exists for -- x_tfa of layer l on the audio stream against the feed-forward-out GEMM of
side block l + 1, on the `.sh` planes of tB / fB -- which shows that it can see the hazard `late_ex` moves the wait for."""
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import v2a_amd  # noqa: E402
from v2a_amd import _lib as L  # noqa: E402
from v2a_amd.dit import DiTConfig, DiTEngine, StreamHandoffs, _Stream  # noqa: E402

# depth 4, T = 24; num_channels = 64 so that the bf16x3 plan can take the folded layer 0
CFG = dict(dim=128, dim_text=192, dim_frames=64, depth=4, heads=2, frames_heads=1, num_registers=4, num_channels=64, max_seq_len=256)
B, T, NC, S = 1, 24, 8, 4
MODES = ("bf16x3", "bf16", "fp32")


# ---- byte ranges --------------------------------------------------------------------------------------------------------------
class Rect:
    """`rows` rows of `width` bytes, `stride` bytes apart, from address `base`."""
    __slots__ = ("base", "rows", "stride", "width")

    def __init__(self, base, rows, stride, width):
        self.base, self.rows, self.stride, self.width = int(base), int(rows), int(stride), int(width)

    @property
    def end(self):
        return self.base + (self.rows - 1) * self.stride + self.width

    def overlaps(self, o):
        if self.base >= o.end or o.base >= self.end:
            return False
        if self.stride != o.stride or self.rows == 1 or o.rows == 1 or self.stride <= 0:
            return True                                   # different pitches: the hulls overlap, take it as an overlap
        # same pitch: column intervals modulo the pitch (both narrower than a row; the hulls already share rows)
        a, b = self.base % self.stride, o.base % self.stride
        for sh in (-self.stride, 0, self.stride):
            if a < b + sh + o.width and b + sh < a + self.width:
                return True
        return False


def _es(t):
    return t.element_size()


class Launch:
    def __init__(self, idx, stream, kind, reads, writes, clock):
        self.idx, self.stream, self.kind, self.reads, self.writes, self.clock = idx, stream, kind, reads, writes, clock
        self.tag = None

    def before(self, o):
        return o.clock.get(self.stream.label, 0) >= self.clock[self.stream.label]


# ---- fake streams, events and the recording launch layer --------------------------------------------------------------------
class FakeStream:
    def __init__(self, label):
        self.label = label
        self.clock = {}


class FakeEvent:
    def __init__(self, clock, is_ex):
        self.clock, self.is_ex = clock, is_ex


class Recorder(StreamHandoffs):
    """Handoffs of forward() on fake streams + the launches that land on them.  drop_ex: waits on eX events are ignored (negative control)."""

    def __init__(self, names, drop_ex=False):
        self.main, self.st, self.sf = FakeStream("main"), FakeStream("st"), FakeStream("sf")
        self.cur = [self.main]
        self.names = names          # [(base, end, name)] of the plan's buffers
        self.launches = []
        self.events = []            # ("rec" | "wait", stream label, launch count at the time)
        self.drop_ex = drop_ex
        self.n_ex = 0
        self.side_out = {"st": 0, "sf": 0}

    # -- StreamHandoffs
    def current(self, dev):
        return self.cur[-1]

    @contextlib.contextmanager
    def on(self, stream):
        self.cur.append(stream)
        try:
            yield
        finally:
            self.cur.pop()

    def rec(self, stream):
        last = next((l for l in reversed(self.launches) if l.stream is stream), None)
        # eX: recorded on the audio stream right behind a cross-condition GEMM -- one that reads a side stream's operand, or the planes of y
        is_ex = stream is self.main and last is not None and last.kind == "gemm" and any(
            n.split(".")[0] in ("tL0", "tA", "tB", "fL0", "fA", "fB", "ybuf") for n in self.named(last.reads))
        if is_ex:
            last.tag = f"x_tfa[{self.n_ex}]"
            self.n_ex += 1
        self.events.append(("rec", stream.label, len(self.launches)))
        return FakeEvent(dict(stream.clock), is_ex)

    def wait(self, stream, event):
        self.events.append(("wait", stream.label, len(self.launches)))
        if self.drop_ex and event.is_ex:
            return
        for k, v in event.clock.items():
            stream.clock[k] = max(stream.clock.get(k, 0), v)

    # -- launches
    def name_of(self, addr):
        for b, e, n in self.names:
            if b <= addr < e:
                return n
        return None

    def named(self, rects):
        return sorted({n for n in (self.name_of(r.base) for r in rects) if n})

    def launch(self, kind, reads, writes):
        s = self.cur[-1]
        s.clock[s.label] = s.clock.get(s.label, 0) + 1
        l = Launch(len(self.launches), s, kind, [r for r in reads if r], [w for w in writes if w], dict(s.clock))
        if s is not self.main and kind == "gemm" and any(n in ("tB.sh", "fB.sh") for n in self.named(l.writes)):
            self.side_out[s.label] += 1                       # the k-th feed-forward-out GEMM of a side stream belongs to side block k
            l.tag = f"{'t' if s is self.st else 'f'}.ff_out[{self.side_out[s.label]}]"
        self.launches.append(l)

    # the wrappers of _lib that forward() launches through
    def gemm(self, a_segs, w, out, *, M, N, compute, epilogue=L.EPI_STORE, bias=None, resid=None, gate=None, step=None, ldo=None, ldr=None,
             out_bf16=None, ld_out_bf16=None, rope_table=None, norm_gamma=None, norm_ssq=None, row_ssq=None, row_norm_dim=0,
             out_bf16_split=False, a_split=False, out_split=False, out_bf16_lo_offset=0, **kw):
        reads, writes = [], []
        for seg in a_segs:
            seg = L.Operand(*seg)
            e = _es(seg.t)
            reads.append(Rect(seg.t.data_ptr(), M, seg.ld * e, seg.k * e))
            if a_split:
                reads.append(Rect(seg.t.data_ptr() + (seg.lo or seg.k) * e, M, seg.ld * e, seg.k * e))
        if resid is not None:
            reads.append(Rect(resid.data_ptr(), M, (ldr or resid.stride(-2)) * 4, N * 4))
        if row_ssq is not None:
            reads.append(Rect(row_ssq.data_ptr(), M, row_ssq.stride(-2) * 4, row_norm_dim // 32 * 4))
        for tab in (gate, norm_gamma):
            if tab is not None:
                reads.append(Rect(tab.data_ptr(), 1, 0, N * 4))
        if step is not None:
            reads.append(Rect(step.data_ptr(), 1, 0, 4))
        ldo = ldo if ldo is not None else out.stride(-2)
        ncol = N // 2 if epilogue in (L.EPI_GEGLU, L.EPI_SWIGLU) else N
        writes.append(Rect(out.data_ptr(), M, ldo * _es(out), (ldo if out_split else ncol) * _es(out)))
        if out_bf16 is not None:
            ld = ld_out_bf16 if ld_out_bf16 is not None else ldo
            writes.append(Rect(out_bf16.data_ptr(), M, ld * 2, N * 2))
            if out_bf16_split:
                writes.append(Rect(out_bf16.data_ptr() + (out_bf16_lo_offset or N) * 2, M, ld * 2, N * 2))
        if norm_ssq is not None:
            writes.append(Rect(norm_ssq.data_ptr(), M, norm_ssq.stride(-2) * 4, N // 32 * 4))
        self.launch("gemm", reads, writes)

    def dwconv(self, x, out, wt, bias, *, B, N, d, ksize, lens=None, norm=None):
        rows = B * N
        reads, writes = [Rect(x.data_ptr(), rows, d * 4, d * 4)], [Rect(out.data_ptr(), rows, d * 4, d * 4)]
        if norm is not None:
            split = bool(norm.get("split"))
            ld = norm.get("ld_out_bf16", 2 * d if split else d)
            writes.append(Rect(norm["out_bf16"].data_ptr(), rows, ld * 2, (2 * d if split else d) * 2))
            writes.append(Rect(norm["ssq"].data_ptr(), rows, norm["ssq"].stride(-2) * 4, d // 32 * 4))
            reads.append(Rect(norm["gamma"].data_ptr(), 1, 0, d * 4))
            if norm.get("step") is not None:
                reads.append(Rect(norm["step"].data_ptr(), 1, 0, 4))
        self.launch("dwconv", reads, writes)

    def rmsnorm(self, x, y, *, rows, d, gamma, step=None, ldx=None, ldy=None, split=False, **kw):
        w = d * (2 if split else 1)
        reads = [Rect(x.data_ptr(), rows, (ldx or d) * 4, d * 4), Rect(gamma.data_ptr(), 1, 0, d * 4)]
        if step is not None:
            reads.append(Rect(step.data_ptr(), 1, 0, 4))
        self.launch("rmsnorm", reads, [Rect(y.data_ptr(), rows, (ldy or w) * _es(y), w * _es(y))])

    def rope(self, qk, *, rows, row_stride, nheads, table, **kw):
        r = Rect(qk.data_ptr(), rows, row_stride * _es(qk), nheads * 64 * _es(qk))
        self.launch("rope", [r], [r])

    def attention(self, q, k, v, gate, out, *, strides, B, H, Nq, Nk, dtype, out_split=False, **kw):
        e = 2 if dtype == L.BF16 else 4
        eo = 4 if dtype == L.F32 else 2
        qs, ks, vs, gs, os_ = strides[:5]
        assert strides[5:] == (Nq * qs, Nk * ks, Nk * vs, Nq * gs, Nq * os_), "sequences are expected back to back"
        reads = [Rect(q, B * Nq, qs * e, H * 64 * e), Rect(k, B * Nk, ks * e, H * 64 * e), Rect(v, B * Nk, vs * e, H * 64 * e),
                 Rect(gate, B * Nq, gs * e, H * e)]
        self.launch("attention", reads, [Rect(out, B * Nq, os_ * eo, H * 64 * eo * (2 if out_split else 1))])

    def unmodelled(self, *a, **kw):
        raise AssertionError("a launch this test does not model: add its byte ranges")


def _plan_names(p):
    """[(base, end, name)] of the storages of a plan, `.x` / `.sh` for the residual streams."""
    out, seen = [], set()

    def add(t, name):
        s = t.untyped_storage()
        if s.nbytes() and s.data_ptr() not in seen:
            seen.add(s.data_ptr())
            out.append((s.data_ptr(), s.data_ptr() + s.nbytes(), name))

    def walk(v, name):
        if isinstance(v, _Stream):
            add(v.x, name + ".x")
            if v.sh is not None:
                add(v.sh.t, name + ".sh")
        elif isinstance(v, L.Operand):
            add(v.t, name)
        elif isinstance(v, torch.Tensor):
            add(v, name)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(x, f"{name}[{i}]")

    for k in sorted(p, key=lambda k: (isinstance(p[k], (list, tuple)) and not isinstance(p[k], (_Stream, L.Operand)), k)):
        walk(p[k], k)                                           # the named streams first: a skip's `.sh` lives in a wide buffer
    return out


_ENG = {}


def _engine(mode):
    if mode not in _ENG:
        cfg = DiTConfig(**CFG)
        sd = {k: torch.zeros(s) for k, s in v2a_amd.expected_state_dict_shapes(cfg).items()}
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(L, "lib", lambda: None)              # nothing is launched: the library is not needed
            _ENG[mode] = DiTEngine(cfg, sd, device="cpu", compute=mode)
    return _ENG[mode]


def _drive(mode, *, late_ex, cross_on_main, interleave, folded, drop_ex=False):
    eng = _engine(mode)
    eng.late_ex, eng.cross_on_main, eng.interleave_capture = late_ex, cross_on_main, interleave
    p = eng.setup(B, T, NC, S, cfg_mode=True)
    if folded:
        assert "ybuf" in p, "the bf16x3 plan takes the folded layer 0"
    rec = Recorder(_plan_names(p), drop_ex)
    p["st"], p["sf"] = rec.st, rec.sf
    old = eng.handoffs
    eng.handoffs = rec
    try:
        with pytest.MonkeyPatch.context() as mp:
            for name in ("gemm", "dwconv", "rmsnorm", "rope", "attention"):
                mp.setattr(L, name, getattr(rec, name))
            for name in ("qproj_xattn", "xattn_absorbed"):
                mp.setattr(L, name, rec.unmodelled)
            eng.forward(folded=folded)
            eng.forward(folded=folded)                        # ... and the seam to the next evaluation
    finally:
        eng.handoffs = old
        p.pop("st"), p.pop("sf")
    return rec


def _violations(rec):
    """(earlier launch, later launch, names of the shared buffers) of every unordered cross-stream pair with a write."""
    bad = []
    ls = rec.launches
    for i, a in enumerate(ls):
        for b in ls[i + 1:]:
            if a.stream is b.stream or a.before(b) or b.before(a):
                continue
            hit = [x for x, y in [(x, y) for x in a.writes for y in b.reads + b.writes] + [(x, y) for x in a.reads for y in b.writes]
                   if x.overlaps(y)]
            if hit:
                bad.append((a, b, rec.named(hit)))
    return bad


def _show(v):
    a, b, names = v
    return f"{a.stream.label}#{a.idx} {a.tag or a.kind} <-> {b.stream.label}#{b.idx} {b.tag or b.kind} on {names}"


CASES = [(m, le, com, il, fo) for m in MODES for le in (True, False) for com in (False, True) for il in (False, True)
         for fo in ((False, True) if m == "bf16x3" else (False,))]


@pytest.mark.parametrize("mode,late_ex,cross_on_main,interleave,folded", CASES)
def test_every_cross_stream_pair_is_ordered(mode, late_ex, cross_on_main, interleave, folded):
    rec = _drive(mode, late_ex=late_ex, cross_on_main=cross_on_main, interleave=interleave, folded=folded)
    assert {l.stream.label for l in rec.launches} == {"main", "st", "sf"}
    bad = _violations(rec)
    assert not bad, "\n".join(_show(v) for v in bad[:10])


@pytest.mark.parametrize("mode", ("bf16x3", "bf16"))
@pytest.mark.parametrize("interleave", (False, True))
def test_late_ex_moves_the_wait_and_nothing_else(mode, interleave):
    """Same launches on the same streams in the same order; the two eX waits of a layer stand in front of the side blocks' last launch."""
    on = _drive(mode, late_ex=True, cross_on_main=False, interleave=interleave, folded=False)
    off = _drive(mode, late_ex=False, cross_on_main=False, interleave=interleave, folded=False)
    key = lambda r: [(l.stream.label, l.kind, r.named(l.reads), r.named(l.writes)) for l in r.launches]
    assert key(on) == key(off)
    assert [e for e in on.events if e[0] == "rec"] == [e for e in off.events if e[0] == "rec"]
    assert len(on.events) == len(off.events) and on.events != off.events
    for r, late in ((on, True), (off, False)):
        for kind, label, at in r.events:
            if kind == "wait" and label != "main" and at < len(r.launches):
                nxt = next(l for l in r.launches[at:] if l.stream.label == label)
                if (nxt.tag or "").startswith(("t.ff_out", "f.ff_out")):
                    assert late, "a wait in front of a side block's last launch without late_ex"
    assert sum(1 for k, label, at in on.events if k == "wait" and label != "main" and at < len(on.launches)
               and (next(l for l in on.launches[at:] if l.stream.label == label).tag or "").startswith(("t.ff_out", "f.ff_out"))) == 2 * 2 * 3


@pytest.mark.parametrize("mode", ("bf16x3", "bf16"))
@pytest.mark.parametrize("late_ex", (True, False))
def test_negative_control_names_the_hazard(mode, late_ex):
    """Without the eX wait: x_tfa of layer l against the feed-forward-out GEMM of side block l + 1, on the `.sh` planes -- and only those."""
    rec = _drive(mode, late_ex=late_ex, cross_on_main=False, interleave=False, folded=False, drop_ex=True)
    got = {(a.tag, b.tag, n) for a, b, names in _violations(rec) for n in names}
    depth = CFG["depth"]
    want = set()
    for ev in range(2):                                     # two evaluations: x_tfa and side blocks count on
        for l in range(1, depth - 1):                       # layer 0 reads tL0 / fL0, which no evaluation writes
            for s in "tf":
                want.add((f"x_tfa[{ev * (depth - 1) + l}]", f"{s}.ff_out[{ev * (depth - 1) + l + 1}]", f"{s}B.sh"))
    assert got == want, (sorted(got - want, key=str), sorted(want - got, key=str))
