"""Launch-trace guard of the DiT, Video2Roll, Roll2Midi, Encodec and image-encoder (CLIP, DINOv2) engines: what the GPU is asked to
do, pinned on the CPU.

The real Python engines run on device="cpu" against a fake libv2a_cfm that records every entry-point call: its name, its
scalars, every ctypes.Structure argument field by field, and the (key, flops, bytes) that `_lib._launch` hands to a
profiler (bench.py's roofline accounting).  Device pointers are written as (allocation index, byte offset, allocation size):
allocations are the storages reachable from the engine (plans, packed weights, Video2Roll maps and tables) and the case's own
inputs, numbered in the order they first appear in the trace; any other pointer is "tmp" (the CPU allocator reuses freed
addresses, so temporaries have no stable identity).  Nothing is computed: the DiT, Video2Roll and Roll2Midi weights are zeros, the
image encoders' and Encodec's are the seeded ones of synth.py (their host-side weight preparation runs).

tests/golden/launch_trace.json.gz holds the trace of every case below and the tile-hint decisions of the DiT engine.  A change
that means to alter the launch sequence regenerates it with `python tests/test_launch_trace.py --write [PATH]` and says so."""
import bisect
import ctypes as C
import gzip
import io
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import v2a_amd  # noqa: E402
from v2a_amd import _lib as L, synth  # noqa: E402
from v2a_amd.clip import CLIPImageEncoder  # noqa: E402
from v2a_amd.dinov2 import DINOv2ImageEncoder  # noqa: E402
from v2a_amd.dit import DiTConfig, DiTEngine  # noqa: E402
from v2a_amd.encodec import EncodecDecoder, EncodecEncoder  # noqa: E402
from v2a_amd.roll2midi import Roll2MidiEngine, expected_state_dict_shapes as r2m_shapes  # noqa: E402
from v2a_amd.video2roll import Video2RollEngine, expected_state_dict_shapes as v2r_shapes  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json.gz")
_PKG = DiTEngine.__module__.rsplit(".", 1)[0]


# ---- recording --------------------------------------------------------------------------------------------------------------
class _Trace:
    def __init__(self):
        self.roots = []         # objects that own the long-lived storages (the engine, the case's inputs)
        self.held = {}          # storage base -> storage; held, so that no temporary can take a freed engine buffer's address
        self.bases = []
        self.index = {}         # storage base -> allocation index, in order of first appearance
        self.calls = []
        self.pending = None     # (key, flops, bytes) of the _launch in progress

    def _walk(self):
        seen, stack = set(), list(self.roots)
        while stack:
            o = stack.pop()
            if id(o) in seen or o is None or isinstance(o, (int, float, str, bool, torch.device, torch.dtype)):
                continue
            seen.add(id(o))
            if isinstance(o, torch.Tensor):
                s = o.untyped_storage()
                if s.nbytes():
                    self.held.setdefault(s.data_ptr(), s)
            elif isinstance(o, dict):
                stack.extend(o.values())
            elif isinstance(o, (list, tuple)):
                stack.extend(o)
            elif type(o).__module__.startswith(_PKG):
                if hasattr(o, "__dict__"):
                    stack.extend(vars(o).values())
                for cls in type(o).__mro__:
                    stack.extend(getattr(o, n, None) for n in getattr(cls, "__slots__", ()))
        self.bases = sorted(self.held)

    def _find(self, v):
        i = bisect.bisect_right(self.bases, v) - 1
        if i >= 0:
            base = self.bases[i]
            if v < base + self.held[base].nbytes():
                return base
        return None

    def ptr(self, v):
        if not v:
            return None
        base = self._find(v)
        if base is None:
            self._walk()
            base = self._find(v)
        if base is None:
            return "tmp"
        return [self.index.setdefault(base, len(self.index)), v - base, self.held[base].nbytes()]

    def _struct(self, s):
        out = {}
        for name, ft in s._fields_:
            v = getattr(s, name)
            if issubclass(ft, C.Array):
                out[name] = [self.ptr(x) for x in v] if ft._type_ is C.c_void_p else list(v)
            else:
                out[name] = self.ptr(v) if ft is C.c_void_p else v
        return out

    def record(self, name, args, argtypes):
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments, the ABI declares {len(argtypes)}"
        rec = []
        for a, t in zip(args, argtypes):
            if hasattr(a, "_obj"):                                  # ctypes.byref(struct)
                rec.append(self._struct(a._obj))
            elif t is C.c_void_p:
                rec.append(self.ptr(a))
            else:
                assert isinstance(a, (int, float)), (name, a)
                rec.append(a)
        self.calls.append(dict(fn=name, args=rec, prof=self.pending))
        self.pending = None


class _Entry:
    def __init__(self, trace, name):
        self.trace, self.name, self.argtypes, self.restype = trace, name, None, None

    def __call__(self, *args):
        self.trace.record(self.name, args, self.argtypes or [])
        return 0


class _Fake:
    def __init__(self, trace):
        for name in L.EXPORTS:
            setattr(self, name, _Entry(trace, name))
        L._declare(self)


class _Prof:
    shapes = True

    def __init__(self, trace):
        self.trace = trace

    def launch(self, key, flops, nbytes, call):
        self.trace.pending = [key, flops, nbytes]
        call()


def _traced(run):
    """run(roots) with the fake library installed, where run appends the objects that own long-lived storages to roots; returns
    the recorded calls.  Restores the library, stream_ptr and the profiler afterwards: the same session loads the real library
    for the GPU tests."""
    tr = _Trace()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "_lib", _Fake(tr))
        mp.setattr(L, "stream_ptr", lambda: 0)
        L.set_profiler(_Prof(tr))
        try:
            run(tr.roots)
        finally:
            L.set_profiler(None)
    return tr.calls


# ---- cases ------------------------------------------------------------------------------------------------------------------
SHIPPED = dict(depth=4)                               # shipped widths; two fused skip layers; the tuned tile table applies
SMALL = dict(dim=128, dim_text=192, dim_frames=64, depth=4, heads=2, frames_heads=1, num_registers=4, num_channels=16,
             max_seq_len=256)                        # the small golden config: untuned widths, no one-launch cross-attention
MODES = ("fp32", "bf16", "bf16x3")
_SD = {}


def _state_dict(cfg):
    key = tuple(sorted(cfg.to_dict().items()))
    if key not in _SD:
        _SD[key] = {k: torch.zeros(s) for k, s in v2a_amd.expected_state_dict_shapes(cfg).items()}
    return _SD[key]


def _inputs(cfg, B, T, nc, S, *, cond=False):
    return dict(text=torch.zeros(B, T, cfg.dim_text), roll=torch.zeros(B, T, cfg.notes), ctx=torch.zeros(B, nc, cfg.ctx_dim),
                ctx_mask=torch.ones(B, nc, dtype=torch.bool), t=torch.linspace(0, 0.75, S), dt=torch.full((S,), 0.25),
                y=torch.zeros(B, T, cfg.num_channels), cond=torch.zeros(B, T, cfg.num_channels) if cond else None)


def _dit_case(cfg_kw, mode, B, T=778, nc=64, S=4, *, ctor=None, attrs=None, lens=None, cond=False, rpc=False,
              per_sample=None, switch=None):
    """One setup -> prepare -> euler_step (per_sample = n_ctx_seqs: setup without CFG, per-sample times, embed + forward as
    E2TTS.transformer_with_pred_head runs them; switch = T of a second plan, after which the first is set up again)."""
    def run(roots):
        cfg = DiTConfig(**cfg_kw, cond_proj_in=cond)
        eng = DiTEngine(cfg, _state_dict(cfg), device="cpu", compute=mode, **(ctor or {}))
        for k, v in (attrs or {}).items():
            setattr(eng, k, v)
        shapes = [T] if switch is None else [T, switch, T]
        ins = [_inputs(cfg, B, t, nc, S if per_sample is None else B, cond=cond) for t in shapes]
        roots += [eng, ins]
        for t, i in zip(shapes, ins):
            if per_sample is not None:
                eng.setup(B, t, nc, B, cfg_mode=False)
                eng.plan["per_sample_t"] = True
                eng.prepare(i["text"], i["roll"], i["ctx"], i["ctx_mask"], i["t"], lens=lens)
                eng.embed(i["y"])
                eng.forward(n_ctx_seqs=per_sample)
                eng.plan["per_sample_t"] = False
                continue
            eng.setup(B, t, nc, S)
            eng.prepare(i["text"], i["roll"], i["ctx"], i["ctx_mask"], i["t"], lens=lens, dt=i["dt"], step_cond=i["cond"])
            eng.euler_step(i["y"], 2.0, remove_parallel_component=rpc)
    return lambda: _traced(run)


def _v2r_case(mode, t=5, chunk=None):
    def run(roots):
        eng = Video2RollEngine({k: torch.zeros(s) for k, s in v2r_shapes().items()}, device="cpu", compute=mode, chunk=chunk)
        x = torch.zeros(1, 1, t, 100, 900)
        roots += [eng, x]
        eng.encode_frames(x, 3 * t)
    return lambda: _traced(run)


def _r2m_case(mode, tail=None):
    """Three 12 x 20 windows at chunk 2: a chunk of 2 and a chunk of 1, so maps and tables are built for two sizes.  tail: `refine`
    of 2 x 25 frames in windows of 10 instead (the window cutting and the width of the last, shorter window)."""
    def run(roots):
        eng = Roll2MidiEngine({k: torch.zeros(s) for k, s in r2m_shapes().items()}, device="cpu", compute=mode, chunk=2)
        x = torch.zeros(3, 1, 12, 20) if tail is None else torch.zeros(2, 25, 12)
        roots += [eng, x]
        if tail is None:
            eng.forward(x)
        else:
            eng.refine(x, window=10, tail=tail)
    return lambda: _traced(run)


def _encodec_dec_case():
    def run(roots):
        dec = EncodecDecoder(synth.random_encodec_decoder_state_dict(0), "cpu")
        emb = torch.zeros(2, 128, 9)
        roots += [dec, emb]
        dec.decoder(emb)
    return lambda: _traced(run)


def _encodec_enc_case(fused):
    """Two clips of different lengths: ragged padding and different buffer sizes."""
    def run(roots):
        enc = EncodecEncoder(synth.random_encodec_encoder_state_dict(0), "cpu", fused_stem=fused)
        waves = [torch.zeros(2500), torch.zeros(3207)]
        roots += [enc, waves]
        enc.encode_list(waves)
    return lambda: _traced(run)


# the small configs of test_clip_host.py (dp = 256 > d = 208 and kp = 640 > 588: both K paddings live) and test_dinov2_host.py
CLIP_SMALL = dict(hidden_size=208, intermediate_size=832, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                  projection_dim=128, layer_norm_eps=1e-5, hidden_act="gelu", num_channels=3)
DINOV2_SMALL = dict(hidden_size=192, num_hidden_layers=2, num_attention_heads=3, mlp_ratio=4, image_size=70, patch_size=14,
                    layer_norm_eps=1e-6, use_swiglu_ffn=True, num_channels=3)


def _vit_case(kind, mode, n, h, w, *, cfg=None, ctor=None, attrs=None, crop=False, moved=False):
    """One image encoder, chunk 2, over n seeded h x w frames: enc(frames), so n = 3 runs a chunk of 2 and a chunk of 1 (the
    buffers are rebuilt for the second size).  crop: one encode_chunk call with a tap and a uint8 crop buffer instead.  moved:
    enc.to("cpu") and a second enc(frames), for which plans and buffers are rebuilt."""
    def run(roots):
        if kind == "clip":
            c = dict(CLIP_SMALL, **(cfg or {}))
            enc = CLIPImageEncoder(synth.random_clip_vision_state_dict(c, 3), "cpu", config=c, compute=mode, chunk=2)
        else:
            c = dict(DINOV2_SMALL, **(cfg or {}))
            enc = DINOv2ImageEncoder(synth.random_dinov2_state_dict(c, 3), "cpu", config=c, compute=mode, chunk=2,
                                     **{**dict(resize=64, crop=56), **(ctor or {})})
        for k, v in (attrs or {}).items():
            setattr(enc, k, v)
        fr = torch.from_numpy(synth.synthetic_video_frames(n, h, w, 1))
        roots += [enc, fr]
        if crop:
            buf = torch.zeros(n, enc.S, enc.S, 3, dtype=torch.uint8)
            roots.append(buf)
            enc.encode_chunk(fr, taps={1: None}, crop=buf)
            return
        enc(fr)
        if moved:
            enc.to("cpu")
            enc(fr)
    return lambda: _traced(run)


CASES = {}
for _m in ("fp32", "bf16x3"):
    CASES[f"clip/{_m}"] = _vit_case("clip", _m, 3, 40, 72)                      # landscape, upscaled
    CASES[f"dinov2/{_m}"] = _vit_case("dinov2", _m, 3, 200, 300)                # SWIGLU
CASES["clip/bf16x3/crop"] = _vit_case("clip", "bf16x3", 2, 120, 90, crop=True)  # portrait, downscaled: the wider filter
CASES["dinov2/bf16x3/gelu"] = _vit_case("dinov2", "bf16x3", 3, 200, 300, cfg=dict(use_swiglu_ffn=False))
# T = 197 > 128: attention launches and the qkv / ao buffers are padded to _attn_frames(1) = _attn_frames(2) = 17 frames
CASES["dinov2/bf16x3/T197"] = _vit_case("dinov2", "bf16x3", 3, 200, 300, ctor=dict(resize=200, crop=196))
CASES["dinov2/fp32/clip_attention"] = _vit_case("dinov2", "fp32", 3, 200, 300, attrs=dict(f32_attention="v2a_clip_attention"))
CASES["dinov2/fp32/moved"] = _vit_case("dinov2", "fp32", 3, 200, 300, moved=True)
for _m in MODES:
    for _b in (1, 2, 4):                              # regimes 0, 1, 2
        CASES[f"dit/{_m}/B{_b}"] = _dit_case(SHIPPED, _m, _b)
for _m in ("bf16", "bf16x3"):
    CASES[f"dit/{_m}/B1/ragged"] = _dit_case(SHIPPED, _m, 1, lens=[700])
    CASES[f"dit/{_m}/B1/step_cond"] = _dit_case(SHIPPED, _m, 1, cond=True)
    CASES[f"dit/{_m}/B1/rope_cross"] = _dit_case(SHIPPED, _m, 1, ctor=dict(rope_cross=True))
    CASES[f"dit/{_m}/B1/rope_half"] = _dit_case(SHIPPED, _m, 1, ctor=dict(rope_layout="half"))
    CASES[f"dit/{_m}/B1/rope_half_cross"] = _dit_case(SHIPPED, _m, 1, ctor=dict(rope_layout="half", rope_cross=True))
    for _k, _v in (("fuse_xattn", False), ("fold_norm", False), ("fuse_skip", False), ("fold_gemm_all", True)):
        CASES[f"dit/{_m}/B1/{_k}={_v}"] = _dit_case(SHIPPED, _m, 1, attrs={_k: _v})
    CASES[f"dit/{_m}/B4/fold_gemm_all=True"] = _dit_case(SHIPPED, _m, 4, attrs=dict(fold_gemm_all=True))
    CASES[f"dit/{_m}/B1/remove_parallel_component"] = _dit_case(SHIPPED, _m, 1, rpc=True)
    CASES[f"dit/{_m}/per_sample/B2/ctx1"] = _dit_case(SHIPPED, _m, 2, per_sample=1)
    CASES[f"dit/{_m}/per_sample/B1/ctx0"] = _dit_case(SHIPPED, _m, 1, per_sample=0)
    CASES[f"dit/{_m}/B1/plan_switch"] = _dit_case(SHIPPED, _m, 1, switch=500)
for _m in MODES:
    CASES[f"dit_small/{_m}/B2"] = _dit_case(SMALL, _m, 2, T=40, nc=5)
    CASES[f"v2r/{_m}"] = _v2r_case(_m)
    CASES[f"v2r/{_m}/chunk2"] = _v2r_case(_m, chunk=2)
    CASES[f"r2m/{_m}"] = _r2m_case(_m)
for _m in ("bf16x3", "fp32"):
    for _t in ("pad", "own"):
        CASES[f"r2m/{_m}/refine_{_t}"] = _r2m_case(_m, tail=_t)
CASES["encodec/dec"] = _encodec_dec_case()
CASES["encodec/enc/fused"] = _encodec_enc_case(True)
CASES["encodec/enc/composed"] = _encodec_enc_case(False)


# ---- tile hints -------------------------------------------------------------------------------------------------------------
AUDIO_OPS = ("x_tfa", "skip", "qkv", "out", "q2", "out2", "ff1", "ff2")
SIDE_OPS = ("cross", "qkv", "out", "ff1", "ff2")


def _hint(eng, stream, op):
    if hasattr(eng, "_tile_hint"):
        return eng._tile_hint(stream, op)
    # the engines before the one tile-hint function: _side_hint for the text / frames streams, _main_hint for the audio stream
    return eng._main_hint(op).get("tile_hint", 0) if stream == "a" else eng._side_hint(stream, op)


def _hint_table():
    """{"mode/regime/tuned|untuned/side_tile/main_tile/stream/op": tile_hint} for every decision that is not 0."""
    out = {}
    for widths, cfg_kw in (("tuned", SHIPPED), ("untuned", SMALL)):
        cfg = DiTConfig(**cfg_kw)
        sd = _state_dict(cfg)
        for mode in MODES:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(L, "_lib", _Fake(_Trace()))
                eng = DiTEngine(cfg, sd, device="cpu", compute=mode)
            for regime, tiles in enumerate((100, 200, 400)):
                per_row = max(1, cfg.dim // 128)
                eng.plan = dict(rows=128 * -(-tiles // per_row))
                assert eng._regime() == regime
                for side_tile in (0, -1):
                    for main_tile in (-1, 14):
                        eng.side_tile, eng.main_tile = side_tile, main_tile
                        for stream, ops in (("a", AUDIO_OPS), ("t", SIDE_OPS), ("f", SIDE_OPS)):
                            for op in ops:
                                h = _hint(eng, stream, op)
                                if h:
                                    out[f"{mode}/{regime}/{widths}/{side_tile}/{main_tile}/{stream}/{op}"] = h
    return out


# ---- golden -----------------------------------------------------------------------------------------------------------------
def build_all():
    return dict(cases={name: case() for name, case in CASES.items()}, hints=_hint_table())


def _dump(obj, path):
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0) as f:
        f.write(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def _flat(v, path=""):
    if isinstance(v, dict):
        for k in sorted(v):
            yield from _flat(v[k], f"{path}.{k}" if path else k)
    elif isinstance(v, list):
        for i, x in enumerate(v):
            yield from _flat(x, f"{path}[{i}]")
    else:
        yield path, v


def _first_difference(want, got):
    """'launch #i (name): field: golden ..., now ...' of the first launch that differs, or None."""
    want = json.loads(json.dumps(want))            # tuples -> lists, as in the golden
    got = json.loads(json.dumps(got))
    for i, (w, g) in enumerate(zip(want, got)):
        if w == g:
            continue
        fw, fg = dict(_flat(w)), dict(_flat(g))
        for k in sorted(set(fw) | set(fg), key=lambda k: (k != "fn", k)):
            if fw.get(k, "<absent>") != fg.get(k, "<absent>"):
                return f"launch #{i} ({w['fn']}): {k}: golden {fw.get(k, '<absent>')!r}, now {fg.get(k, '<absent>')!r}"
    if len(want) != len(got):
        i = min(len(want), len(got))
        extra = (got if len(got) > len(want) else want)[i]["fn"]
        return f"launch #{i}: golden has {len(want)} launches, now {len(got)} (first unmatched: {extra})"
    return None


def test_golden_covers_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, golden):
    diff = _first_difference(golden["cases"][name], CASES[name]())
    assert diff is None, f"{name}: {diff}"


def test_tile_hints(golden):
    got = _hint_table()
    want = golden["hints"]
    diff = [k for k in sorted(set(want) | set(got)) if want.get(k, 0) != got.get(k, 0)]
    assert not diff, f"{diff[0]}: golden {want.get(diff[0], 0)}, now {got.get(diff[0], 0)} ({len(diff)} decisions differ)"


def test_fake_library_is_restored():
    before = (L._lib, L.stream_ptr, L._prof)
    _traced(lambda _: L.split_bf16(torch.zeros(2, 8), torch.zeros(2, 16, dtype=torch.bfloat16), rows=2, d=8))
    assert (L._lib, L.stream_ptr, L._prof) == before


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_launch_trace.py --write [PATH]")
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    _dump(build_all(), path)
    print("wrote", path, os.path.getsize(path), "bytes")
