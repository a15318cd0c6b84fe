"""Tile selection of v2a_gemm, pinned on the CPU: which kernel instantiation a call gets, for every shape class, hint and tuning.

`v2a_gemm_choose` runs v2a_gemm up to, but not including, its first HIP call; the launcher it reaches reports its own template constants
(family, split, BM x BN x BK, waves, ring depth), the workgroup count, the XCD grid and the epilogue form.  The arguments are built
directly as `GemmArgs` with fabricated, suitably aligned addresses: nothing is dereferenced, no GPU is needed.  A wrong threshold
computes correct numbers on a slower tile, which no numeric test sees; this file sees it.

tests/golden/gemm_choice.json.gz holds the answer for every case of CASES: the twelve fields of v2a_gemm_choice, or [return code, error
text] of a refusal.  It was written by the selection code as it stood BEFORE selection moved into pure functions over one tile table
(that commit's parent plus a recording patch: the same early return in the three launchers and the export), so it pins behaviour, not
the code under test.  A change that means to alter a decision regenerates it with `python tests/test_gemm_choice.py --write [PATH]`
and says so.  (`--lib SO` answers from another build of the library, e.g. a patched older commit.)

The cases:
 (a) by shape (hint 0, default tuning): M in ROWS x N in COLS for every operand family (exact fp32, fp32 A on bf16 compute, plain
     bf16, split), every epilogue / output type the family builds, dense and -- where admitted -- with offset tables, with aligned
     epilogue operands and with a misaligned output pointer (vec_epi = 0).
 (b) thresholds: every comparison of a tile count with a constant in the selectors (csrc/gemm.hip: fp32_tile_by_shape,
     plain_tile_by_shape, split_tile_by_shape), at a fixed N with M stepped in whole tile heights: the last M below it, that M + 1 (the
     first above it) and the next whole tile height.  tm tile rows x tn tile columns; M values are (tm - 1) * bm, + 1, tm * bm:
       fp32   N 1024  tiles(128,128) <  224 : tm 28 x tn 8   M 3456 3457 3584
       plain  N   64  tiles(128,64)  >= 512 : tm 512 x tn 1  M 65408 65409 65536
       plain  N  128  tiles(128,128) >= 512 : tm 512 x tn 1  M 65408 65409 65536
       plain  N  128  tiles(128,64)  >= 512 : tm 256 x tn 2  M 32640 32641 32768
       plain  N 4096  tiles(256,256) >= 400 (min_tiles_8phase)        : tm 25 x tn 16  M 6144 6145 6400
       plain  N 4096  tiles(256,256) >= 100 (eight_phase_min_tiles)   : tm 7 x tn 16   M 1536 1537 1792
       plain  N 4096  tiles(256,256) >= 512 (8-phase off)             : tm 32 x tn 16  M 7936 7937 8192
       plain  N 2048  tiles(128,256) >= 96  : tm 12 x tn 8   M 1408 1409 1536
       plain  N 1024  tiles(256,256) >= 150 : tm 38 x tn 4   M 9472 9473 9728
       plain  N 1024  tiles(128,256) >= 180 : tm 45 x tn 4   M 5632 5633 5760
       plain  N 1024  tiles(128,128) >= 180 : tm 23 x tn 8   M 2816 2817 2944
       plain  N  512  tiles(128,256) >= 150 : tm 75 x tn 2   M 9472 9473 9600
       plain  N  512  tiles(128,128) >= 256 : tm 64 x tn 4   M 8064 8065 8192
       split  N 1024  tiles(256,256) >= 150 : tm 38 x tn 4   M 9472 9473 9728
       split  N  128  tiles(128,128) >= 256 (offset tables) : tm 256 x tn 1  M 32640 32641 32768
       split  N 2048  tiles(128,128) >= 200 : tm 13 x tn 16  M 1536 1537 1664
       split  N 1024  tiles(128,128) >= 200 (GEGLU) : tm 25 x tn 8  M 3072 3073 3200
       split  N  512  tiles(128,256) >= 128 : tm 64 x tn 2   M 8064 8065 8192
       split  N 1024  tiles(64,128)  >= 160 : tm 20 x tn 8   M 1216 1217 1280
     The plain selector's last test, tiles(64,64) >= 2048 and tiles(128,64) >= 512, has no such pair: it is reached only with fewer than
     256 tiles of 128x128, i.e. fewer than 1024 of 64x64.  The fp32 selector's M > 64 is covered by M = 64 and 65 of (a).
 (c) every hint 0..17 in both spaces at 333x416, K = 128: STORE, GEGLU with bf16 output (plain) or split output (split), RESID with a
     norm_ssq producer, and STORE with offset tables.
 (d) tunings on a thin subset of (a): force_tile -1..9 (4 and 9 are refused by v2a_set_tuning, which is what the case records),
     eight_phase 0 / 1 / 2, eight_phase_min_tiles 100, xcd_order_1x8; and hints under a forced tile / a switched-off 8-phase kernel.
 (e) K in {64, 4096} on a thin subset, for the XCD grid."""
import ctypes as C
import gzip
import io
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import v2a_amd  # noqa: E402,F401
from v2a_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_choice.json.gz")
FIELDS = [f for f, _ in L.GemmChoice._fields_]
EPI = dict(store=L.EPI_STORE, sigmoid=L.EPI_SIGMOID, geglu=L.EPI_GEGLU, resid=L.EPI_RESID, gate_resid=L.EPI_GATE_RESID, gelu=L.EPI_GELU,
           swiglu=L.EPI_SWIGLU)
DTYPE = dict(f32=L.F32, bf16=L.BF16, split=L.BF16_SPLIT)
KINDS = dict(fp32=(L.F32, L.F32), a_f32=(L.F32, L.BF16), plain=(L.BF16, L.BF16), split=(L.BF16_SPLIT, L.BF16))     # (A dtype, compute dtype)


def gemm_args(kind, M, N, K=1024, epi="store", out="f32", hint=0, scattered=False, misaligned=False, norm_ssq=False):
    """One segment of K, every operand at a fabricated 16-byte aligned address (misaligned: the output pointer 4 bytes further)."""
    g = L.GemmArgs()
    wide = 2 if kind == "split" else 1                  # hi | lo planes
    g.a_dtype, g.compute_dtype = KINDS[kind]
    g.nseg, g.a[0], g.ka[0], g.lda[0] = 1, 0x10000000, K, wide * K
    g.w, g.ldw = 0x20000000, wide * K
    g.M, g.N, g.epilogue, g.tile_hint = M, N, EPI[epi], hint
    g.out, g.ldo, g.out_dtype = 0x30000000 + (4 if misaligned else 0), 2 * N, DTYPE[out]
    if epi in ("resid", "gate_resid"):
        g.resid, g.ldr = 0x40000000, N
    if epi == "gate_resid":
        g.gate = 0x50000000
    if scattered:
        g.a_row_offset, g.a_ktile_offset, g.out_row_offset = 0x70000000, 0x71000000, 0x72000000
        if kind == "split":
            g.a_lo_offset[0] = 1 << 24
    if norm_ssq:
        g.out_bf16, g.ld_out_bf16, g.norm_ssq, g.ld_norm_ssq = 0x60000000, N, 0x80000000, N // 32
    return g


def tuning(force_tile=-1, eight_phase=1, eight_phase_min_tiles=0, xcd_order_1x8=0):
    return L.Tuning(force_tile, 0, eight_phase, eight_phase_min_tiles, 0, xcd_order_1x8, 0, (C.c_int32 * 1)(0))


def answer(lib, case, entry="v2a_gemm_choose"):
    """The twelve fields of the choice, or [return code, error text].  Tuning is process-wide: a case that sets it restores the defaults."""
    tune = case.get("tune")
    try:
        if tune is not None:
            rc = lib.v2a_set_tuning(C.byref(tuning(**tune)))
            if rc:
                return [rc, lib.v2a_last_error().decode()]
        g, c = gemm_args(**case["args"]), L.GemmChoice()
        rc = lib.v2a_gemm_choose(C.byref(g), C.byref(c)) if entry == "v2a_gemm_choose" else lib.v2a_gemm(C.byref(g), None)
        return [rc, lib.v2a_last_error().decode()] if rc else [getattr(c, f) for f in FIELDS]
    finally:
        if tune is not None:
            lib.v2a_set_tuning(None)


# ---- cases ------------------------------------------------------------------------------------------------------------------
ROWS = (1, 28, 64, 65, 273, 1564, 3128, 4692, 6256, 12512, 25024, 28900, 47000, 100000, 370000, 1410000)     # clips; convolution rows
COLS = (16, 64, 128, 256, 512, 528, 1024, 1280, 1552, 2048, 3088, 4096, 8192)
# (epilogue, output type) a family builds
BUILDS = dict(
    fp32=[("store", "f32"), ("sigmoid", "f32"), ("gelu", "f32"), ("geglu", "f32"), ("swiglu", "f32"), ("resid", "f32"), ("gate_resid", "f32")],
    a_f32=[("store", "f32"), ("store", "bf16"), ("sigmoid", "f32"), ("geglu", "bf16"), ("resid", "f32"), ("gate_resid", "f32")],
    plain=[("store", "f32"), ("store", "bf16"), ("sigmoid", "f32"), ("geglu", "f32"), ("geglu", "bf16"), ("geglu", "split"), ("resid", "f32"),
           ("gate_resid", "f32")],
    split=[("store", "f32"), ("geglu", "split"), ("swiglu", "f32"), ("swiglu", "split"), ("gelu", "f32"), ("gelu", "split"), ("resid", "f32"),
           ("gate_resid", "f32")])
# (section, family, tile, threshold, N, extra arguments, tuning): section (b) of the docstring
THRESHOLDS = [
    ("fp32", (128, 128), 224, 1024, {}, None),
    ("plain", (128, 64), 512, 64, {}, None), ("plain", (128, 128), 512, 128, {}, None), ("plain", (128, 64), 512, 128, {}, None),
    ("plain", (256, 256), 400, 4096, {}, None), ("plain", (256, 256), 100, 4096, {}, dict(eight_phase_min_tiles=100)),
    ("plain", (256, 256), 512, 4096, {}, dict(eight_phase=0)), ("plain", (128, 256), 96, 2048, {}, None),
    ("plain", (256, 256), 150, 1024, {}, None), ("plain", (128, 256), 180, 1024, {}, None), ("plain", (128, 128), 180, 1024, {}, None),
    ("plain", (128, 256), 150, 512, {}, None), ("plain", (128, 128), 256, 512, {}, None),
    ("split", (256, 256), 150, 1024, {}, None), ("split", (128, 128), 256, 128, dict(scattered=True, epi="resid", K=1152), None),
    ("split", (128, 128), 200, 2048, {}, None), ("split", (128, 128), 200, 1024, dict(epi="geglu", out="split"), None),
    ("split", (128, 256), 128, 512, {}, None), ("split", (64, 128), 160, 1024, {}, None),
]
HINT_SHAPE = dict(M=333, N=416, K=128)
THIN_ROWS, THIN_COLS = (1564, 12512), (64, 512, 1024, 4096)


RING, PH8, REG = L.GEMM_RING, L.GEMM_8PHASE, L.GEMM_REGISTER_STAGED
# (arguments, the leading fields family, split, bm, bn, bk, waves_m, waves_n, stages, and the workgroup count): all of default tuning
ANCHORS = [
    (dict(kind="plain", M=1564, N=1024), (RING, 0, 64, 64, 64, 2, 2, 3), 400),
    (dict(kind="plain", M=3128, N=1024), (RING, 0, 128, 128, 64, 2, 2, 3), 200),
    (dict(kind="plain", M=1564, N=4096), (RING, 0, 128, 256, 64, 2, 4, 3), 208),
    (dict(kind="plain", M=12512, N=512), (RING, 0, 128, 256, 64, 2, 4, 3), 196),
    (dict(kind="plain", M=12512, N=1024), (PH8, 0, 256, 256, 64, 2, 4, 2), 196),
    (dict(kind="split", M=1564, N=1024), (RING, 1, 64, 128, 64, 2, 4, 3), 200),
    (dict(kind="split", M=1564, N=3088), (RING, 1, 128, 128, 64, 2, 4, 2), 325),
    (dict(kind="split", M=3128, N=3088), (PH8, 1, 256, 256, 32, 2, 4, 2), 169),
    (dict(kind="split", M=12512, N=512), (RING, 1, 128, 256, 32, 2, 4, 3), 196),
    (dict(kind="split", M=12512, N=64), (RING, 1, 64, 128, 64, 2, 4, 3), 196),
    (dict(kind="fp32", M=1564, N=1024, K=64), (REG, 0, 64, 64, 16, 2, 2, 2), 400),
    (dict(kind="fp32", M=12512, N=4096, K=64), (REG, 0, 128, 128, 16, 2, 2, 2), 3136),
    (dict(kind="fp32", M=64, N=1024, K=64), (REG, 0, 128, 128, 16, 2, 2, 2), 8),
    (dict(kind="split", M=370000, N=128, K=1152, epi="resid", scattered=True), (RING, 1, 128, 128, 64, 2, 4, 2), 2891),
    (dict(kind="split", M=1410000, N=64, K=576, epi="resid", scattered=True), (RING, 1, 128, 64, 64, 2, 2, 3), 11016),
]


def _name(section, args, tune):
    a = dict(args)
    s = "%s/%s/%s.%s/%dx%dx%d" % (section, a.pop("kind"), a.pop("epi", "store"), a.pop("out", "f32"), a.pop("M"), a.pop("N"), a.pop("K", 1024))
    s += "".join("/%s=%s" % (k, int(v)) for k, v in sorted(a.items()) if v)
    return s + "".join("/%s=%s" % kv for kv in sorted((tune or {}).items()))


def _cases():
    out = {}

    def add(section, tune=None, **args):
        out[_name(section, args, tune)] = dict(args=args, tune=tune)

    for kind, builds in BUILDS.items():                                                                        # (a)
        for M in ROWS:
            for N in COLS:
                for epi, o in builds:
                    add("a", kind=kind, M=M, N=N, epi=epi, out=o)
                    if kind != "split" or (epi, o) == ("store", "f32"):       # split operands refuse every misaligned launch alike
                        add("a", kind=kind, M=M, N=N, epi=epi, out=o, misaligned=True)
                if kind in ("plain", "split"):
                    for epi in ("store", "resid"):
                        add("a", kind=kind, M=M, N=N, epi=epi, scattered=True)
    for kind, (bm, bn), thr, N, extra, tune in THRESHOLDS:                                                     # (b)
        tm = -(-thr // -(-N // bn))
        for M in ((tm - 1) * bm, (tm - 1) * bm + 1, tm * bm):
            add("b", tune, **{**dict(kind=kind, M=M, N=N), **extra})
    for kind in ("plain", "split"):                                                                            # (c)
        for hint in range(18):
            add("c", kind=kind, hint=hint, **HINT_SHAPE)
            add("c", kind=kind, hint=hint, epi="geglu", out="bf16" if kind == "plain" else "split", **HINT_SHAPE)
            add("c", kind=kind, hint=hint, epi="resid", norm_ssq=True, **HINT_SHAPE)
            add("c", kind=kind, hint=hint, scattered=True, **HINT_SHAPE)
    tunes = [dict(force_tile=k) for k in range(-1, 10)] + [dict(eight_phase=v) for v in (0, 1, 2)] + [dict(eight_phase_min_tiles=100),
                                                                                                        dict(xcd_order_1x8=1)]
    for tune in tunes:                                                                                         # (d)
        for kind in ("fp32", "plain", "split"):
            for M in THIN_ROWS:
                for N in THIN_COLS:
                    add("d", tune, kind=kind, M=M, N=N)
                    if kind != "fp32" and "force_tile" in tune:
                        add("d", tune, kind=kind, M=M, N=N, scattered=True)
    for tune in (dict(force_tile=1), dict(force_tile=6), dict(eight_phase=0)):            # hints under a forced tile / without the 8-phase kernel
        for kind, hints in (("plain", (3, 7, 14)), ("split", (3, 5))):
            for hint in hints:
                add("d", tune, kind=kind, hint=hint, **HINT_SHAPE)
                add("d", tune, kind=kind, hint=hint, M=12512, N=1024)
    for args, _, _ in ANCHORS:
        add("anchor", **args)
    for K in (64, 4096):                                                                                       # (e)
        for kind in ("fp32", "a_f32", "plain", "split"):
            for M in THIN_ROWS + (370000,):
                for N in THIN_COLS:
                    add("e", kind=kind, M=M, N=N, K=K)
                    add("e", dict(xcd_order_1x8=1), kind=kind, M=M, N=N, K=K)
    return out


CASES = _cases()


def build_all(lib):
    return dict(fields=FIELDS, cases={name: answer(lib, case) for name, case in CASES.items()})


def _dump(obj, path):
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0) as f:
        f.write(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.lib()


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answers(lib):
    return {name: answer(lib, case) for name, case in CASES.items()}


def _show(v):
    return dict(zip(FIELDS, v)) if len(v) == len(FIELDS) else "refused (%d): %s" % tuple(v)


def test_golden_covers_every_case(golden):
    assert golden["fields"] == FIELDS
    assert sorted(golden["cases"]) == sorted(CASES)


def test_choices_match_golden(golden, answers):
    diff = [k for k in sorted(CASES) if golden["cases"].get(k) != answers[k]]
    assert not diff, "%s: golden %s, now %s (%d of %d cases differ)" % (diff[0], _show(golden["cases"].get(diff[0], [0, "<absent>"])),
                                                                          _show(answers[diff[0]]), len(diff), len(CASES))


@pytest.mark.parametrize("args,geometry,tiles", ANCHORS, ids=[_name("anchor", a, None) for a, _, _ in ANCHORS])
def test_anchor(lib, golden, args, geometry, tiles):
    """Decisions of the shipped shapes, stated here as well as in the golden: one clip, two, eight; the Video2Roll convolutions."""
    got = answer(lib, dict(args=args, tune=None))
    assert tuple(got[:8]) == geometry and got[8] == tiles, _show(got)
    assert golden["cases"][_name("anchor", args, None)] == got


def _header_table(space):
    """{hint: (bm, bn, waves_m, waves_n, stages, bk)} of the `plain hint | ...` / `split hint | ...` table in the tile_hint comment."""
    src = open(os.path.join(ROOT, "include", "v2a_cfm.h")).read()
    m = re.search(r"\* +%s hint \| tile +\| waves \(rows x columns\) \| ring depth \| K stage \| wave tile\n((?: +\* +\d+ \|.*\n)+)" % space, src)
    rows = {}
    for line in m.group(1).splitlines():
        hint, tile, waves, depth, bk, wave_tile = [c.strip().split()[0] for c in line.strip(" *").split("|")]
        (bm, bn), (wm, wn), (tm, tn) = ([int(x) for x in c.split("x")] for c in (tile, waves, wave_tile))
        assert (bm // wm, bn // wn) == (tm, tn), line                              # the table agrees with itself
        rows[int(hint)] = (bm, bn, wm, wn, int(depth), int(bk))
    return rows


PLAIN_8PHASE_HINT, SPLIT_8PHASE_HINT = L.TILE_8PHASE + 1, L.SPLIT_TILE_8PHASE


def test_every_hint_reports_the_geometry_the_header_documents(lib):
    plain, split = _header_table("plain"), _header_table("split")
    assert sorted(plain) == [h for h in range(1, 17) if h != PLAIN_8PHASE_HINT]
    assert sorted(split) == [h for h in range(1, 8) if h != SPLIT_8PHASE_HINT]
    for kind, table in (("plain", plain), ("split", split)):
        for hint, (bm, bn, wm, wn, depth, bk) in table.items():
            got = answer(lib, dict(args=dict(kind=kind, hint=hint, **HINT_SHAPE), tune=None))
            tiles = -(-HINT_SHAPE["M"] // bm) * -(-HINT_SHAPE["N"] // bn)
            assert got[:9] == [RING, int(kind == "split"), bm, bn, bk, wm, wn, depth, tiles], (kind, hint, _show(got))
    for kind, hint, bk in (("plain", PLAIN_8PHASE_HINT, 64), ("split", SPLIT_8PHASE_HINT, 32)):
        got = answer(lib, dict(args=dict(kind=kind, hint=hint, **HINT_SHAPE), tune=None))
        assert got[:9] == [PH8, int(kind == "split"), 256, 256, bk, 2, 4, 2, 4], (kind, hint, _show(got))


def test_hints_outside_a_space_are_refused(lib):
    def refusal(**args):
        got = answer(lib, dict(args=dict(**args, **HINT_SHAPE), tune=None))
        assert len(got) == 2 and got[0] == -1, _show(got)
        return got[1]
    for hint in range(8, 17):
        assert "tile_hint %d with split operands" % hint in refusal(kind="split", hint=hint)
    assert "tile_hint 17" in refusal(kind="split", hint=17) and "tile_hint 17" in refusal(kind="plain", hint=17)
    assert "unsupported epilogue" in refusal(kind="plain", hint=14, epi="geglu", out="bf16")        # wave tiles of 16 columns: no value / gate pairs
    assert "cannot write norm_ssq" in refusal(kind="plain", hint=14, epi="resid", norm_ssq=True)
    assert "needs dense rows" in refusal(kind="plain", hint=PLAIN_8PHASE_HINT, scattered=True)
    for hint in (5, 6, 7):
        assert "with split operands and offset tables" in refusal(kind="split", hint=hint, scattered=True)


def test_named_tiles_are_what_their_names_say(lib):
    def at(kind, hint):
        return dict(zip(FIELDS, answer(lib, dict(args=dict(kind=kind, hint=hint, **HINT_SHAPE), tune=None))))
    c = at("plain", L.TILE_128x128 + 1)
    assert (c["family"], c["bm"], c["bn"], c["waves_m"] * c["waves_n"]) == (RING, 128, 128, 4)
    c = at("plain", L.TILE_128x128_8WAVES + 1)
    assert (c["family"], c["bm"], c["bn"], c["waves_m"] * c["waves_n"]) == (RING, 128, 128, 8)
    c = at("plain", L.TILE_128x64_8WAVES + 1)
    assert (c["family"], c["bm"], c["bn"], c["waves_m"] * c["waves_n"]) == (RING, 128, 64, 8)
    assert (at("plain", L.TILE_8PHASE + 1)["family"], at("plain", L.TILE_8PHASE + 1)["split"]) == (PH8, 0)
    assert (at("split", L.SPLIT_TILE_8PHASE)["family"], at("split", L.SPLIT_TILE_8PHASE)["split"]) == (PH8, 1)
    c = at("split", L.SPLIT_TILE_128x256_K32)
    assert (c["family"], c["split"], c["bm"], c["bn"], c["bk"]) == (RING, 1, 128, 256, 32)


def test_forced_tile_and_hint_agree(lib):
    """gemm_force_tile = k and tile_hint = k + 1 are the same tile, for every k v2a_set_tuning admits."""
    forceable = [k for k in range(-1, 17) if lib.v2a_set_tuning(C.byref(tuning(force_tile=k))) == 0]
    lib.v2a_set_tuning(None)
    assert forceable == [-1, 0, 1, 2, 3, 5, 6, 7, 8]
    for k in forceable[1:]:
        for M, N in ((333, 416), (12512, 1024)):
            forced = answer(lib, dict(args=dict(kind="plain", M=M, N=N), tune=dict(force_tile=k)))
            assert len(forced) == len(FIELDS) and forced == answer(lib, dict(args=dict(kind="plain", M=M, N=N, hint=k + 1), tune=None)), (k, M, N)


def test_refusals_are_those_of_v2a_gemm(lib, answers):
    """Every refused case of the grid: v2a_gemm (null stream; it never gets as far as a launch) returns the same code and text."""
    refused = [k for k in sorted(CASES) if len(answers[k]) == 2]
    assert len(refused) > 500
    for k in refused:
        assert answer(lib, CASES[k], entry="v2a_gemm") == answers[k], k


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_gemm_choice.py --write [PATH] [--lib SO]")
    rest = sys.argv[2:]
    so = rest.pop(rest.index("--lib") + 1) if "--lib" in rest else None
    if so:
        rest.remove("--lib")
        lib_ = C.CDLL(so)
        L._declare(lib_)
    else:
        lib_ = L.lib()
    path = rest[0] if rest else GOLDEN
    _dump(build_all(lib_), path)
    print("wrote", path, os.path.getsize(path), "bytes,", len(CASES), "cases")
