"""The environment knobs (csrc/pvol_env.h) through pvol_env_parse: every read point over a caller-supplied table of
(name, value) pairs, never the process environment.  Needs no GPU.  The expectations are the table of DESIGN.md 4.10 worked out by
hand for each value, not produced by running the parser.  BIG is 2^32 + 3: the 64-bit parses (atol, atoll) keep it, the float ones
round it to 2^32, and the int ones (atoi, which glibc defines as strtol cut to 32 bits) see 3 -- that is what the knobs did before
they had one reader, so it is pinned here as it is."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")
BIG = str(2 ** 32 + 3)
VALUES = (None, "", "0", "1", "10", "-3", "abc", BIG)   # None: unset
U32 = 0xffffffff


class CtxKnobs(C.Structure):
    _fields_ = [("forceSeq", C.c_bool), ("noGroup", C.c_bool), ("noLite", C.c_bool), ("noMoments", C.c_bool), ("lpNoSort", C.c_bool),
                ("tileGeneral", C.c_bool), ("groupWavesPerCU", C.c_int), ("fixWavesPerCU", C.c_int), ("tileWaves", C.c_int),
                ("groupPrecore", C.c_float)]


class LaunchKnobs(C.Structure):   # as tests/test_launch_plan.py mirrors it
    _fields_ = [("sliceRays", C.c_int64), ("specPool", C.c_int64), ("tileBatchRays", C.c_int64), ("groupGuess", C.c_float),
                ("fxgWiden", C.c_float), ("fxgAim", C.c_float), ("fixExact", C.c_int32)]


class EnvKnobs(C.Structure):
    _fields_ = [("ctx", CtxKnobs), ("liCoalesce", C.c_uint32), ("subgrid", C.c_int32), ("launch", LaunchKnobs),
                ("shootRankCapMax", C.c_uint32), ("shootPoolStart", C.c_uint32), ("shootWpe", C.c_int32), ("tileDebugSet", C.c_int32),
                ("tileDebug", C.c_uint32), ("pad", C.c_uint32)]


def f32(x):
    return C.c_float(x).value


FLAG = (False, False, False, True, True, False, False, False)          # on iff the first character is '1'
I64 = (0, 0, 0, 1, 10, -3, 0, 2 ** 32 + 3)                             # atoll, unset 0
REAL = (0.0, 0.0, 0.0, 1.0, 10.0, -3.0, 0.0, 2.0 ** 32)                # atof, unset 0
LOWERED = (U32, U32, U32, 1, 10, U32, U32, U32)                        # what a knob that only lowers leaves of 2^32 - 1
# knob -> (where it lands, the eight expectations in the order of VALUES)
ROWS = {
    "PVOL_FORCE_SEQ": (lambda k: k.ctx.forceSeq, FLAG),
    "PVOL_NO_GROUP": (lambda k: k.ctx.noGroup, FLAG),
    "PVOL_NO_LITE": (lambda k: k.ctx.noLite, FLAG),
    "PVOL_NO_MOMENTS": (lambda k: k.ctx.noMoments, FLAG),
    "PVOL_LPHOTON_NO_SORT": (lambda k: k.ctx.lpNoSort, FLAG),
    "PVOL_TILE_GENERAL": (lambda k: k.ctx.tileGeneral, FLAG),
    "PVOL_GROUP_WAVES": (lambda k: k.ctx.groupWavesPerCU, (12, 1, 1, 1, 10, 1, 1, 3)),        # unset 12; else max(1, atoi)
    "PVOL_FIX_WAVES": (lambda k: k.ctx.fixWavesPerCU, (16, 1, 1, 1, 10, 1, 1, 3)),            # unset 16; else max(1, atoi)
    "PVOL_TILE_WAVES": (lambda k: k.ctx.tileWaves, (0, 0, 0, 1, 10, 0, 0, 3)),                # unset 0; else max(0, atoi)
    "PVOL_LI_COALESCE": (lambda k: k.liCoalesce, (0, 0, 0, 0, 10, 0, 0, 0)),                  # atol; 2..4096, anything else 0
    "PVOL_GROUP_PRECORE": (lambda k: k.ctx.groupPrecore, tuple(f32(v) for v in (0.7, 0.7, 0.0, 1.0, 1.0, 0.7, 0.7, 1.0))),
    "PVOL_SLICE_RAYS": (lambda k: k.launch.sliceRays, I64),
    "PVOL_SPEC_POOL": (lambda k: k.launch.specPool, I64),
    "PVOL_TILE_BATCH_RAYS": (lambda k: k.launch.tileBatchRays, I64),
    "PVOL_GROUP_GUESS": (lambda k: k.launch.groupGuess, tuple(f32(v) for v in (1.15, 1.15, 1.15, 1.0, 10.0, 1.15, 1.15, 2.0 ** 32))),
    "PVOL_FXG_WIDEN": (lambda k: k.launch.fxgWiden, REAL),
    "PVOL_FXG_AIM": (lambda k: k.launch.fxgAim, REAL),
    "PVOL_FIX_EXACT": (lambda k: k.launch.fixExact, (0, 1, 1, 1, 1, 1, 1, 1)),                # 1 iff set at all
    "PVOL_SUBGRID": (lambda k: k.subgrid, (-1, 0, 0, 1, 1, 1, 0, 1)),                         # unset -1 (occupancy decides); else atoi != 0
    "PVOL_SHOOT_RANK_CAP_MAX": (lambda k: k.shootRankCapMax, LOWERED),
    "PVOL_SHOOT_POOL_START": (lambda k: k.shootPoolStart, LOWERED),
    "PVOL_SHOOT_WPE": (lambda k: k.shootWpe, (2, 2, 2, 2, 2, 2, 2, 3)),                       # 3 or 4; everything else 2
    "PVOL_TILE_DEBUG": (lambda k: (k.tileDebugSet, k.tileDebug),                              # set: (uint32_t)atoi; unset: untouched
                        ((0, 0), (1, 0), (1, 0), (1, 1), (1, 10), (1, U32 - 2), (1, 0), (1, 3))),
}
BOUNDARIES = [
    ("PVOL_LI_COALESCE", ("1", "2", "4096", "4097"), (0, 2, 4096, 0)),
    ("PVOL_GROUP_GUESS", ("0.99", "1", "1.3", "nan"), (f32(1.15), 1.0, f32(1.3), f32(1.15))),
    ("PVOL_SHOOT_WPE", ("2", "3", "4", "5"), (2, 3, 4, 2)),
    ("PVOL_FIX_EXACT", ("",), (1,)),
    ("PVOL_FORCE_SEQ", ("01", "true", "1x"), (False, False, True)),
    ("PVOL_GROUP_PRECORE", ("0.6", "3", "-1"), (f32(0.6), 1.0, f32(0.7))),
]


@pytest.fixture(scope="module")
def parse():
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_env_parse.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(EnvKnobs)]
    L.pvol_env_parse.restype = None

    def run(table):
        names = (C.c_char_p * max(1, len(table)))(*[n.encode() for n in table])
        values = (C.c_char_p * max(1, len(table)))(*[v.encode() for v in table.values()])
        out = EnvKnobs()
        L.pvol_env_parse(names, values, len(table), C.byref(out))
        return out
    return run


def test_the_mirror_has_the_records_size():
    """static_assert(sizeof(CtxKnobs) == 24 && sizeof(LaunchKnobs) == 40 && sizeof(EnvKnobs) == 96) in pvol_env.h"""
    assert (C.sizeof(CtxKnobs), C.sizeof(LaunchKnobs), C.sizeof(EnvKnobs)) == (24, 40, 96)
    assert re.search(r"static_assert\(sizeof\(CtxKnobs\) == 24 && sizeof\(LaunchKnobs\) == 40 && sizeof\(EnvKnobs\) == 96",
                     open(os.path.join(CSRC, "pvol_env.h")).read())


def test_the_table_covers_every_knob_the_library_names():
    named = set()
    for f in os.listdir(CSRC):
        if f.endswith((".h", ".hip")):
            named |= set(re.findall(r'get\("(PVOL_[A-Z_]+)"\)', open(os.path.join(CSRC, f)).read()))
    assert named == set(ROWS) and len(ROWS) == 23


@pytest.mark.parametrize("knob", sorted(ROWS))
def test_knob_by_value(parse, knob):
    where, want = ROWS[knob]
    base = parse({})
    for value, w in zip(VALUES, want):
        k = parse({} if value is None else {knob: value})
        assert where(k) == w, (knob, value)
        for other, (at, _) in ROWS.items():   # and nothing else moves
            if other != knob:
                assert at(k) == at(base), (knob, value, other)


@pytest.mark.parametrize("knob,values,want", BOUNDARIES)
def test_knob_boundaries(parse, knob, values, want):
    for value, w in zip(values, want):
        assert ROWS[knob][0](parse({knob: value})) == w, (knob, value)


def test_the_process_environment_is_not_consulted(parse, monkeypatch):
    for knob in ROWS:
        monkeypatch.setenv(knob, "1")
    k = parse({})
    for knob, (where, want) in ROWS.items():
        assert where(k) == want[0], knob
    k = parse({"PVOL_GROUP_WAVES": "7", "PVOL_SLICE_RAYS": "128"})   # several pairs at once, the later ones too
    assert (k.ctx.groupWavesPerCU, k.launch.sliceRays, k.ctx.fixWavesPerCU) == (7, 128, 16)


def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}


def test_one_place_asks_the_process():
    hits = [(f, i + 1) for f, t in sources().items() for i, line in enumerate(t.split("\n")) for _ in re.findall(r"getenv\s*\(", line)]
    assert len(hits) == 1 and hits[0][0] == "pvol_api.hip", hits


def test_raw_hip_handles_live_in_the_owners_only():
    names = ("hipEventCreate", "hipEventDestroy", "hipStreamCreate", "hipStreamDestroy", "hipHostMalloc", "hipHostFree", "hipMalloc", "hipFree")
    hits = sorted({(f, n) for f, t in sources().items() for n in names if n in t and f != "pvol_host.h"})
    assert hits == []
    host = sources()["pvol_host.h"]
    assert all(n in host for n in names)
