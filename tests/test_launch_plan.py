"""The plan of a batch (plan_path / plan_size in pvol_api.hip, exported as pvol_plan_batch next to pvol_rccl_symbol): which path, tile
pre-pass and li_group_kernel form a batch takes, and the sizes it reserves.  Pure host arithmetic: needs no GPU.  Every expectation
below is read off the conditions pvol_launch_batch had before the planner existed, not produced by running the planner."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, abi

NONE, HOMOGENEOUS, GRID = 0, 1, 2                      # pvol_volume.kind
PAR, SLICED, SEQ = 0, 1, 2                             # BatchPlan.path
T_NONE, T_COUNT, T_GRID_COUNT, T_FUSED = 0, 1, 2, 3    # BatchPlan.tile
DEFER_REC = 32                                         # sizeof(DeferRec), pvol_dev.h


class Knobs(C.Structure):
    _fields_ = [("sliceRays", C.c_int64), ("specPool", C.c_int64), ("tileBatchRays", C.c_int64), ("groupGuess", C.c_float),
                ("fxgWiden", C.c_float), ("fxgAim", C.c_float), ("fixExact", C.c_int32)]


class PlanIn(C.Structure):
    _fields_ = [("nLights", C.c_int32), ("volKind", C.c_int32), ("g", C.c_float), ("nPhotons", C.c_uint32), ("nUsed", C.c_int32),
                ("candCap", C.c_int32), ("maxSteps", C.c_int32), ("nTris", C.c_int32), ("roulette", C.c_int32), ("distant", C.c_int32),
                ("forceSeq", C.c_int32), ("noGroup", C.c_int32), ("noLite", C.c_int32), ("statsOn", C.c_int32),
                ("nCU", C.c_int32), ("groupWavesPerCU", C.c_int32), ("fixWavesPerCU", C.c_int32), ("tileWaves", C.c_int32),
                ("nRays", C.c_uint32), ("nStreams", C.c_uint32), ("maxRays", C.c_uint32), ("hasInit", C.c_int32), ("transOnly", C.c_int32),
                ("hasTile", C.c_int32), ("spp", C.c_uint32), ("specOn", C.c_int32), ("hasTauOut", C.c_int32), ("knobs", Knobs)]


class BatchPlan(C.Structure):
    _fields_ = [("rc", C.c_int32), ("path", C.c_int32), ("tile", C.c_int32), ("groupForm", C.c_int32), ("fixGroup", C.c_int32),
                ("liteResolve", C.c_int32), ("resolve", C.c_int32), ("recStride", C.c_uint32), ("sliceM", C.c_uint32), ("nSlices", C.c_uint32),
                ("nWaves", C.c_uint32), ("gWaves", C.c_uint32), ("fixWaves", C.c_uint32), ("tileWavesPerTask", C.c_int32),
                ("recBytes", C.c_uint64), ("stateBytes", C.c_uint64), ("deferWant", C.c_uint64), ("specCap", C.c_uint64),
                ("ldsSeq", C.c_uint64), ("ldsPar", C.c_uint64), ("ldsResolve", C.c_uint64), ("ldsGroup", C.c_uint64), ("ldsTile", C.c_uint64),
                ("kernel", C.c_char_p)]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_plan_batch.argtypes = [C.POINTER(PlanIn), C.POINTER(BatchPlan)]
    L.pvol_plan_batch.restype = None
    L.pvol_rec_stride.argtypes = [C.c_int, C.c_bool]
    L.pvol_rec_stride.restype = C.c_size_t
    L.pvol_li_piece.argtypes = [C.c_int, C.c_int, C.c_uint32]
    L.pvol_li_piece.restype = C.c_uint32
    return L


def cand_cap(n_used):   # pvol_set_scene
    return (n_used + 63) // 64 * 64 + 192


def plan(lib, **kw):
    """Row 1 of the table: homogeneous, one distant light, g 0, a photon map, nused 50, no initial state, no tile."""
    v = dict(nLights=1, volKind=HOMOGENEOUS, g=0.0, nPhotons=100000, nUsed=50, maxSteps=100, nTris=0, roulette=0, distant=1,
             nCU=256, groupWavesPerCU=12, fixWavesPerCU=16, nRays=4000, nStreams=4, maxRays=1000, spp=0)
    knobs = dict(groupGuess=1.15)
    for k, x in kw.items():
        (knobs if k in dict(Knobs._fields_) else v)[k] = x
    v.setdefault("candCap", cand_cap(v["nUsed"]))
    if v.get("hasTile"):
        v["spp"] = v["spp"] or 4
    i = PlanIn(**v)
    i.knobs = Knobs(**knobs)
    out = BatchPlan()
    lib.pvol_plan_batch(C.byref(i), C.byref(out))
    return out


def shape(p):
    return p.rc, p.path, p.tile, p.groupForm, (p.kernel or b"").decode()


TILE = dict(hasTile=1)
GRID1 = dict(volKind=GRID, hasTile=1)            # row 8
TWO = dict(nLights=2, hasTile=1)                 # row 10
OK = abi.PVOL_OK
ROWS = [
    (1, {}, (OK, PAR, T_NONE, 1, "li_group_kernel")),
    (2, dict(g=0.6), (OK, PAR, T_NONE, 0, "li_par_kernel")),
    (3, dict(nUsed=500), (OK, PAR, T_NONE, 0, "li_par_kernel")),
    (4, dict(noGroup=1), (OK, PAR, T_NONE, 0, "li_par_kernel")),
    (5, dict(hasInit=1), (OK, SLICED, T_NONE, 1, "li_group_kernel")),
    (6, dict(hasInit=1, statsOn=1), (OK, SLICED, T_NONE, 0, "li_replay_kernel")),
    (7, TILE, (OK, PAR, T_COUNT, 1, "li_group_kernel")),
    (8, GRID1, (OK, SLICED, T_GRID_COUNT, 2, "li_group_kernel")),
    (9, dict(GRID1, noLite=1), (OK, SLICED, T_FUSED, 2, "li_group_kernel")),   # the group form does not ask for liteResolve
    (10, TWO, (OK, SLICED, T_FUSED, 1, "li_group_kernel")),
    (11, dict(TWO, nUsed=500), (OK, SLICED, T_FUSED, 1, "li_group_kernel")),
    (12, dict(TILE, roulette=1), (OK, SLICED, T_FUSED, 0, "li_replay_kernel")),
    (13, dict(TILE, forceSeq=1), (OK, SEQ, T_COUNT, 0, "li_seq_kernel")),
    (15, dict(volKind=NONE, nLights=2, nPhotons=0), (OK, SEQ, T_NONE, 0, "li_seq_kernel")),
    (16, dict(volKind=GRID, transOnly=1), (OK, SEQ, T_NONE, 0, "li_seq_kernel")),
    (19, dict(TWO, specOn=1), (OK, SLICED, T_FUSED, 1, "li_group_kernel")),
    # further corners of the same conditions
    (20, dict(nUsed=9), (OK, PAR, T_NONE, 0, "li_par_kernel")),                 # the bucket plan needs k >= 10
    (21, dict(nUsed=64, candCap=320), (OK, PAR, T_NONE, 0, "li_par_kernel")),   # and, on PAR only, candCap <= 256
    (22, dict(nPhotons=0), (OK, PAR, T_NONE, 0, "li_par_kernel")),
    (23, dict(statsOn=1), (OK, PAR, T_NONE, 1, "li_group_kernel")),             # PAR's form does not mind the counters
    (24, dict(hasInit=1, nUsed=500), (OK, SLICED, T_NONE, 1, "li_group_kernel")),   # no upper bound on the SLICED form
    (25, dict(forceSeq=1), (OK, SEQ, T_NONE, 0, "li_seq_kernel")),
    (26, dict(volKind=GRID), (OK, SLICED, T_NONE, 2, "li_group_kernel")),
]


@pytest.mark.parametrize("row,kw,want", ROWS, ids=["row%d" % r[0] for r in ROWS])
def test_plan_rows(lib, row, kw, want):
    assert shape(plan(lib, **kw)) == want


@pytest.mark.parametrize("kw", [dict(TWO, forceSeq=1),            # row 14: nothing counts the draws of two lights for li_seq_kernel
                                dict(volKind=GRID, hasTauOut=1),  # row 17: *T of a VolumeGrid is no TauRec
                                dict(GRID1, hasTauOut=1),
                                dict(GRID1, forceSeq=1),
                                dict(GRID1, specOn=1),            # row 18: only the FUSED pre-pass walks the segments
                                dict(TWO, specOn=1, noLite=1),    # ... and only in its liteResolve form
                                dict(TWO, specOn=1, roulette=1)])
def test_plan_refuses(lib, kw):
    assert plan(lib, **kw).rc == abi.PVOL_E_UNSUPPORTED


def test_plan_flags_of_the_sliced_path(lib):
    p = plan(lib, hasInit=1)                     # row 5
    assert (p.resolve, p.liteResolve, p.fixGroup) == (1, 1, 0)
    assert (plan(lib, **GRID1).resolve, plan(lib, **GRID1).liteResolve) == (1, 1)                       # row 8
    p = plan(lib, **dict(GRID1, noLite=1))       # row 9
    assert (p.resolve, p.liteResolve) == (0, 0)
    assert plan(lib, **TWO).resolve == 0         # row 10: the FUSED pre-pass wrote the records
    assert plan(lib, **dict(TWO, nUsed=500)).fixGroup == 1                                              # row 11
    assert plan(lib, **dict(TWO, nUsed=500, fixExact=1)).fixGroup == 0
    assert plan(lib, **dict(TWO, nUsed=100)).fixGroup == 0
    assert plan(lib, hasInit=1, roulette=1).liteResolve == 0
    assert plan(lib, nUsed=500, candCap=256).fixGroup == 0   # PAR never pads its hand-over list


def test_plan_sizes(lib):
    # homogeneous, 100 march steps: 16 + round16(100) = 128 bytes a slot; 1000 rays a stream round up to one slice of 1024
    p = plan(lib, hasInit=1)
    assert (p.recStride, p.sliceM, p.nSlices) == (128, 1024, 1)
    assert (p.recBytes, p.stateBytes) == (128 * 4 * 1024, 4 * 625 * 4)
    assert p.nWaves == 1024 // 64 * 4 and p.gWaves == 1024 // 512 * 4 and p.fixWaves == 256 * 16
    assert p.deferWant == 1024 * 4 + 65536
    assert (p.ldsPar, p.ldsResolve, p.ldsSeq) == (256 * 8 + 5120, 624 * 4 + 400, 624 * 4 + 256 * 8 + 400 + 5120)
    p = plan(lib, hasInit=1, sliceRays=64)
    assert (p.sliceM, p.nSlices) == (64, 16)
    assert plan(lib, hasInit=1, sliceRays=63).sliceM == 1024          # the knob counts from 64
    assert plan(lib, hasInit=1, maxRays=0).nSlices == 1               # empty streams still run one slice
    # VolumeGrid: the drawn offsets of every step, 8 bytes each
    assert plan(lib, volKind=GRID).recStride == 16 + 112 + 800 == 928
    assert lib.pvol_rec_stride(100, False) == 128 and lib.pvol_rec_stride(100, True) == 928 and lib.pvol_rec_stride(0, False) == 16
    # the 4 GB record budget: 928-byte slots, 4096 streams
    p = plan(lib, volKind=GRID, nStreams=4096, maxRays=1 << 20, nRays=1 << 30)
    assert p.sliceM == ((4 << 30) // (928 * 4096)) // 64 * 64 and p.recBytes <= 4 << 30
    # a tile: whole pixels in a slice
    p = plan(lib, **dict(TWO, spp=256, maxRays=1000, sliceRays=320))
    assert p.sliceM == 256
    p = plan(lib, **dict(TWO, spp=256, maxRays=100000))
    assert p.sliceM % 256 == 0 and p.sliceM == (100000 + 63) // 64 * 64 // 256 * 256
    assert p.tileWavesPerTask == 1 and plan(lib, **TILE).tileWavesPerTask == 4       # FUSED: one wave; COUNT with 4 tasks on 256 CUs
    assert plan(lib, **dict(TILE, nStreams=4096)).tileWavesPerTask == 1 and plan(lib, **dict(TILE, tileWaves=8)).tileWavesPerTask == 8
    # tile_waves_per_task at its thresholds on 256 CUs: 12 tasks a CU and more one wave, 3 and more two, fewer four
    for n_streams, waves in [(3072, 1), (3071, 2), (768, 2), (767, 4)]:
        assert plan(lib, **dict(TILE, nStreams=n_streams)).tileWavesPerTask == waves
    for tile_waves in (0, 2, 16):                                     # FUSED ignores tileWaves
        assert plan(lib, **dict(TWO, tileWaves=tile_waves)).tileWavesPerTask == 1
    # nused beyond the bucket plan: 64 list entries a ray, the list within 8 GB
    cap = (8 << 30) // DEFER_REC
    p = plan(lib, hasInit=1, nUsed=500, nStreams=1024, maxRays=1 << 20, nRays=1 << 30)
    assert p.sliceM == cap // 64 // 1024 and p.sliceM * 1024 * 64 <= cap
    assert p.deferWant == cap                       # 64 per ray + 65536 would pass it
    p = plan(lib, hasInit=1, nUsed=500)
    assert p.deferWant == 1024 * 4 * 64 + 65536
    # PAR: half an entry a ray
    p = plan(lib)
    assert (p.deferWant, p.nWaves, p.gWaves) == (4000 // 2 + 65536, 63, 8)
    assert (p.recStride, p.sliceM, p.recBytes, p.stateBytes, p.specCap) == (0, 0, 0, 0, 0)
    assert plan(lib, g=0.6).deferWant == 0


def test_plan_spec_pool(lib):
    p = plan(lib, **dict(TWO, specOn=1))            # row 19
    assert p.specCap == max(65536, 2 * p.sliceM * 4)
    p = plan(lib, **dict(TWO, specOn=1, nStreams=64, maxRays=1 << 20, nRays=1 << 26))
    assert p.sliceM == (8 << 20) // 64 and p.specCap == 1 << 24      # 8 M / nStreams rays a stream, twice that many slots
    assert plan(lib, **dict(TWO, specOn=1, specPool=1000)).specCap == 1000
    assert plan(lib, **dict(TWO, specOn=1, specPool=1 << 30)).specCap == 1 << 24
    assert plan(lib, **dict(TILE, specOn=1, nRays=1 << 20)).specCap == 2 << 20     # COUNT pre-pass: one pool for the batch


def test_coalescer_piece_uses_the_same_stride(lib):
    """run_batch (pvol_li_coalesce.hip) cuts a batch so that 64 slots a call stay within the 4 GB record budget."""
    assert lib.pvol_li_piece(100, 0, 4096) == 4096            # 128-byte slots: half a million calls would fit
    assert lib.pvol_li_piece(11968, 1, 4096) == (4 << 30) // ((16 + 11968 + 8 * 11968) * 64) < 4096   # the longest step plan of a VolumeGrid
    assert lib.pvol_li_piece(11968, 0, 4096) == 4096
    assert lib.pvol_li_piece(100, 1, 0) == 1
