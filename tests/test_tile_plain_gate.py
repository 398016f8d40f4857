"""The gate of the tile pre-pass's PLAIN form (pvol_tile_plain_gate, pvol_api.hip beside plan_path): PLAIN exactly for a
COUNT-mode batch over a homogeneous extent lit by a distant first light, whose triangles fit the LDS rows, without hierarchy, spheres,
surface integrator or specular link -- and the general form as soon as any one of these is flipped, or PVOL_TILE_GENERAL=1 is set.
The inputs are derived from the committed scenes the way the host derives them, the batch's mode comes from the plan itself
(pvol_plan_batch).  Pure host code: needs no GPU."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, load_scene

from test_moment_plan import BatchPlan, Knobs, PlanIn

NONE, HOMOGENEOUS, GRID, RAINBOW, EXPONENTIAL = 0, 1, 2, 3, 4   # pvol.h: pvol_volume_kind
POINT, SPOT, DISTANT = 0, 1, 2                                  # pvol.h: pvol_light_kind
TILE_NONE, TILE_COUNT, TILE_GRID_COUNT, TILE_FUSED = 0, 1, 2, 3  # pvol_host.h: BatchPlan::tile
MAX_TRIS = 64                                                   # pvol_dev.h: PVOL_MAX_TRIS, triangles (and shadow rows) the LDS plan holds
GENERAL, PLAIN = 0, 1


class TilePlainIn(C.Structure):   # pvol_host.h
    _fields_ = [("tile", C.c_int32), ("volKind", C.c_int32), ("nLights", C.c_int32), ("light0Kind", C.c_int32), ("hasBvh", C.c_int32),
                ("nSpheres", C.c_int32), ("nTris", C.c_int32), ("surfOn", C.c_int32), ("specLink", C.c_int32), ("tileGeneral", C.c_int32)]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_tile_plain_gate.argtypes = [C.POINTER(TilePlainIn)]
    L.pvol_tile_plain_gate.restype = C.c_int
    L.pvol_plan_batch.argtypes = [C.POINTER(PlanIn), C.POINTER(BatchPlan)]
    L.pvol_plan_batch.restype = None
    return L


def tile_mode(lib, vol_kind, n_lights, distant):
    """BatchPlan::tile of a render batch (hasTile) over such a scene, from the plan."""
    i = PlanIn(nLights=n_lights, volKind=vol_kind, g=0.0, nPhotons=100000, nUsed=50, candCap=256, maxSteps=100, nTris=0, roulette=0,
               distant=int(distant), nCU=256, groupWavesPerCU=12, fixWavesPerCU=16, nRays=4000, nStreams=4, maxRays=1000, hasTile=1, spp=4,
               momentTerms=3, outXYZ=1)
    i.knobs = Knobs(groupGuess=1.15)
    out = BatchPlan()
    lib.pvol_plan_batch(C.byref(i), C.byref(out))
    assert out.rc == 0
    return out.tile


def scene_inputs(lib, name, surf_on=0, spec_link=0):
    """What pvol_launch_batch hands the gate for a committed scene: more than PVOL_MAX_TRIS triangles live in the hierarchy (nTris 0)."""
    s = load_scene(name)
    kinds = [int(k) for k in s["lights.kind"]]
    nt = len(s["tris.material"])
    ns = len(s["spheres.material"]) if "spheres.material" in s else 0
    vol = int(s["vol.kind"][0])
    return dict(tile=tile_mode(lib, vol, len(kinds), bool(kinds) and kinds[0] == DISTANT), volKind=vol, nLights=len(kinds),
                light0Kind=kinds[0] if kinds else -1, hasBvh=int(nt > MAX_TRIS), nSpheres=ns, nTris=nt if nt <= MAX_TRIS else 0,
                surfOn=surf_on, specLink=spec_link, tileGeneral=0)


def gate(lib, v):
    return lib.pvol_tile_plain_gate(C.byref(TilePlainIn(**v)))


@pytest.fixture(scope="module")
def flagship(lib):
    v = scene_inputs(lib, "volumescene_h")
    assert v == dict(v, tile=TILE_COUNT, volKind=HOMOGENEOUS, nLights=1, light0Kind=DISTANT, hasBvh=0, nSpheres=0)
    assert 0 < v["nTris"] <= MAX_TRIS
    return v


def test_struct_size(lib):
    assert C.sizeof(TilePlainIn) == 40          # pvol_host.h's static_assert
    assert C.sizeof(PlanIn) == 152 and C.sizeof(BatchPlan) == 136   # the gate's inputs took no room in either


def test_flagship_scene_takes_plain(lib, flagship):
    assert gate(lib, flagship) == PLAIN


@pytest.mark.parametrize("flip", [
    dict(hasBvh=1, nTris=0),                    # a hierarchy: the triangles are not in LDS
    dict(nSpheres=1),                           # one sphere
    dict(surfOn=1),                             # surface integrator on
    dict(specLink=1),                           # the specular recursion's link table is written
    dict(volKind=GRID), dict(volKind=EXPONENTIAL),   # a density region, either kind (the mode becomes GRID_COUNT as well: see below)
    dict(volKind=NONE),                         # no medium
    dict(light0Kind=POINT), dict(light0Kind=SPOT),   # light 0 is not a distant one: no shadow rows
    dict(nLights=0, light0Kind=-1),             # no light: the general form's early return needs no rows
    dict(nTris=MAX_TRIS + 1),                   # more triangles than the rows hold
    dict(tile=TILE_FUSED), dict(tile=TILE_GRID_COUNT), dict(tile=TILE_NONE),   # not COUNT mode
    dict(tileGeneral=1),                        # PVOL_TILE_GENERAL=1
], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_any_one_flip_takes_the_general_form(lib, flagship, flip):
    assert gate(lib, dict(flagship, **flip)) == GENERAL


def test_what_does_not_enter_the_gate(lib, flagship):
    assert gate(lib, dict(flagship, nTris=0)) == PLAIN                  # an empty scene: zero rows fit
    assert gate(lib, dict(flagship, nTris=MAX_TRIS)) == PLAIN           # the last count that fits
    assert gate(lib, dict(flagship, volKind=RAINBOW)) == PLAIN          # a homogeneous extent with another phase function
    assert gate(lib, dict(flagship, nLights=1)) == PLAIN


def test_modes_from_the_plan(lib, flagship):
    """FUSED is what the plan gives a scene with more than one light, GRID_COUNT a density region: neither is COUNT, so neither is PLAIN."""
    assert tile_mode(lib, HOMOGENEOUS, 1, True) == TILE_COUNT
    assert tile_mode(lib, HOMOGENEOUS, 2, True) == TILE_FUSED
    assert gate(lib, dict(flagship, nLights=2, tile=tile_mode(lib, HOMOGENEOUS, 2, True))) == GENERAL
    for kind in (GRID, EXPONENTIAL):
        assert tile_mode(lib, kind, 1, True) == TILE_GRID_COUNT
        assert gate(lib, dict(flagship, volKind=kind, tile=TILE_GRID_COUNT)) == GENERAL


@pytest.mark.parametrize("name,why", [("meshroom", "hasBvh"), ("sphereroom", "nSpheres"), ("pinkfloyd", "nLights")])
def test_committed_scenes_that_keep_the_general_form(lib, name, why):
    v = scene_inputs(lib, name)
    assert gate(lib, v) == GENERAL
    assert {"hasBvh": v["hasBvh"] == 1, "nSpheres": v["nSpheres"] > 0, "nLights": v["nLights"] > 1 and v["tile"] == TILE_FUSED}[why]
