"""Volume "exponential" (the reference's volumes/exponential.{h,cpp}) on the host side: the scene-file front end, the ctypes
packing of kind 4, the library's argument check and the batch plan.  No GPU."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, abi, load_scene
from test_launch_plan import GRID1, ROWS, TWO, BatchPlan, plan

ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
EXPONENTIAL = 4

HEAD = """Film "image" "integer xresolution" [8] "integer yresolution" [8] "string filename" "x.png"
Camera "perspective" "float fov" [40]
WorldBegin
"""


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_plan_batch.argtypes = [C.c_void_p, C.c_void_p]
    L.pvol_plan_batch.restype = None
    L.pvol_rec_stride.argtypes = [C.c_int, C.c_bool]
    L.pvol_rec_stride.restype = C.c_size_t
    L.pvol_li_piece.argtypes = [C.c_int, C.c_int, C.c_uint32]
    L.pvol_li_piece.restype = C.c_uint32
    L.pvol_check_exponential.argtypes = [C.POINTER(abi.Volume), C.POINTER(C.c_float)]
    L.pvol_check_exponential.restype = C.c_int
    L.pvol_exponential_max_density.argtypes = [C.POINTER(abi.Volume), C.POINTER(C.c_float)]
    L.pvol_exponential_max_density.restype = C.c_float
    return L


def _parse(tmp_path, volume_line):
    f = tmp_path / "s.pbrt"
    f.write_text(HEAD + volume_line + "\nWorldEnd\n")
    return ps.load(str(f))


def test_front_end_parses_the_defaults(tmp_path):
    """CreateExponentialVolumeRegion's defaults (exponential.cpp:42-50)."""
    d = _parse(tmp_path, 'Volume "exponential"')
    assert int(d["vol.kind"][0]) == EXPONENTIAL
    np.testing.assert_array_equal(d["vol.exp"], np.array([1, 1], np.float32))
    np.testing.assert_array_equal(d["vol.updir"], np.array([0, 1, 0], np.float32))
    np.testing.assert_array_equal(d["vol.extent"], np.array([0, 0, 0, 1, 1, 1], np.float32))
    np.testing.assert_array_equal(d["vol.dims"], np.zeros(3, np.int32))
    assert float(d["vol.g"][0]) == 0.0 and not d["vol.sigma_a"].any() and not d["vol.sigma_s"].any() and not d["vol.le"].any()
    assert "vol.density" not in d


def test_front_end_parses_every_parameter(tmp_path):
    d = _parse(tmp_path, 'Translate 1 2 3\nVolume "exponential" "color sigma_a" [.1 .1 .1] "color sigma_s" [.3 .3 .3] "float g" [.25] '
                         '"color Le" [.5 .5 .5] "point p0" [-1 -2 -3] "point p1" [4 5 6] "float a" [2.5] "float b" [0.75] "vector updir" [0 0 1]')
    assert int(d["vol.kind"][0]) == EXPONENTIAL
    np.testing.assert_array_equal(d["vol.exp"], np.array([2.5, 0.75], np.float32))
    np.testing.assert_array_equal(d["vol.updir"], np.array([0, 0, 1], np.float32))
    np.testing.assert_array_equal(d["vol.extent"], np.array([-1, -2, -3, 4, 5, 6], np.float32))
    assert float(d["vol.g"][0]) == np.float32(.25)
    # the spectra and the transform go the way every other Volume's do
    h = _parse(tmp_path, 'Translate 1 2 3\nVolume "homogeneous" "color sigma_a" [.1 .1 .1] "color sigma_s" [.3 .3 .3] "color Le" [.5 .5 .5]')
    for k in ("vol.sigma_a", "vol.sigma_s", "vol.le", "vol.w2v", "vol.v2w"):
        np.testing.assert_array_equal(d[k], h[k], err_msg=k)
    assert d["vol.v2w"].reshape(4, 4)[:3, 3].tolist() == [1, 2, 3]


def test_front_end_keeps_a_non_unit_updir_as_given(tmp_path):
    """The scene dictionary carries updir as written; Normalize() is the library's (pvol.h at pvol_volume.density)."""
    d = _parse(tmp_path, 'Volume "exponential" "vector updir" [0 3 4]')
    np.testing.assert_array_equal(d["vol.updir"], np.array([0, 3, 4], np.float32))
    d = ps.load(os.path.join(GOLD, "scenes", "fog_exponential.pbrt"))
    assert int(d["vol.kind"][0]) == EXPONENTIAL
    np.testing.assert_array_equal(d["vol.exp"], np.array([1.4, 0.9], np.float32))
    np.testing.assert_array_equal(d["vol.updir"], np.array([0, 2, 0], np.float32))
    abi.SceneHolder(d)


def _exp_scene(a=1.0, b=0.5, up=(0, 1, 0)):
    s = dict(load_scene("volumescene_grid16"))
    s["vol.kind"] = np.array([EXPONENTIAL], np.int32)
    del s["vol.density"]
    s["vol.exp"] = np.array([a, b], np.float32)
    s["vol.updir"] = np.array(up, np.float32)
    return s


def test_scene_holder_packs_kind_4():
    h = abi.SceneHolder(_exp_scene(0.5, 1.25, (1, 2, 2)))   # the dims of the blob (16^3) must not survive
    v = h.scene.volume
    assert v.kind == EXPONENTIAL == abi.VOLUME_EXPONENTIAL
    assert (v.nx, v.ny, v.nz) == (0, 0, 0)
    assert h.density.dtype == np.float32 and h.density.tolist() == [0.5, 1.25, 1, 2, 2]
    assert [v.density[i] for i in range(5)] == [0.5, 1.25, 1, 2, 2]
    assert C.addressof(v.density.contents) == h.density.ctypes.data   # the holder keeps the array the struct points into


def test_argument_check_of_kind_4(lib):
    """pvol_set_scene's check of {a, b, updir}, through the entry that needs no device (pvol_create fails without one, so
    pvol_set_scene itself cannot be reached there): NULL, non-finite values and a zero-length updir are PVOL_E_INVALID."""
    def check(vals):
        h = abi.SceneHolder(_exp_scene())
        v = h.scene.volume
        up = (C.c_float * 3)()
        if vals is None:
            v.density = None
        else:
            h.density[:] = vals
        return lib.pvol_check_exponential(C.byref(v), up), list(up)
    rc, up = check([1, 0.5, 0, 3, 0])
    assert rc == abi.PVOL_OK and up == [0, 1, 0]
    rc, up = check([1, 0.5, 3, 0, 4])                      # Normalize(): one reciprocal of the length, three products
    inv = np.float32(1) / np.float32(5)
    assert rc == abi.PVOL_OK and up == [float(np.float32(3) * inv), 0, float(np.float32(4) * inv)]
    assert check(None)[0] == abi.PVOL_E_INVALID
    assert check([1, 0.5, 0, 0, 0])[0] == abi.PVOL_E_INVALID
    for i in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            vals = [1, 0.5, 0, 1, 0]
            vals[i] = bad
            assert check(vals)[0] == abi.PVOL_E_INVALID, (i, bad)
    assert check([0, 0, 1e-30, 0, 0])[0] == abi.PVOL_E_INVALID   # a length that underflows to zero
    assert lib.pvol_check_exponential(None, None) == abi.PVOL_E_INVALID


PLAN_INPUTS = [r[1] for r in ROWS] + [dict(TWO, forceSeq=1), dict(hasTauOut=1), dict(GRID1, hasTauOut=1), dict(GRID1, forceSeq=1),
                                      dict(GRID1, specOn=1), dict(TWO, specOn=1, noLite=1), dict(TWO, specOn=1, roulette=1),
                                      dict(hasInit=1), dict(nStreams=4096, maxRays=1 << 20, nRays=1 << 30), dict(GRID1, noLite=1),
                                      dict(GRID1, roulette=1), dict(TWO, nUsed=500), dict(statsOn=1), dict(g=0.6), dict(noGroup=1)]


@pytest.mark.parametrize("kw", PLAN_INPUTS, ids=[str(i) for i in range(len(PLAN_INPUTS))])
def test_plan_of_kind_4_is_the_plan_of_kind_2(lib, kw):
    """Every input test_launch_plan.py sweeps (its rows, its refusals, its size cases), asked once as a VolumeGrid and once as an
    exponential medium through the same entry (pvol_plan_batch): the two plans are equal field by field."""
    kw = {k: v for k, v in kw.items() if k != "volKind"}
    a, b = plan(lib, volKind=2, **kw), plan(lib, volKind=EXPONENTIAL, **kw)
    for name, _ in BatchPlan._fields_:
        assert getattr(a, name) == getattr(b, name), name
    if not kw:
        assert (a.rc, a.path, a.groupForm, a.recStride) == (abi.PVOL_OK, 1, 2, 928)   # row 26: SLICED, the density-region form


def test_record_stride_and_piece_of_kind_4(lib):
    assert plan(lib, volKind=EXPONENTIAL).recStride == plan(lib, volKind=2).recStride == lib.pvol_rec_stride(100, True) == 928
    # the coalescer cuts a batch by the same stride: the `grid` argument is "a density region" (pvol_li_coalesce.hip)
    assert lib.pvol_li_piece(11968, 1, 4096) == (4 << 30) // ((16 + 11968 + 8 * 11968) * 64) < 4096 == lib.pvol_li_piece(11968, 0, 4096)


def _max_density(lib, a, b, up, extent):
    s = _exp_scene(a, b, up)
    s["vol.extent"] = np.array(extent, np.float32)
    h = abi.SceneHolder(s)
    n = (C.c_float * 3)()
    assert lib.pvol_check_exponential(C.byref(h.scene.volume), n) == abi.PVOL_OK
    return float(lib.pvol_exponential_max_density(C.byref(h.scene.volume), n)), np.array(list(n), np.float64)


@pytest.mark.parametrize("a,b,up", [(1.0, 1.5, (0, 1, 0)), (2.0, 0.5, (1, 1, 0)), (1.0, -0.7, (0, 1, 0)), (0.5, -0.3, (1, -2, 0.5)), (3.0, 0.0, (0, 0, 1)),
                                    (1.0, 1.0, (0, -1, 0))])
def test_max_density_is_the_maximum_over_the_extent(lib, a, b, up):
    """What feeds the "can one step reach the roulette" bound: never below the density anywhere in the extent (sampled densely, in
    float64), and attained -- b < 0 and a updir that points down put it at a far corner, an oblique updir at a corner off the axes."""
    extent = (-1.0, 0.5, 2.0, 3.0, 2.5, 2.75)
    md, n = _max_density(lib, a, b, up, extent)
    g = [np.linspace(extent[i], extent[i + 3], 9) for i in range(3)]
    pts = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    dens = a * np.exp(-b * ((pts - np.array(extent[:3])) @ n))
    assert md >= dens.max() * (1 - 1e-6)
    assert md <= dens.max() * (1 + 1e-6)   # the lattice holds the corners


def test_a_density_that_overflows_is_reported(lib):
    md, _ = _max_density(lib, 1.0, -60.0, (0, 1, 0), (0, 0, 0, 1, 2, 1))   # e^120 is beyond fp32: pvol_set_scene answers PVOL_E_INVALID
    assert md == np.inf


def test_every_kernel_and_launcher_of_the_second_compilation_is_renamed():
    """pvol_region_exp.h renames by a list.  A template kernel left off it would share one host stub between the two compilations and
    a scene could launch the other region's code without a word, so every __global__ function and every extern "C" definition of
    the sources compiled twice must be on the list."""
    import re
    csrc = os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")
    listed = set(re.findall(r"^#define (\w+) \1_exp$", open(os.path.join(csrc, "pvol_region_exp.h")).read(), re.M))
    seen, todo, found = set(), ["pvol_march.hip", "pvol_shoot.hip"], set()
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(os.path.join(csrc, f)):
            continue
        seen.add(f)
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
        todo += re.findall(r'#include "([^"/]+)"', text)
        found |= set(re.findall(r"__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?void\s+(\w+)\s*\(", text))
        found |= set(re.findall(r'^extern "C"[^;{(]*?(\w+)\s*\([^;{]*\)\s*\{', text, re.M))
    assert {"li_seq_kernel", "li_group_kernel", "tile_mw_kernel", "shoot_kernel", "pvol_launch_tile", "pvol_launch_shoot"} <= found
    assert found - listed == set(), sorted(found - listed)


def test_abi_version_is_still_3(lib):
    assert lib.pvol_abi_version() == 3
