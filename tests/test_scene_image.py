"""The scene's device image (pvol_scene_image in csrc/pvol_scene_host.hip, exported for the tests as pvol_check_scene next to
pvol_plan_batch): the status pvol_set_scene gives a scene, decided by pure host code.  Every golden scene is accepted; every
status path is reached by one mutation of volumescene_h; a scene with two faults answers with the earlier check.  No GPU."""
import ctypes as C
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, abi, blob, load_scene

ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
OK, INVALID, UNSUPPORTED, LIMIT = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_UNSUPPORTED, abi.PVOL_E_LIMIT


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_check_scene.argtypes = [C.POINTER(abi.Params), C.POINTER(abi.Scene)]
    L.pvol_check_scene.restype = C.c_int
    return L


def _golden_scenes():
    """Every scene of tests/golden: the blobs the reference wrote and the scene files the front end parses."""
    out = [(os.path.basename(f), f) for f in sorted(glob.glob(os.path.join(GOLD, "scene_*.bin")))]
    for d in ("scenes", "projectScene"):
        out += [(d + "/" + os.path.basename(f), f) for f in sorted(glob.glob(os.path.join(GOLD, d, "*.pbrt")))]
    return [(n, f) for n, f in out if n != "scenes/wedge.pbrt"]   # an Include of pinkfloyd_equiv.pbrt (its prism), no scene of its own


# the two scene files the front end itself refuses by name (an image-map texture, test_pbrt_scene.py) never become a pvol_scene
TEXTURED = {"projectScene/rainbow_png.pbrt", "projectScene/rainbow2_png.pbrt"}


def test_the_golden_set_is_the_one_the_suite_loads():
    names = [n for n, _ in _golden_scenes()]
    assert len([n for n in names if n.endswith(".bin")]) == 13 and len(names) == 13 + 4 + 10   # 13: with the hit zoos spherezoo, trizoo, trizoo_h and sphereroom_kr


@pytest.mark.parametrize("name,path", _golden_scenes(), ids=[n for n, _ in _golden_scenes()])
def test_every_golden_scene_is_accepted_with_its_own_params(lib, name, path):
    if name in TEXTURED:
        with pytest.raises(ps.Unsupported):
            ps.load(path)
        return
    s = blob.load(path) if path.endswith(".bin") else ps.load(path)
    h = abi.SceneHolder(s)
    p = abi.params_from_blob(s)
    assert lib.pvol_check_scene(C.byref(p), C.byref(h.scene)) == OK


# ---- mutations of volumescene_h: each takes the blob (a dict of arrays), returns (blob, edit of the packed scene, edit of the params)
def _vh():
    return {k: np.array(v) for k, v in load_scene("volumescene_h").items()}


def _with(**arrays):
    def f(s):
        s.update({k.replace("__", "."): np.asarray(v) for k, v in arrays.items()})
    return f


def _grid(s):
    s["vol.kind"] = np.array([abi.VOLUME_GRID], np.int32)
    s["vol.dims"] = np.array([2, 2, 2], np.int32)
    s["vol.density"] = np.ones(8, np.float32)


def _exponential(vals):
    def f(s):
        s["vol.kind"] = np.array([abi.VOLUME_EXPONENTIAL], np.int32)
        s["vol.exp"] = np.array(vals[:2], np.float32)
        s["vol.updir"] = np.array(vals[2:], np.float32)
        s["vol.extent"] = np.array([0, 0, 0, 1, 2, 1], np.float32)
    return f


def _spheres(radius=1.0, material=0):
    def f(s):
        sp = load_scene("sphereroom")
        for k in ("o2w", "w2o", "f", "flip"):
            s["spheres." + k] = np.array(sp["spheres." + k])
        n = len(sp["spheres.material"])
        s["spheres.f"][0] = radius
        s["spheres.material"] = np.full(n, material, np.int32)
    return f


def _tris65(nan=False):
    def f(s):
        p = np.tile(s["tris.p"].reshape(-1, 9), (11, 1))[:65].astype(np.float32)
        if nan:
            p[40, 4] = np.nan
        s["tris.p"] = p.reshape(-1)
        s["tris.material"] = np.zeros(65, np.int32)
        s["tris.flip"] = np.zeros(65, np.int32)
    return f


def _set(**fields):
    def f(scene):
        for k, v in fields.items():
            setattr(scene, k, v)
    return f


def _volume(**fields):
    def f(scene):
        for k, v in fields.items():
            setattr(scene.volume, k, v)
    return f


def _all(*fs):
    def f(x):
        for g in fs:
            g(x)
    return f


def _null(t):
    return C.POINTER(t)()


def _status(lib, blob_edit=None, scene_edit=None, **params):
    s = _vh()
    if blob_edit:
        blob_edit(s)
    h = abi.SceneHolder(s)
    if scene_edit:
        scene_edit(h.scene)
    p = abi.params_from_blob(s, **params)
    return lib.pvol_check_scene(C.byref(p), C.byref(h.scene))


def _kind(k):
    return _with(vol__kind=np.array([k], np.int32))


BAD_LIGHT = _with(lights__kind=np.array([5], np.int32))
NO_LIGHTS = _set(lights=_null(abi.Light))
TINY_STEP = dict(step_size=1e-6)

# (id, expected status, blob edit, packed-scene edit, params), in the order of the checks
ONE_FAULT = [
    ("unknown_volume_kind", UNSUPPORTED, _kind(7), None, {}),
    ("nine_lights", UNSUPPORTED, None, _set(n_lights=9), {}),
    ("too_many_triangles", UNSUPPORTED, None, _set(n_triangles=(1 << 24) + 1), {}),
    ("null_lights", INVALID, None, NO_LIGHTS, {}),
    ("null_triangles", INVALID, None, _set(triangles=_null(abi.Triangle)), {}),
    ("nine_spheres", UNSUPPORTED, None, _set(n_spheres=9), {}),
    ("null_spheres", INVALID, None, _set(n_spheres=1, spheres=_null(abi.Sphere)), {}),
    ("sphere_radius_0", INVALID, _spheres(radius=0.0), None, {}),
    ("sphere_material_out_of_range", INVALID, _spheres(material=1), None, {}),
    ("sphere_material_negative", INVALID, _spheres(material=-1), None, {}),
    ("grid_nx_0", INVALID, _grid, _volume(nx=0), {}),
    ("grid_null_density", INVALID, _grid, _volume(density=_null(C.c_float)), {}),
    ("exponential_zero_updir", INVALID, _exponential([1, 0, 0, 0, 0]), None, {}),
    ("exponential_nan_a", INVALID, _exponential([np.nan, 0, 0, 1, 0]), None, {}),
    ("exponential_inf_b", INVALID, _exponential([1, np.inf, 0, 1, 0]), None, {}),
    ("exponential_null", INVALID, _exponential([1, 0.5, 0, 1, 0]), _volume(density=_null(C.c_float)), {}),
    ("exponential_overflow", INVALID, _exponential([1, -60, 0, 1, 0]), None, {}),   # e^120 at the top of the extent
    ("light_of_unknown_kind", UNSUPPORTED, BAD_LIGHT, None, {}),
    ("step_bound_past_12000", LIMIT, None, None, TINY_STEP),
    ("nine_materials", UNSUPPORTED, None, _set(n_materials=9), {}),
    ("null_materials", INVALID, None, _set(materials=_null(abi.Material)), {}),
    ("material_of_unknown_kind", UNSUPPORTED, _with(mats__kind=np.array([5], np.int32)), None, {}),
    ("triangle_material_out_of_range", INVALID, _with(tris__material=np.array([0, 0, 9, 0, 0, 0], np.int32)), None, {}),
    ("nan_vertex_in_65_triangles", INVALID, _tris65(nan=True), None, {}),
]
# the earlier check wins; the first two are the issue's, the others pair two different statuses
TWO_FAULTS = [
    ("volume_kind_before_light_count", UNSUPPORTED, _kind(7), _set(n_lights=9), {}),
    ("null_lights_before_bad_sphere", INVALID, _spheres(radius=0.0), NO_LIGHTS, {}),
    ("null_lights_before_sphere_count", INVALID, None, _all(NO_LIGHTS, _set(n_spheres=9)), {}),
    ("sphere_count_before_grid_dims", UNSUPPORTED, _grid, _all(_set(n_spheres=9), _volume(nx=0)), {}),
    ("exponential_before_light_kind", INVALID, _all(_exponential([1, 0, 0, 0, 0]), BAD_LIGHT), None, {}),
    ("light_kind_before_step_bound", UNSUPPORTED, BAD_LIGHT, None, TINY_STEP),
    ("step_bound_before_materials", LIMIT, None, _set(n_materials=9), TINY_STEP),
    ("material_kind_before_nan_vertex", UNSUPPORTED, _all(_tris65(nan=True), _with(mats__kind=np.array([5], np.int32))), None, {}),
]


def test_the_mutated_scene_is_accepted_unmutated(lib):
    assert len(load_scene("volumescene_h")["mats.kind"]) == 1 and len(load_scene("volumescene_h")["tris.material"]) == 6
    assert _status(lib) == OK
    for edit in (_grid, _exponential([1, 0.5, 0, 3, 0]), _spheres(), _tris65()):   # the carriers of the mutations below, without the fault
        assert _status(lib, edit) == OK


@pytest.mark.parametrize("want,blob_edit,scene_edit,params", [c[1:] for c in ONE_FAULT], ids=[c[0] for c in ONE_FAULT])
def test_one_mutation_per_status_path(lib, want, blob_edit, scene_edit, params):
    assert _status(lib, blob_edit, scene_edit, **params) == want


@pytest.mark.parametrize("want,blob_edit,scene_edit,params", [c[1:] for c in TWO_FAULTS], ids=[c[0] for c in TWO_FAULTS])
def test_two_faults_answer_with_the_earlier_check(lib, want, blob_edit, scene_edit, params):
    assert _status(lib, blob_edit, scene_edit, **params) == want


def test_null_arguments(lib):
    s = load_scene("volumescene_h")
    h, p = abi.SceneHolder(s), abi.params_from_blob(s)
    assert lib.pvol_check_scene(None, C.byref(h.scene)) == INVALID
    assert lib.pvol_check_scene(C.byref(p), None) == INVALID
    assert "pvol_check_scene" not in open(os.path.join(ROOT, "include", "pvol.h")).read()   # a test entry like pvol_plan_batch, not ABI
