"""The surface integrator with both maps of its LPhoton calls, without a GPU: every status of
pvol_set_surface_integrator_maps is decided by one pure host function (pvol_check_surface_maps, exported for the tests next to
pvol_check_radiance / pvol_check_scene) in one fixed order, and the fixture scene reaches the front end's blob as written."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT, abi

OK, INVALID, UNSUPPORTED, NO_SCENE = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_UNSUPPORTED, abi.PVOL_E_NO_SCENE
MATTE, GLASS, OTHER = 0, 1, 2   # what the scene's materials allow


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _map(n, seed=1, n_paths=10):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32), rng.random((n, 30)).astype(np.float32), n_paths


def _check(pvol, n_used=50, max_dist=0.1, depth=5, final_gather=0, store=0, have_scene=1, materials=MATTE, kept=0, store_n=(0, 0), store_paths=(0, 0),
           caustic=None, indirect=None, host=1, null_sp=False):
    sp = abi.SurfaceParams()
    sp.n_used, sp.max_dist, sp.max_specular_depth, sp.final_gather, sp.use_preprocess_store = n_used, max_dist, depth, final_gather, store
    sp.n_caustic_paths, sp.n_indirect_photons = 12345, 777   # not read by this entry point
    ca, keep_c = pvol.photon_array(caustic) if not isinstance(caustic, abi.PhotonArray) else (caustic, None)
    ia, keep_i = pvol.photon_array(indirect) if not isinstance(indirect, abi.PhotonArray) else (indirect, None)
    n, paths = (C.c_uint32 * 2)(*store_n), (C.c_uint32 * 2)(*store_paths)
    return pvol.lib().pvol_check_surface_maps(None if null_sp else C.byref(sp), have_scene, materials, kept, n, paths,
                                              C.byref(ca) if ca is not None else None, C.byref(ia) if ia is not None else None, host)


def test_good_calls(pvol):
    assert _check(pvol) == OK                                           # no map at all: the direct term alone
    assert _check(pvol, caustic=_map(20)) == OK
    assert _check(pvol, indirect=_map(20)) == OK                        # the two maps are independent
    assert _check(pvol, caustic=_map(20), indirect=_map(7, 2)) == OK
    assert _check(pvol, materials=GLASS, depth=5, indirect=_map(7)) == OK
    empty = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 30)), 0)
    assert _check(pvol, caustic=empty, indirect=empty) == OK            # n == 0: LPhoton's `if (map && ...)`
    assert _check(pvol, store=1, kept=1, store_n=(0, 0)) == OK          # kept stores may be empty
    assert _check(pvol, store=1, kept=1, store_n=(5, 9), store_paths=(100, 200)) == OK
    assert _check(pvol, max_dist=float("inf")) == OK                    # as pvol_set_surface_integrator: any max_dist > 0


def test_every_status_in_its_order(pvol):
    assert _check(pvol, null_sp=True) == INVALID
    # 1. the parameters
    for kw in ({"n_used": 0}, {"n_used": -4}, {"max_dist": 0.0}, {"max_dist": -1.0}, {"max_dist": float("nan")}, {"depth": -1}):
        assert _check(pvol, **kw) == INVALID
    # 2. the materials, 3. maxspeculardepth with glass
    assert _check(pvol, materials=OTHER) == UNSUPPORTED
    assert _check(pvol, materials=GLASS, depth=6) == UNSUPPORTED
    assert _check(pvol, materials=MATTE, depth=6) == OK                 # without glass the depth only costs draws
    # 4. the scene
    assert _check(pvol, have_scene=0) == NO_SCENE
    # 5. the arrays and the stores
    good = _map(20)
    f32p = C.POINTER(C.c_float)
    full = [x.ctypes.data_as(f32p) for x in good[:3]]
    for which in ("caustic", "indirect"):
        for i in range(3):                                              # n > 0 and a NULL pointer
            pa = abi.PhotonArray(*[None if j == i else full[j] for j in range(3)], 20, 10)
            assert _check(pvol, **{which: pa}) == INVALID
        assert _check(pvol, **{which: good[:3] + (0,)}) == INVALID      # n > 0 with n_paths == 0
        for field in range(3):                                          # a non-finite value
            for v in (np.nan, np.inf, -np.inf):
                bad = [x.copy() for x in good[:3]]
                bad[field][13, 1] = v
                assert _check(pvol, **{which: (bad[0], bad[1], bad[2], 10)}) == INVALID
                assert _check(pvol, host=0, **{which: (bad[0], bad[1], bad[2], 10)}) == OK   # device pointers are not read
        assert _check(pvol, store=1, kept=1, **{which: good}) == INVALID    # use_preprocess_store together with an array
    assert _check(pvol, store=1, kept=0) == INVALID                     # ... or without kept stores
    assert _check(pvol, store=1, kept=1, store_n=(5, 0), store_paths=(0, 0)) == INVALID   # a kept store without its path count
    assert _check(pvol, store=1, kept=1, store_n=(0, 5), store_paths=(7, 0)) == INVALID
    # 6. the final gather
    assert _check(pvol, final_gather=1, indirect=_map(1)) == UNSUPPORTED
    assert _check(pvol, final_gather=1, store=1, kept=1, store_n=(0, 1), store_paths=(0, 9)) == UNSUPPORTED


def test_final_gather_only_matters_with_an_indirect_map(pvol):
    """photonmap.cpp:183: `finalGather && indirectMap != NULL`.  Without a map the flag changes nothing."""
    empty = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 30)), 0)
    assert _check(pvol, final_gather=1) == OK
    assert _check(pvol, final_gather=1, caustic=_map(20)) == OK
    assert _check(pvol, final_gather=1, caustic=_map(20), indirect=empty) == OK
    assert _check(pvol, final_gather=1, store=1, kept=1, store_n=(40, 0), store_paths=(9, 0)) == OK
    assert _check(pvol, final_gather=1, indirect=_map(1)) == UNSUPPORTED
    assert _check(pvol, final_gather=0, indirect=_map(1)) == OK


def test_the_first_fault_answers(pvol):
    """Two faults at once: the earlier check in the stated order gives the status."""
    one = _map(1)
    gather = {"final_gather": 1, "indirect": one}                       # by itself UNSUPPORTED (6)
    assert _check(pvol, n_used=0, **gather) == INVALID                  # 1 before 6
    assert _check(pvol, n_used=0, materials=OTHER) == INVALID           # 1 before 2
    assert _check(pvol, n_used=0, have_scene=0) == INVALID              # 1 before 4
    assert _check(pvol, materials=OTHER, have_scene=0) == UNSUPPORTED   # 2 before 4
    assert _check(pvol, materials=GLASS, depth=6, have_scene=0) == UNSUPPORTED   # 3 before 4
    assert _check(pvol, have_scene=0, caustic=one[:3] + (0,)) == NO_SCENE        # 4 before 5
    assert _check(pvol, have_scene=0, **gather) == NO_SCENE             # 4 before 6
    assert _check(pvol, final_gather=1, indirect=one, caustic=one[:3] + (0,)) == INVALID   # 5 before 6
    assert _check(pvol, final_gather=1, store=1, kept=1, indirect=one) == INVALID          # 5 (store with an array) before 6
    assert _check(pvol, materials=OTHER, **gather) == UNSUPPORTED


def test_entry_point_without_a_context_or_a_device(pvol):
    L = pvol.lib()
    sp = abi.SurfaceParams()
    sp.n_used, sp.max_dist, sp.max_specular_depth = 50, 0.1, 5
    assert L.pvol_set_surface_integrator_maps(None, C.byref(sp), None, None) == INVALID
    assert L.pvol_set_surface_integrator_maps(None, None, None, None) == INVALID
    assert "pvol_set_surface_integrator_maps" in pvol.EXPORTS
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    assert "pvol_check_surface_maps" not in text and "pvol_set_surface_integrator_maps" in text   # a test entry like pvol_check_scene, not ABI
    assert L.pvol_abi_version() == 3
    if L.pvol_device_count() == 0:   # no CPU path: as for every GPU entry, no context exists to call it with
        from conftest import load_scene
        with pytest.raises(pvol.PvolError) as e:
            pvol.PhotonVolume(abi.params_from_blob(load_scene("volumescene_h")))
        assert e.value.status == abi.PVOL_E_NO_DEVICE


def test_surface_params_keep_their_size(pvol, tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "pvol.h"\nint main(){printf("%zu %zu\\n",sizeof(pvol_surface_params),sizeof(pvol_photon_array));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert sizes == [32, C.sizeof(abi.PhotonArray)] and C.sizeof(abi.SurfaceParams) == 32


def test_fixture_scene_reaches_the_blob(pvol):
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    s = ps.load(os.path.join(ROOT, "tests", "golden", "indirect", "room_indirect.pbrt"))
    assert s["surf.name"] == "photonmap"
    assert int(s["surf.params.i"][2]) == 0 and int(s["params.i"][5]) == 0          # finalgather false, integrator and shooter
    assert int(s["params.i"][4]) == 2000 and int(s["params.i"][3]) == 0            # indirectphotons, causticphotons
    assert int(s["surf.params.i"][0]) == 300 and abs(float(s["surf.params.f"][0]) - 0.15) < 1e-7
    p = abi.params_from_blob(s)
    assert (p.n_indirect_photons, p.n_caustic_photons, p.final_gather) == (2000, 0, 0)
    assert int(np.asarray(s["vol.kind"]).ravel()[0]) == abi.VOLUME_HOMOGENEOUS
    # the light's direction has no x component: the wall at x = 5 (normal along x) gets no direct light
    assert float(np.asarray(s["lights.dir"]).reshape(-1, 3)[0, 0]) == 0.0
    kd = np.asarray(s["mats.kd"]).reshape(-1, 30)
    assert kd.min() > 0.3                                                          # grey walls: photons survive the bounces
