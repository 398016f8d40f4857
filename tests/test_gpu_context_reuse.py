"""One context driven through a sequence of scenes and photon maps: whatever pvol_set_scene, pvol_upload_photons and
pvol_set_surface_integrator keep, replace or free between the steps, every step must give what a fresh context set up for that step
alone gives, and a rejected scene must change nothing.  The contexts are created under PVOL_NO_GROUP=1: that path has no float
atomics, so the comparison is bit for bit (spectral output, draw counts, stream end positions, transmittance)."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLD, abi, blob, load_li_case, load_photons

pytestmark = pytest.mark.gpu


def _results(pv, rays, streams):
    st = streams.copy()
    out, draws = pv.li(rays, st)
    st2 = streams.copy()
    return out, draws, st["end_draw"].copy(), pv.transmittance(rays, st2), st2["end_draw"].copy()


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_scene_map_and_integrator_changes_on_one_context(monkeypatch):
    from test_gpu_bvh import _edge_scene
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert pvol.lib().pvol_device_count() >= 1
    monkeypatch.setenv("PVOL_NO_GROUP", "1")
    grid, p, grid_rays, grid_streams, _ = load_li_case("grid16")
    _, p_mesh, mesh_rays, mesh_streams, _ = load_li_case("mesh")
    assert bytes(p) == bytes(p_mesh)   # one set of parameters serves every context of the sequence
    big, n_tris = _edge_scene("just_over")
    assert n_tris == 65   # the smallest scene that takes the hierarchy
    cb = blob.load(os.path.join(GOLD, "caustic_vh.bin"))
    caustic = (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30))

    def step_grid(pv):
        pv.set_scene(abi.SceneHolder(grid))
        pv.upload_photons(*load_photons("grid16"))
        assert pv.accel_info()[0] == 0
        return _results(pv, grid_rays, grid_streams)

    def step_big(pv):
        pv.set_scene(abi.SceneHolder(big))
        pv.upload_photons(*load_photons("mesh"))
        pv.set_surface_integrator(50, 0.1, 5, False, caustic, int(cb["n_paths"][0]))
        assert pv.accel_info()[0] == n_tris
        return _results(pv, mesh_rays, mesh_streams)

    fresh = []
    for step in (step_grid, step_big):
        pv = pvol.PhotonVolume(p)
        try:
            fresh.append(step(pv))
        finally:
            pv.close()
    assert np.abs(fresh[0][0][:, :30]).sum() > 0 and np.abs(fresh[1][0][:, :30]).sum() > 0
    assert (fresh[0][3] < 1).any() and (fresh[1][3] < 1).any()

    pv = pvol.PhotonVolume(p)
    try:
        _same(step_grid(pv), fresh[0])                                    # 1
        _same(step_big(pv), fresh[1])                                     # 2
        nan = dict(big)                                                   # 3: rejected by the last check of all, then by the first
        nan["tris.p"] = big["tris.p"].copy()
        nan["tris.p"][9 * 40 + 4] = np.nan
        unknown = dict(grid)
        unknown["vol.kind"] = np.array([7], np.int32)
        for bad, status in ((nan, abi.PVOL_E_INVALID), (unknown, abi.PVOL_E_UNSUPPORTED)):
            with pytest.raises(pvol.PvolError) as e:
                pv.set_scene(abi.SceneHolder(bad))
            assert e.value.status == status
        assert pv.accel_info()[0] == n_tris and pv.photon_count() == len(load_photons("mesh")[0])
        _same(_results(pv, mesh_rays, mesh_streams), fresh[1])
        pv.upload_photons(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 30), np.float32))   # 4
        assert pv.photon_count() == 0
        _same(step_grid(pv), fresh[0])                                    # 5
    finally:
        pv.close()
