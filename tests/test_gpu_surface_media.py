"""The surface integrator in front of the media li_group_kernel does not cover: a rainbow medium, Henyey-Greenstein scattering,
any nused, no photon map, several lights, a medium dense enough for the Russian roulette, no volume at all.  There the
wave-per-ray kernels (li_par_kernel, li_seq_kernel, li_replay_kernel) report every camera sample's *T -- the last march step's
Tr, doubled by a roulette survival, zero after a kill -- and surface_kernel composes T * Ls + Lvi (samplerrenderer.cpp:95-97).
Against the oracle's SamplerRendererTask loop with PhotonIntegrator in place, and against the reference's own records.
Bars as in test_gpu_render.py: draws exact; Ls, T * Ls + Lvi within 1e-4 per sample; T.y and the film allclose."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD, abi, blob, load_photons, load_render_case, load_scene

pytestmark = pytest.mark.gpu

LIGHT_KEYS = ("lights.kind", "lights.pos", "lights.dir", "lights.l2w", "lights.w2l", "lights.intensity", "lights.cos")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _pvol():
    import importlib
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _caustic():
    cb = blob.load(os.path.join(GOLD, "caustic_vh.bin"))
    return (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), int(cb["n_paths"][0])


def _render_surface(torch, pv, cam, film, smp, tasks, n):
    dev = torch.device("cuda:0")
    pixels = torch.zeros((film.y_resolution, film.x_resolution, 4), dtype=torch.float32, device=dev)
    rays = torch.zeros((max(n, 1), 48), dtype=torch.uint8, device=dev)
    xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    xyz = torch.zeros((max(n, 1), 4), dtype=torch.float32, device=dev)
    sxyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    streams = torch.zeros((len(tasks), 32), dtype=torch.uint8, device=dev)
    dbg = abi.RenderDebug(rays.data_ptr(), xy.data_ptr(), xyz.data_ptr(), streams.data_ptr(), sxyz.data_ptr())
    pv.render_tasks(cam, film, smp, tasks, pixels.data_ptr(), dbg)
    torch.cuda.synchronize()
    pv.check_errors()
    return {"pixels": pixels.cpu().numpy(), "rays": rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)[:n], "xy": xy.cpu().numpy()[:n],
            "xyzT": xyz.cpu().numpy()[:n], "surf_xyz": sxyz.cpu().numpy()[:n], "streams": streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)}


def _rel_l2(got, ref):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-4 * scale)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _two_lights(s):
    """A second distant light from another direction: the stream-sequential draws of the light choice (FUSED pre-pass + replay)."""
    s = dict(s)
    for k in LIGHT_KEYS:
        s[k] = np.concatenate([s[k], s[k]])
    d = np.array([0.3, 0.4, -0.866], np.float32)
    s["lights.dir"][3:] = d / np.linalg.norm(d)
    return s


def _dense(s, k):
    s = dict(s)
    s["vol.sigma_a"] = s["vol.sigma_a"] * np.float32(k)
    s["vol.sigma_s"] = s["vol.sigma_s"] * np.float32(k)
    return s


def _no_volume(s):
    s = dict(s)
    s["vol.kind"] = np.array([abi.VOLUME_NONE], s["vol.kind"].dtype)
    return s


def _vs_oracle(torch, orc, s, n_used, photons, kernel, step_size=None, env=None):
    """The vh_surf frame (camera, film, sampler, tasks) over scene `s`: device vs oracle.  Returns the oracle's records."""
    pvol = _pvol()
    _, p0, cam, film, smp, c = load_render_case("vh_surf")
    p = abi.params_from_blob(s, step_size=step_size or p0.step_size, max_dist=p0.max_dist, n_used=n_used)
    caustic, n_paths = _caustic()
    holder = abi.SceneHolder(s)
    o = orc.Oracle(holder, p)
    if photons:
        o.set_photons(*load_photons(photons))
    o.set_surface_integrator(50, 0.15, False, caustic, n_paths)
    ro = orc.render_tasks(o, cam, film, smp, c["tasks"])
    o.close()
    assert not ro["unsupported_hits"]
    pv = _with_env(env or {}, lambda: pvol.PhotonVolume(p))
    try:
        pv.set_scene(holder)
        if photons:
            pv.upload_photons(*load_photons(photons))
        pv.set_surface_integrator(50, 0.15, 5, False, caustic, n_paths)
        r = _render_surface(torch, pv, cam, film, smp, c["tasks"], ro["n_samples"])
        assert pv.march_kernel_name() == kernel
    finally:
        pv.close()
    np.testing.assert_array_equal(r["rays"]["rng_skip"], ro["rays"]["rng_skip"])
    np.testing.assert_array_equal(r["streams"]["end_draw"], ro["end_draws"])
    ref_s = ro["surf_xyz"].reshape(-1, 3)
    assert (ref_s.sum(1) > 0).mean() > 0.5                       # the walls are in view and lit
    err = _rel_l2(r["surf_xyz"], ref_s)
    assert err.max() <= 1e-4, "surface Li per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    ref = ro["xyzT"].reshape(-1, 4)
    err = _rel_l2(r["xyzT"][:, :3], ref[:, :3])
    assert err.max() <= 1e-4, "T * Ls + Lvi per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    np.testing.assert_allclose(r["xyzT"][:, 3], ref[:, 3], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r["pixels"], ro["pixels"].reshape(r["pixels"].shape), rtol=1e-4, atol=1e-5 * np.abs(ro["pixels"]).max())
    return ro


def test_rainbow_medium_one_light(torch_cuda, orc):
    """projectScene/volumescene_png.pbrt's medium: RainbowVolume (no photon lookups), one distant light, li_par_kernel."""
    _vs_oracle(torch_cuda, orc, load_scene("volumescene_rainbow"), 50, None, "li_par_kernel")


def test_henyey_greenstein_medium(torch_cuda, orc):
    _vs_oracle(torch_cuda, orc, load_scene("volumescene_hg"), 50, "vhg", "li_par_kernel")


@pytest.mark.parametrize("n_used,photons", [(300, "vh"), (5, "vh"), (50, None)])
def test_homogeneous_medium_beyond_the_group_kernel(torch_cuda, orc, n_used, photons):
    """nused 300 (projectScene/darkside.pbrt's), nused below 10, and no photon map at all."""
    _vs_oracle(torch_cuda, orc, load_scene("volumescene_h"), n_used, photons, "li_par_kernel")


@pytest.mark.parametrize("scene,photons", [("volumescene_hg", "vhg"), ("volumescene_rainbow", None)])
def test_two_lights_replay_path(torch_cuda, orc, scene, photons):
    _vs_oracle(torch_cuda, orc, _two_lights(load_scene(scene)), 50, photons, "li_replay_kernel")


def test_dense_medium_russian_roulette(torch_cuda, orc):
    """sigma_t x stepsize near 9: most march steps roll the roulette.  A killed ray leaves T = 0, a survivor of its last step
    T = 2 Tr; the doubled samples carry a surface share that a missing factor 2 would put far outside the bar."""
    ro = _vs_oracle(torch_cuda, orc, _dense(load_scene("volumescene_h"), 60), 50, "vh", "li_replay_kernel", step_size=1.0)
    ty = ro["xyzT"].reshape(-1, 4)[:, 3]
    killed = ty == 0
    doubled = (ty > 0) & (ty < 1e-3)    # Tr.y() < 1e-3 is only left behind by the roulette, divided by .5
    assert killed.sum() > 100 and doubled.sum() > 20
    share = ty * np.linalg.norm(ro["surf_xyz"].reshape(-1, 3), axis=1) / np.maximum(np.linalg.norm(ro["xyzT"].reshape(-1, 4)[:, :3], axis=1), 1e-30)
    assert (share[doubled] > 1e-2).sum() > 10


def test_no_volume(torch_cuda, orc):
    _vs_oracle(torch_cuda, orc, _no_volume(load_scene("volumescene_h")), 50, None, "li_par_kernel")


@pytest.mark.parametrize("env,kernel", [({"PVOL_NO_GROUP": "1"}, "li_par_kernel"), ({"PVOL_FORCE_SEQ": "1"}, "li_seq_kernel")])
def test_reference_capture_through_the_wave_per_ray_kernels(torch_cuda, env, kernel):
    """The reference's own PhotonIntegrator + PhotonVolumeIntegrator records of vh_surf, rendered without li_group_kernel."""
    pvol = _pvol()
    s, p, cam, film, smp, c = load_render_case("vh_surf")
    caustic, n_paths = _caustic()
    pv = _with_env(env, lambda: pvol.PhotonVolume(p))
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*load_photons("vh"))
        pv.set_surface_integrator(int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), 5, bool(c["surf.params.i"][1]), caustic, n_paths)
        r = _render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], len(c["samples.time"]))
        assert pv.march_kernel_name() == kernel
    finally:
        pv.close()
    np.testing.assert_array_equal(r["xy"].ravel(), c["samples.image"])
    np.testing.assert_array_equal(r["rays"]["maxt"], c["rays.t"][1::2])
    np.testing.assert_array_equal(r["rays"]["rng_skip"], c["rays.skip"])
    np.testing.assert_array_equal(r["streams"]["end_draw"], c["task.end_draw"])
    err = _rel_l2(r["surf_xyz"], c["surf.xyz"].reshape(-1, 3))
    assert err.max() <= 1e-4, "surface Li per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    ref = c["xyzT"].reshape(-1, 4)
    err = _rel_l2(r["xyzT"][:, :3], ref[:, :3])
    assert err.max() <= 1e-4, "T * Ls + Lvi per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    np.testing.assert_allclose(r["xyzT"][:, 3], ref[:, 3], rtol=1e-4, atol=1e-6)
    refpix = c["film.pixels"].reshape(film.y_resolution, film.x_resolution, 4)
    np.testing.assert_allclose(r["pixels"], refpix, rtol=1e-4, atol=1e-5 * np.abs(refpix).max())


def _render_pbrt():
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    return rp


@pytest.mark.parametrize("fname,caustic", [("scenes/volumescene_equiv.pbrt", None), ("projectScene/darkside.pbrt", 5000)])
def test_scene_files_keep_the_surface_term(torch_cuda, fname, caustic):
    """The rainbow room and darkside.pbrt (homogeneous, spot light, nused 300) as written: the surface term is applied."""
    rp = _render_pbrt()
    f = os.path.join(GOLD, fname)
    notes = []
    kw = dict(xres=48, yres=32, spp=8, photons=20000, shoot_tasks=64, caustic_photons=caustic)
    img, info = rp.render_scene_file(f, log=lambda *a: notes.append(" ".join(str(x) for x in a)), **kw)
    assert info["surface_integrator"], notes
    assert not [m for m in notes if "not applied" in m], notes
    assert img.shape == (32, 48, 3) and np.isfinite(img).all()
    img2, info2 = rp.render_scene_file(f, surface=False, log=lambda *a: None, **kw)
    assert not info2["surface_integrator"] and img.mean() > img2.mean() > 0          # the walls add light
