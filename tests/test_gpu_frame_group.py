"""pvol_preprocess_group / pvol_render_frame_group: one process drives N contexts, one host thread each.  N contexts on ONE device run
the whole N-way protocol (the in-process all-gather of the sharded shoot, the task deal, the film reduce on context 0's stream), so
every GPU run covers it; with several devices the same calls run across them.

Bars: a group frame equals a single-context render of all tasks (pvol_render_tasks_device + pvol_film_resolve_device) at rtol 2e-5,
atol 1e-6 x max (the film's float atomics add in another order); a group shoot equals pvol_preprocess_blocks on one context bit for
bit, on every context.  Calls that could hang run on a helper thread with a time limit."""
import os
import threading

import numpy as np
import pytest

from conftest import GOLD, RENDER_CASES, RENDER_SPECULAR_CASES, ROOT, abi, blob, load_photons, load_render_case, load_scene

pytestmark = pytest.mark.gpu

CALL_TIMEOUT = 180   # seconds for one group call: they are small; a hang fails the test instead of blocking the suite


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _pvol():
    import importlib
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _within_time(fn, *args, **kw):
    """fn(*args) on a helper thread; its exception is re-raised here, a call that outlasts CALL_TIMEOUT fails the test."""
    out = {}

    def run():
        try:
            out["value"] = fn(*args, **kw)
        except BaseException as e:   # noqa: BLE001 -- handed to the test thread
            out["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(CALL_TIMEOUT)
    if t.is_alive():
        pytest.fail("%s did not return within %d s" % (getattr(fn, "__name__", fn), CALL_TIMEOUT))
    if "error" in out:
        raise out["error"]
    return out.get("value")


def _tag(name):
    return (RENDER_CASES.get(name) or RENDER_SPECULAR_CASES[name])[1]


def _context(name, device, with_scene=True):
    """A context of golden render case `name` on `device`: its own scene, volume photon map and (for the specular cases) caustic map."""
    pvol = _pvol()
    s, p, cam, film, smp, c = load_render_case(name)
    p.device = device
    pv = pvol.PhotonVolume(p)
    if with_scene:
        _give_scene(pv, name, s, c)
    return pv, s, cam, film, smp, c


def _give_scene(pv, name, s, c):
    pv.set_scene(abi.SceneHolder(s))
    pv.upload_photons(*load_photons(_tag(name)))
    if name in RENDER_SPECULAR_CASES:   # the surface integrator with the specular recursion (as test_gpu_render.py sets it up)
        cb = blob.load(os.path.join(GOLD, "caustic_%s.bin" % _tag(name)))
        pv.set_surface_integrator(int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), 5, bool(c["surf.params.i"][1]),
                                  (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), int(cb["n_paths"][0]))


def _single_frame(torch, name):
    """The whole frame (every task of the sampler) on one context of device 0: pixels and resolved RGB."""
    pv, s, cam, film, smp, c = _context(name, 0)
    try:
        dev = torch.device("cuda:0")
        px = torch.zeros((film.y_resolution, film.x_resolution, 4), dtype=torch.float32, device=dev)
        rgb = torch.zeros((film.y_resolution, film.x_resolution, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pv.render_tasks(cam, film, smp, np.arange(smp.n_tasks, dtype=np.uint32), px.data_ptr())
        pv.film_resolve(film, px.data_ptr(), rgb.data_ptr())
        torch.cuda.synchronize()
        pv.check_errors()
        return px.cpu().numpy(), rgb.cpu().numpy()
    finally:
        pv.close()


def _group_buffers(torch, film, devices):
    """Films filled with garbage (the call zeroes them), an RGB target on the first device, one stream per context."""
    px = [torch.full((film.y_resolution, film.x_resolution, 4), 7.0, dtype=torch.float32, device="cuda:%d" % d) for d in devices]
    rgb = torch.full((film.y_resolution, film.x_resolution, 3), -1.0, dtype=torch.float32, device="cuda:%d" % devices[0])
    streams = [torch.cuda.Stream(device="cuda:%d" % d) for d in devices]
    for d in sorted(set(devices)):
        torch.cuda.synchronize(d)
    return px, rgb, streams


def _group_frame(torch, pvs, cam, film, smp, devices):
    pvol = _pvol()
    px, rgb, streams = _group_buffers(torch, film, devices)
    _within_time(pvol.render_frame_group, pvs, cam, film, smp, [x.data_ptr() for x in px], rgb.data_ptr(), [s.cuda_stream for s in streams])
    streams[0].synchronize()   # covers every context's device
    for pv in pvs:
        pv.check_errors()
    return px[0].cpu().numpy(), rgb.cpu().numpy()


def _assert_close(got, ref, what):
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6 * np.abs(ref).max(), err_msg=what)


def _frame_matches_single(torch, name, devices):
    ref_px, ref_rgb = _single_frame(torch, name)
    assert np.abs(ref_px).max() > 0
    made = [_context(name, d) for d in devices]
    pvs = [m[0] for m in made]
    try:
        _, _, cam, film, smp, _ = made[0]
        px, rgb = _group_frame(torch, pvs, cam, film, smp, devices)
        _assert_close(px, ref_px, "%s pixels, devices %s" % (name, devices))
        _assert_close(rgb, ref_rgb, "%s rgb, devices %s" % (name, devices))
    finally:
        for pv in pvs:
            pv.close()


# ---------------------------------------------------------------- render_frame_group

def test_group_of_one_is_the_task_loop_plus_resolve(torch_cuda):
    _frame_matches_single(torch_cuda, "vh", [0])


@pytest.mark.parametrize("name", ["vh", "grid16", "sph", "pf_surf"])   # ray-parallel; sliced resolve + replay; FUSED pre-pass; specular recursion
def test_three_contexts_on_one_device_render_the_single_context_frame(torch_cuda, name):
    _frame_matches_single(torch_cuda, name, [0, 0, 0])


@pytest.mark.parametrize("name", ["vh", "grid16", "sph", "pf_surf"])
def test_contexts_on_distinct_devices_render_the_single_context_frame(torch_cuda, name):
    n = _pvol().lib().pvol_device_count()
    if n < 2:
        pytest.skip("one HIP device visible: distinct devices need at least two (the one-device protocol is covered above)")
    _frame_matches_single(torch_cuda, name, list(range(min(3, n))))


# ---------------------------------------------------------------- preprocess_group

def _shoot_result(pv):
    res = {"stats": pv.shoot_stats()}
    res["p"], res["wi"], res["alpha"] = pv.download_photons()
    if pv.params.keep_surface_photons:
        for kind in range(3):
            res["surf%d" % kind] = pv.surface_photons(kind)
        res["rad"] = pv.radiance_photons()
    return res


def _assert_same_shoot(got, ref, what):
    assert got["stats"] == ref["stats"], what
    assert sorted(got) == sorted(ref), what
    for k in ref:
        if k == "stats":
            continue
        g, r = (got[k], ref[k]) if isinstance(ref[k], tuple) else ((got[k],), (ref[k],))
        assert len(g) == len(r), (what, k)
        for x, y in zip(g, r):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("scene,n_photons,n_tasks,block,over", [
    ("volumescene_h", 1500, 16, 256, {}),                           # small blocks: many rounds of count exchanges
    ("pinkfloyd", 4000, 4, 4096, {"keep_surface_photons": 1}),     # spectral splits, the surface stores and radiance photons
])
def test_group_shoot_is_the_single_context_shoot_bit_for_bit(torch_cuda, scene, n_photons, n_tasks, block, over):
    pvol = _pvol()
    s = load_scene(scene)
    p = abi.params_from_blob(s, n_volume_photons=n_photons, **over)
    holder = abi.SceneHolder(s)
    one = pvol.PhotonVolume(p)
    try:
        one.set_scene(holder)
        one.preprocess(n_tasks, block)
        ref = _shoot_result(one)
    finally:
        one.close()
    assert len(ref["p"]) >= n_photons
    if over.get("keep_surface_photons"):
        assert sum(len(ref["surf%d" % k][0]) for k in range(3)) > 0
    for n in (2, 3):
        pvs = [pvol.PhotonVolume(p) for _ in range(n)]
        try:
            for pv in pvs:
                pv.set_scene(holder)
            _within_time(pvol.preprocess_group, pvs, n_tasks, block)
            for i, pv in enumerate(pvs):
                _assert_same_shoot(_shoot_result(pv), ref, "%s N=%d context %d" % (scene, n, i))
                assert pv.exchange_seconds() >= 0.0
        finally:
            for pv in pvs:
                pv.close()


def test_group_shoot_agrees_on_a_local_error(torch_cuda):
    """Every context's block pools are held to 2 photons: each fails its first round on its own (PVOL_E_LIMIT), reports it at the
    count exchange, and the group returns that code with no map anywhere, as the single-context shoot does."""
    pvol = _pvol()
    s = load_scene("volumescene_h")
    p = abi.params_from_blob(s, n_volume_photons=1500)
    holder = abi.SceneHolder(s)
    old = os.environ.get("PVOL_SHOOT_RANK_CAP_MAX")
    os.environ["PVOL_SHOOT_RANK_CAP_MAX"] = "2"
    pvs = [pvol.PhotonVolume(p) for _ in range(2)]
    try:
        for pv in pvs:
            pv.set_scene(holder)
        with pytest.raises(pvol.PvolError) as e:
            _within_time(pvol.preprocess_group, pvs, 16)
        assert e.value.status == abi.PVOL_E_LIMIT
        assert all(pv.photon_count() == 0 for pv in pvs)
    finally:
        if old is None:
            os.environ.pop("PVOL_SHOOT_RANK_CAP_MAX", None)
        else:
            os.environ["PVOL_SHOOT_RANK_CAP_MAX"] = old
        for pv in pvs:
            pv.close()


# ---------------------------------------------------------------- errors

def test_errors_agree_and_nothing_is_left_waiting(torch_cuda):
    pvol = _pvol()
    name = "vh"
    ref_px, ref_rgb = _single_frame(torch_cuda, name)
    made = [_context(name, 0, with_scene=(i != 1)) for i in range(3)]   # context 1 has no scene
    pvs = [m[0] for m in made]
    _, s, cam, film, smp, c = made[0]
    try:
        with pytest.raises(pvol.PvolError) as e:
            _within_time(pvol.preprocess_group, pvs, 4)
        assert e.value.status == abi.PVOL_E_NO_SCENE
        px, rgb, streams = _group_buffers(torch_cuda, film, [0, 0, 0])
        with pytest.raises(pvol.PvolError) as e:
            _within_time(pvol.render_frame_group, pvs, cam, film, smp, [x.data_ptr() for x in px], rgb.data_ptr(),
                         [t.cuda_stream for t in streams])
        assert e.value.status == abi.PVOL_E_NO_SCENE
        torch_cuda.cuda.synchronize()
        assert (rgb.cpu().numpy() == -1.0).all()   # nothing reduced, nothing resolved
        # the same group, once context 1 has its scene
        _give_scene(pvs[1], name, s, c)
        got_px, got_rgb = _group_frame(torch_cuda, pvs, cam, film, smp, [0, 0, 0])
        _assert_close(got_px, ref_px, "pixels after set_scene")
        _assert_close(got_rgb, ref_rgb, "rgb after set_scene")
        # argument checks
        ptrs = [x.data_ptr() for x in px]
        for bad_pvs, bad_px in [([], []), ([pvs[0], pvs[1], pvs[0]], ptrs), (pvs, [ptrs[0], 0, ptrs[2]])]:
            with pytest.raises(pvol.PvolError) as e:
                pvol.render_frame_group(bad_pvs, cam, film, smp, bad_px, rgb.data_ptr())
            assert e.value.status == abi.PVOL_E_INVALID
        for bad_pvs in ([], [pvs[0], pvs[0]]):
            with pytest.raises(pvol.PvolError) as e:
                pvol.preprocess_group(bad_pvs, 4)
            assert e.value.status == abi.PVOL_E_INVALID
    finally:
        for pv in pvs:
            pv.close()


# ---------------------------------------------------------------- front end

def test_render_pbrt_on_two_contexts_matches_one(torch_cuda):
    import importlib.util
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(ROOT, "tools", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    f = os.path.join(GOLD, "scenes", "pinkfloyd_equiv.pbrt")
    kw = dict(xres=48, yres=48, spp=8, photons=30000, shoot_tasks=64, log=lambda *a: None)
    ref, info = rp.render_scene_file(f, **kw)
    img, ginfo = _within_time(rp.render_scene_file, f, devices=[0, 0], **kw)
    assert ginfo["devices"] == [0, 0] and "devices" not in info
    assert ginfo["surface_integrator"] == info["surface_integrator"] and ginfo["photons"] == info["photons"]
    assert ref.mean() > 0
    _assert_close(img, ref, "render_pbrt devices=[0, 0]")
