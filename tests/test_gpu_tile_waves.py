"""The COUNT-mode tile pre-pass in every form it ships in: the one-wave kernel (tile_kernel<count>, one 64-sample trip after the other
with a bulk advance of the stream per trip) and tile_mw_kernel<2|4|8|16>, at sample counts that give every split of a workgroup into
G sample groups x NSL march-step slices (G = min(spp / 64, NW), NSL = NW / G):

    NW  spp   G  NSL          NW  spp   G  NSL
     1  256   -   -  4 trips   8  128   2   4
     2  256   2   1           16  256   4   4
     4  128   2   2           16    4   1  16   more slices than most rays have step pairs
     4  256   4   1            4 1024   4   1   each wave loops over 4 groups
     1 1024   -   - 16 trips  16 1024  16   1

The pre-pass decides every camera ray, every rng_skip and where each task's MT19937 stream stands for the next pixel: one wrong draw
count in one pixel changes the LD shuffles of all later pixels of the task and the stream's end.  So each case renders a tiny frame
(4 x 2 pixels: a 9 x 7 sample extent, 4 tasks of 12 .. 20 pixels) through pvol_render_tasks_device and compares with the oracle's
SamplerRendererTask loop exactly as test_gpu_render.py::test_render_larger_frame_matches_oracle does: sampler values, rays, rng_skip and
stream ends bit for bit, radiance <= 1e-4 relative L2 per sample, film with the same rtol / atol.  pvol_tile_kernel_name says which
form really ran (a requested wave count is rounded down, sliced launches fall back to one wave), and every case asserts it.

The oracle renders once per (scene, spp) (module cache, arrays read-only); every wave count is compared with that."""
import os

import numpy as np
import pytest

from conftest import GOLD, abi, blob, load_photons, load_scene

pytestmark = pytest.mark.gpu

XRES, YRES, NTASKS = 4, 2, 4
LIGHT_KEYS = ("lights.kind", "lights.pos", "lights.dir", "lights.l2w", "lights.w2l", "lights.intensity", "lights.cos")

# scene blob, photon map tag, light kept where the scene has two (None: it has one), surface integrator.  Every one takes the COUNT
# pre-pass on the PAR path (one light, homogeneous medium, no roulette).
SCENES = {
    "vh": ("volumescene_h", "vh", None, False),          # distant light, triangles in LDS: the paired-step shadow-row loop
    "pf_spot": ("pinkfloyd", "pf", 0, False),            # spot light only: the general per-step loop with the falloff test
    "mesh": ("meshroom", "mesh", None, False),           # 966 triangles: BVH closest / any hit inside the counted loop
    "sph_spot": ("sphereroom", "sph", 0, False),         # spheres clip maxt and shadow the steps (both C.nSpheres branches)
    "vh_surf": ("volumescene_h", "vh", None, True),      # surface integrator on: its draws added by slice 0 only, folded into rng_skip
}
WAVES = [None, "1", "2", "4", "8", "16"]
SPPS = [4, 64, 128, 256]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _pvol():
    import importlib
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _render(torch, pv, cam, film, smp, tasks, n):
    dev = torch.device("cuda:0")
    pixels = torch.zeros((film.y_resolution, film.x_resolution, 4), dtype=torch.float32, device=dev)
    rays = torch.zeros((max(n, 1), 48), dtype=torch.uint8, device=dev)
    xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    xyz = torch.zeros((max(n, 1), 4), dtype=torch.float32, device=dev)
    streams = torch.zeros((len(tasks), 32), dtype=torch.uint8, device=dev)
    dbg = abi.RenderDebug(rays.data_ptr(), xy.data_ptr(), xyz.data_ptr(), streams.data_ptr())
    pv.render_tasks(cam, film, smp, tasks, pixels.data_ptr(), dbg)
    rgb = torch.zeros((film.y_resolution, film.x_resolution, 3), dtype=torch.float32, device=dev)
    pv.film_resolve(film, pixels.data_ptr(), rgb.data_ptr())
    torch.cuda.synchronize()
    pv.check_errors()
    return {"pixels": pixels.cpu().numpy(), "rgb": rgb.cpu().numpy(),
            "rays": rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)[:n],
            "xy": xy.cpu().numpy()[:n], "xyzT": xyz.cpu().numpy()[:n],
            "streams": streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)}


class _Scene:
    """One scene's inputs, shared by the oracle and every device context made for it."""

    def __init__(self, name):
        scene, tag, keep, surface = SCENES[name]
        s = load_scene(scene)
        n_lights = len(s["lights.kind"])
        if keep is not None:
            assert n_lights == 2
            s = dict(s)
            for k in LIGHT_KEYS:
                per = len(s[k]) // n_lights
                s[k] = s[k][keep * per:(keep + 1) * per].copy()
        else:
            assert n_lights == 1
        self.blob = s
        self.params = abi.params_from_blob(s)
        self.holder = abi.SceneHolder(s)
        self.photons = load_photons(tag)
        self.surface = None
        self.sampler_kw = {}
        if surface:   # the reference's PhotonIntegrator as the vh_surf capture has it: its sample requests, nused, maxdist, caustic map
            c = blob.load(os.path.join(GOLD, "render_vh_surf.bin"))
            cb = blob.load(os.path.join(GOLD, "caustic_vh.bin"))
            si = c["sampler.i"]
            self.sampler_kw = dict(n1d=tuple(int(v) for v in c["sampler.n1d"]), n2d=tuple(int(v) for v in c["sampler.n2d"]),
                                   tau_index=int(si[4]), scatter_index=int(si[5]))
            self.surface = dict(n_used=int(c["surf.params.i"][0]), max_dist=float(c["surf.params.f"][0]), final_gather=bool(c["surf.params.i"][1]),
                                caustic=(cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), n_paths=int(cb["n_paths"][0]))
        self.oracle = None

    def frame(self, spp):
        pvol = _pvol()
        cam = abi.perspective_camera(float(self.blob["camera.fov"][0]), XRES, YRES, self.blob["camera.c2w"])
        film = abi.make_film(XRES, YRES, pvol.gaussian_filter_table())
        smp = abi.make_sampler(XRES, YRES, spp, NTASKS, **self.sampler_kw)
        return cam, film, smp, np.arange(NTASKS, dtype=np.uint32)

    def device(self, waves):
        """A context created with PVOL_TILE_WAVES = waves (None: unset), which is read at creation."""
        pvol = _pvol()
        old = os.environ.pop("PVOL_TILE_WAVES", None)
        if waves is not None:
            os.environ["PVOL_TILE_WAVES"] = waves
        try:
            pv = pvol.PhotonVolume(self.params)
        finally:
            os.environ.pop("PVOL_TILE_WAVES", None)
            if old is not None:
                os.environ["PVOL_TILE_WAVES"] = old
        try:
            pv.set_scene(self.holder)
            pv.upload_photons(*self.photons)
            if self.surface:
                u = self.surface
                pv.set_surface_integrator(u["n_used"], u["max_dist"], 5, u["final_gather"], u["caustic"], u["n_paths"])
        except Exception:
            pv.close()
            raise
        return pv


@pytest.fixture(scope="module")
def reference(orc):
    """(scene name, spp) -> (scene, camera, film, sampler, tasks, the oracle's render): computed once, then only read."""
    scenes, renders = {}, {}

    def get(name, spp):
        if name not in scenes:
            scenes[name] = _Scene(name)
        sc = scenes[name]
        if (name, spp) not in renders:
            if sc.oracle is None:
                sc.oracle = orc.Oracle(sc.holder, sc.params)
                sc.oracle.set_photons(*sc.photons)
                if sc.surface:
                    u = sc.surface
                    sc.oracle.set_surface_integrator(u["n_used"], u["max_dist"], u["final_gather"], u["caustic"], u["n_paths"])
            cam, film, smp, tasks = sc.frame(spp)
            ref = orc.render_tasks(sc.oracle, cam, film, smp, tasks, n_threads=8)
            assert not ref["unsupported_hits"]
            ref["rgb"] = orc.film_resolve(film, ref["pixels"])
            _not_vacuous(orc, smp, tasks, spp, ref)
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            renders[(name, spp)] = (cam, film, smp, tasks, ref)
        return (sc,) + renders[(name, spp)]
    return get


def _not_vacuous(orc, smp, tasks, spp, ref):
    """What keeps a case from passing without testing anything, asserted on the oracle's own output."""
    for t in tasks:
        w = orc.sub_window(smp, int(t))
        assert (w[1] - w[0]) * (w[3] - w[2]) >= 8                       # a chain of pixels per stream: an early error reaches later ones
    assert ref["n_samples"] == (XRES + 5) * (YRES + 5) * spp
    end = ref["end_draws"]
    if spp >= 128:
        assert end.max() > 624 * 1000                                   # a thousand regenerations of the MT19937 state
    finite = np.isfinite(ref["rays"]["maxt"])
    assert finite.any() and not finite.all()                            # rays clipped by a surface and rays that leave the scene
    assert len(set(end.tolist())) == len(tasks)                         # the tasks' streams do not end alike


def _expected_form(waves):
    if waves is None:
        return "tile_mw_kernel<4>"      # tile_waves_per_task: 4 tasks are fewer than 3 per CU on any device with two CUs or more
    return "tile_kernel<count>" if waves == "1" else "tile_mw_kernel<%s>" % waves


def _check(r, ref):
    """The comparison of test_render_larger_frame_matches_oracle."""
    np.testing.assert_array_equal(r["xy"], ref["image_xy"])
    for f in ("o", "d", "maxt", "time", "scatter_u", "rng_skip"):
        np.testing.assert_array_equal(r["rays"][f], ref["rays"][f], err_msg=f)
    np.testing.assert_array_equal(r["streams"]["end_draw"], ref["end_draws"])
    a, b = r["xyzT"].astype(np.float64), ref["xyzT"].astype(np.float64)
    scale = np.abs(b[:, :3]).max()
    err = np.linalg.norm(a[:, :3] - b[:, :3], axis=1) / np.maximum(np.linalg.norm(b[:, :3], axis=1), 1e-6 * scale)
    assert err.max() <= 1e-4, "per-sample XYZ rel L2 %.3g at %d" % (err.max(), err.argmax())
    np.testing.assert_allclose(r["pixels"], ref["pixels"], rtol=1e-4, atol=1e-5 * np.abs(ref["pixels"]).max())
    np.testing.assert_allclose(r["rgb"], ref["rgb"], rtol=2e-4, atol=1e-4 * np.abs(ref["rgb"]).max())


def _run_case(torch, reference, name, spp, waves):
    sc, cam, film, smp, tasks, ref = reference(name, spp)
    pv = sc.device(waves)
    try:
        assert pv.tile_kernel_name() == ""                               # nothing has run yet
        r = _render(torch, pv, cam, film, smp, tasks, ref["n_samples"])
        assert pv.tile_kernel_name() == _expected_form(waves)            # the form that ran, not the one asked for
        assert pv.march_kernel_name() in ("li_group_kernel", "li_par_kernel")   # the PAR path behind the COUNT pre-pass
        _check(r, ref)
    finally:
        pv.close()


@pytest.mark.parametrize("waves", WAVES, ids=["waves_%s" % (w or "unset") for w in WAVES])
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("name", list(SCENES))
def test_tile_prepass_matches_oracle(torch_cuda, reference, name, spp, waves):
    _run_case(torch_cuda, reference, name, spp, waves)


@pytest.mark.parametrize("waves", ["1", "4", "16"])
def test_tile_prepass_1024spp_matches_oracle(torch_cuda, reference, waves):
    """16 sample groups a pixel: 16 one-wave trips; 4 waves looping over 4 groups each; 16 groups side by side, one slice each."""
    _run_case(torch_cuda, reference, "vh", 1024, waves)


@pytest.mark.parametrize("waves,form", [("3", "tile_mw_kernel<2>"), ("7", "tile_mw_kernel<4>"), ("12", "tile_mw_kernel<8>"), ("101", "tile_mw_kernel<16>")])
def test_requested_wave_count_is_rounded_down_and_named_so(torch_cuda, reference, waves, form):
    sc, cam, film, smp, tasks, ref = reference("vh", 4)
    pv = sc.device(waves)
    try:
        r = _render(torch_cuda, pv, cam, film, smp, tasks, ref["n_samples"])
        assert pv.tile_kernel_name() == form
        _check(r, ref)
    finally:
        pv.close()


def test_forms_that_ignore_the_wave_count_are_named_so(torch_cuda):
    """Two lights: the FUSED pre-pass, one wave per task whatever PVOL_TILE_WAVES says."""
    pvol = _pvol()
    s = load_scene("sphereroom")
    assert len(s["lights.kind"]) == 2
    old = os.environ.pop("PVOL_TILE_WAVES", None)
    os.environ["PVOL_TILE_WAVES"] = "8"
    try:
        pv = pvol.PhotonVolume(abi.params_from_blob(s))
    finally:
        os.environ.pop("PVOL_TILE_WAVES", None)
        if old is not None:
            os.environ["PVOL_TILE_WAVES"] = old
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*load_photons("sph"))
        cam = abi.perspective_camera(float(s["camera.fov"][0]), XRES, YRES, s["camera.c2w"])
        film = abi.make_film(XRES, YRES, pvol.gaussian_filter_table())
        smp = abi.make_sampler(XRES, YRES, 4, NTASKS)
        tasks = np.arange(NTASKS, dtype=np.uint32)
        _render(torch_cuda, pv, cam, film, smp, tasks, int(pvol.render_sample_count(smp, tasks)))
        assert pv.tile_kernel_name() == "tile_kernel<fused>"
    finally:
        pv.close()
