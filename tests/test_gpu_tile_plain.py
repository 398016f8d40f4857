"""The PLAIN form of the COUNT-mode tile pre-pass (pvol_tile_dev.h, chosen per batch by pvol_tile_plain_gate) against the general form on the
same inputs: PVOL_TILE_GENERAL=1, read when a context is created, keeps the general kernels.  PLAIN only compiles tests out -- the taken
path executes the same operations in the same order -- so the camera rays (all 48 bytes: origin, direction, maxt, time, scatter_u, rng_skip),
the image positions and the stream records (every end_draw) must be bitwise equal, and so must the radiance the Li kernels compute from those
rays.  pvol_tile_form_name says which form really ran and every case asserts it.

Every case renders on both Li paths.  Behind li_par_kernel (PVOL_NO_GROUP=1: one wave per ray, a fixed summation order) d_xyz is asserted
bitwise equal like the other three records.  Behind li_group_kernel, the default, rays, image positions and stream records are asserted
bitwise equal and the d_xyz figure is printed, not asserted: that kernel adds a ray's deferred lookups to its result with floating-point
atomics (li_fixup_kernel), in whatever order they finish, so d_xyz is not reproducible from one run to the next of the SAME form on the same
rays.  Measured on an MI355X at 24 x 16, 16 spp: general against general 1 and 2 of 9 744 records differ, PLAIN against general 5 and 1, all by
one ulp in one component; at 6 x 4, 256 spp none differ either way; behind li_par_kernel none differ in any render.

Shapes, on scene_volumescene_h (tests/test_gpu_tile_waves.py pins the same kernels against the oracle):
    24 x 16 pixels, 16 spp, 8 tasks   a partial lane trip (16 of 64 lanes); its rays are checked to hold odd and even march-step counts (the
                                      j + 1 < nSamples tail of the two-step loop); repeated with the one-wave kernel and tile_mw_kernel at
                                      2, 4, 8 and 16 waves per task (PVOL_TILE_WAVES)
    6 x 4 pixels, 256 spp, 4 tasks    four 64-sample trips per pixel in the one-wave kernel, four sample groups in tile_mw_kernel<4>
    12 x 8 pixels, 16 spp, 4 tasks    the camera pulled 8 units back, out of the medium (the scene's own camera stands inside it, so all its
                                      rays cross the extent): three rays in four miss the extent (tile_count_draws' early return), the
                                      others hold odd and even step counts
and scene_meshroom (a triangle hierarchy: never PLAIN) renders identically with and without the knob, in the general form both times.

The general form renders once per shape and Li path (module cache, arrays read-only); every other render is compared with that."""
import os

import numpy as np
import pytest

from conftest import abi, load_photons, load_scene

pytestmark = pytest.mark.gpu

# name -> scene blob, photon map tag, x resolution, y resolution, spp, tasks, how far the camera is moved back along its view axis
SHAPES = {
    "vh_24x16_16spp": ("volumescene_h", "vh", 24, 16, 16, 8, 0.0),
    "vh_6x4_256spp": ("volumescene_h", "vh", 6, 4, 256, 4, 0.0),
    "vh_outside_12x8_16spp": ("volumescene_h", "vh", 12, 8, 16, 4, 8.0),
    "mesh_6x4_16spp": ("meshroom", "mesh", 6, 4, 16, 4, 0.0),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _pvol():
    import importlib
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _context(params, holder, photons, waves, general, par):
    """A context created with PVOL_TILE_WAVES = waves (None: unset), PVOL_TILE_GENERAL = 1 or unset and PVOL_NO_GROUP = 1 (li_par_kernel) or
    unset: all three are read at creation."""
    env = {"PVOL_TILE_WAVES": waves, "PVOL_TILE_GENERAL": "1" if general else None, "PVOL_NO_GROUP": "1" if par else None}
    old = {k: os.environ.pop(k, None) for k in env}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = v
    try:
        pv = _pvol().PhotonVolume(params)
    finally:
        for k in env:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    try:
        pv.set_scene(holder)
        pv.upload_photons(*photons)
    except Exception:
        pv.close()
        raise
    return pv


class _Shape:
    def __init__(self, name):
        self.name = name
        scene, tag, self.xres, self.yres, self.spp, self.ntasks, back = SHAPES[name]
        self.blob = load_scene(scene)
        assert len(self.blob["lights.kind"]) == 1
        self.params = abi.params_from_blob(self.blob)
        self.holder = abi.SceneHolder(self.blob)
        self.photons = load_photons(tag)
        pvol = _pvol()
        c2w = np.array(self.blob["camera.c2w"], np.float32).reshape(4, 4)
        c2w[:3, 3] -= np.float32(back) * c2w[:3, 2]
        self.cam = abi.perspective_camera(float(self.blob["camera.fov"][0]), self.xres, self.yres, c2w.reshape(-1))
        self.film = abi.make_film(self.xres, self.yres, pvol.gaussian_filter_table())
        self.smp = abi.make_sampler(self.xres, self.yres, self.spp, self.ntasks)
        self.tasks = np.arange(self.ntasks, dtype=np.uint32)
        self.n = int(pvol.render_sample_count(self.smp, self.tasks))
        assert self.n == (self.xres + 5) * (self.yres + 5) * self.spp   # the whole sample extent: all tasks

    def render(self, torch, waves, general, par):
        """The debug records of one render as raw bytes / words, with the names of what ran."""
        pv = _context(self.params, self.holder, self.photons, waves, general, par)
        try:
            dev = torch.device("cuda:0")
            n = self.n
            pixels = torch.zeros((self.yres, self.xres, 4), dtype=torch.float32, device=dev)
            rays = torch.zeros((n, 48), dtype=torch.uint8, device=dev)
            xy = torch.zeros((n, 2), dtype=torch.float32, device=dev)
            xyz = torch.zeros((n, 4), dtype=torch.float32, device=dev)
            streams = torch.zeros((self.ntasks, 32), dtype=torch.uint8, device=dev)
            dbg = abi.RenderDebug(rays.data_ptr(), xy.data_ptr(), xyz.data_ptr(), streams.data_ptr())
            pv.render_tasks(self.cam, self.film, self.smp, self.tasks, pixels.data_ptr(), dbg)
            torch.cuda.synchronize()
            pv.check_errors()
            r = {"rays": rays.cpu().numpy(), "xy": xy.cpu().numpy().view(np.uint32), "xyz": xyz.cpu().numpy().view(np.uint32),
                 "streams": streams.cpu().numpy(), "form": pv.tile_form_name(), "kernel": pv.tile_kernel_name(),
                 "march": pv.march_kernel_name()}
        finally:
            pv.close()
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return r


@pytest.fixture(scope="module")
def general(torch_cuda):
    """(shape name, par) -> (shape, its render in the general form at the heuristic's wave count, behind li_par_kernel or li_group_kernel):
    rendered once, then only read."""
    shapes, cache = {}, {}

    def get(name, par):
        if name not in shapes:
            shapes[name] = _Shape(name)
        sh = shapes[name]
        if (name, par) not in cache:
            r = sh.render(torch_cuda, None, True, par)
            assert r["form"] == "general"
            assert r["march"] in (("li_par_kernel",) if par else ("li_group_kernel", "li_par_kernel"))   # the PAR path behind a COUNT pre-pass
            _not_vacuous(sh, r)
            cache[(name, par)] = r
        return sh, cache[(name, par)]
    return get


def _step_counts(sh, rays):
    """Per ray the march steps of tile_count_draws (vol_intersect against the extent in volume space, ceil(length / stepSize)), -1 for a
    ray that misses the extent.  float64: a ray within rounding of a step boundary may be off by one, which no assertion here depends on."""
    r = rays.view(abi.RAY_DTYPE).reshape(-1)
    m = sh.blob["vol.w2v"].astype(np.float64).reshape(4, 4)
    o = r["o"].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    d = r["d"].astype(np.float64) @ m[:3, :3].T
    lo, hi = sh.blob["vol.extent"][:3].astype(np.float64), sh.blob["vol.extent"][3:].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    t0 = np.maximum(np.minimum(ta, tb).max(axis=1), 0.0)
    t1 = np.minimum(np.maximum(ta, tb).min(axis=1), r["maxt"].astype(np.float64))
    hit = t1 > t0
    steps = np.where(hit, np.ceil((t1 - t0) / float(sh.params.step_size)), -1.0)
    return steps.astype(np.int64)


def _not_vacuous(sh, r):
    rays = r["rays"].view(abi.RAY_DTYPE).reshape(-1)
    end = r["streams"].view(abi.STREAM_DTYPE).reshape(-1)["end_draw"]
    assert len(set(end.tolist())) == sh.ntasks and end.min() > 0           # every task walked its own stream
    assert np.abs(r["xyz"].view(np.float32)[:, :3]).max() > 0.0           # the Li kernels ran on these rays
    finite = np.isfinite(rays["maxt"])
    assert finite.any() and not finite.all()                              # rays clipped by a triangle and rays that leave the scene
    if sh.name in ("vh_24x16_16spp", "vh_outside_12x8_16spp"):
        steps = _step_counts(sh, r["rays"])
        n_miss, n_odd, n_even = int((steps < 0).sum()), int(((steps > 0) & (steps % 2 == 1)).sum()), int(((steps > 0) & (steps % 2 == 0)).sum())
        print("%s: %d rays miss the extent, %d with an odd and %d with an even step count" % (sh.name, n_miss, n_odd, n_even))
        assert min(n_odd, n_even) >= len(steps) // 50                     # each kind in bulk, far from any off-by-one of the estimate
        if "outside" in sh.name:
            assert n_miss >= len(steps) // 50


def _assert_same(r, ref, par):
    for k, what in (("rays", "camera rays"), ("xy", "image positions"), ("streams", "stream records"), ("xyz", "radiance (d_xyz)")):
        diff = int((r[k] != ref[k]).any(axis=1).sum())
        print("%s behind %s: %d of %d records differ" % (what, ref["march"], diff, len(ref[k])))
    for k in ("rays", "xy", "streams") + (("xyz",) if par else ()):   # d_xyz behind li_group_kernel: see the module's docstring
        np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def _kernel(waves, heuristic):
    if waves is None:
        return heuristic
    return "tile_kernel<count>" if waves == "1" else "tile_mw_kernel<%s>" % waves


def _compare(torch, general, name, waves, keep_general, form):
    """One render of `name` on each Li path, with the knob (keep_general) or without, against the general form's."""
    for par in (False, True):
        sh, ref = general(name, par)
        r = sh.render(torch, waves, keep_general, par)
        assert r["form"] == form
        assert r["kernel"] == _kernel(waves, ref["kernel"])
        assert r["march"] == ref["march"]
        _assert_same(r, ref, par)


WAVES = [None, "1", "2", "4", "8", "16"]


@pytest.mark.parametrize("waves", WAVES, ids=["waves_%s" % (w or "unset") for w in WAVES])
def test_plain_equals_general_partial_trip(torch_cuda, general, waves):
    """24 x 16 at 16 spp, in the one-wave kernel and every multi-wave one (the heuristic picks among 1, 2 and 4; 8 and 16 by request)."""
    _compare(torch_cuda, general, "vh_24x16_16spp", waves, False, "plain")


@pytest.mark.parametrize("waves", [None, "1"], ids=["waves_unset", "waves_1"])
def test_plain_equals_general_four_trips(torch_cuda, general, waves):
    """6 x 4 at 256 spp: four trips per pixel with one wave per task, four sample groups side by side otherwise."""
    _compare(torch_cuda, general, "vh_6x4_256spp", waves, False, "plain")


@pytest.mark.parametrize("waves", [None, "1"], ids=["waves_unset", "waves_1"])
def test_plain_equals_general_rays_that_miss_the_extent(torch_cuda, general, waves):
    _compare(torch_cuda, general, "vh_outside_12x8_16spp", waves, False, "plain")


def test_general_one_wave_kernel_equals_the_reference_render(torch_cuda, general):
    """The reference ran at the heuristic's wave count; the general one-wave kernel (the flagship's before PLAIN) gives the same records."""
    _compare(torch_cuda, general, "vh_24x16_16spp", "1", True, "general")


@pytest.mark.parametrize("waves", [None, "1"], ids=["waves_unset", "waves_1"])
def test_scene_with_a_hierarchy_never_takes_plain(torch_cuda, general, waves):
    _compare(torch_cuda, general, "mesh_6x4_16spp", waves, False, "general")   # the gate's decision, not the knob's


