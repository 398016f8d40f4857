"""Volume "exponential" (pvol_volume.kind 4, the reference's volumes/exponential.h: density a * expf(-b * height) inside the extent)
on the device.  The oracle does not know the medium, so three legs that need no new reference code carry it:

  A  wiring, bit for bit: with b = 0 the density is exactly 1 (or a) inside the extent, and so is a 2 x 2 x 2 VolumeGrid of ones
     (of a) over the same extent -- (1 - t) * 1 + t * 1 rounds to 1 in fp32 through all three lerps.  Every device output of the
     two scenes must be bit-identical, and the ones-grid is held to the oracle at the bars test_gpu_group.py / test_gpu_render.py use.
     Radiance out of li_group_kernel (the default path) is the one output that is order-dependent: li_fixup_kernel adds the lookups
     handed over to it with float atomics in whatever order they finish, so a VolumeGrid run does not reproduce ITS OWN bits there.
     Those values are held to the rounding bound of a reordered fp32 sum (_same_up_to_addition_order), and the same test shows that
     two runs of the ones-grid differ within that bound too; T, draw counts, stream positions and every value of the other paths
     stay bit for bit;
  B  the density function against closed form: the optical depth of rays along and across updir;
  C  b != 0 through Li(): against the oracle on the density resampled to a 1 x 1 x N VolumeGrid, within the oracle's own N-vs-2N
     difference plus the usual 1e-4.
The shooter with b != 0 is compared in statistics against the oracle on the resampled grid (paths diverge on one-ulp differences)."""
import importlib
import os

import numpy as np
import pytest

from conftest import abi, load_li_case, load_photons, load_scene, rel_l2

pytestmark = pytest.mark.gpu
EXPONENTIAL = 4
TOL = 1e-4


@pytest.fixture(scope="module")
def pvol():
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1
    return m


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _grid_twin(value=1.0):
    s = dict(load_scene("volumescene_grid16"))
    s["vol.dims"] = np.array([2, 2, 2], np.int32)
    s["vol.density"] = np.full(8, value, np.float32)
    return s


def _exp_scene(a=1.0, b=0.0, up=(0, 1, 0)):
    s = dict(load_scene("volumescene_grid16"))
    s["vol.kind"] = np.array([EXPONENTIAL], np.int32)
    del s["vol.density"]
    s["vol.exp"] = np.array([a, b], np.float32)
    s["vol.updir"] = np.array(up, np.float32)
    return s


def _lattice():
    """16 x 16 rays from the camera of the volumescene (at the origin, inside the medium, looking down +z), four streams of 64."""
    g = (np.arange(16) + .5) / 16 - .5
    yy, xx = np.meshgrid(g, g, indexing="ij")
    d = np.stack([1.2 * xx.ravel(), 1.2 * yy.ravel() + .2, np.ones(256)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = np.random.default_rng(4).random(256).astype(np.float32)
    rays = abi.make_rays(np.zeros((256, 3), np.float32), d.astype(np.float32), np.zeros(256, np.float32), np.full(256, 8.0, np.float32), u)
    return rays, abi.make_streams(np.arange(11, 15, dtype=np.uint32), np.full(4, 64, np.uint32))


NUSED = 50            # params of the grid16 case: a lookup sums up to 50 photons, in the order of the kernel that serves it
LATTICE_TERMS = 55 + NUSED + 4   # one radiance value of the lattice: ceil(8 / 0.15) = 54 steps and the running sum, each step's lookup a sum
                                 # of NUSED photons, a few scalar factors on top
FRAME_STEPS = 125     # a camera ray cannot march more: the diagonal of the medium's world bound (18.7) / 0.15
FRAME_TERMS = FRAME_STEPS + 1 + NUSED + 4
FILM_TERMS = 64       # samples under one pixel's filter: 4 spp x the 4 x 4 pixels a Gaussian of half-width 2 covers


def _same_up_to_addition_order(got, want, n_terms):
    """Equal as sums of the same non-negative fp32 addends taken in two orders, n_terms additions deep (a sum over steps of sums over
    photons: the depths add).  Each order is within (n - 1) 2^-24 of the exact sum, relatively (every partial sum is at most the
    total), so two orders are within 2 (n - 1) 2^-24 of each other."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = 2.0 * (n_terms - 1) * 2.0 ** -24 * np.maximum(np.abs(got), np.abs(want))
    bad = np.abs(got - want) > bound
    assert not bad.any(), "%d values beyond the reordering bound, worst %.3g x the bound" % (int(bad.sum()), float((np.abs(got - want)[bad] / bound[bad]).max()))
    return int((got != want).sum())


def _li(pvol, scene, params, photons, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        pv = pvol.PhotonVolume(params)   # the knobs are read when the context is made
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.upload_photons(*photons)
        rays, streams = _lattice()
        out, draws = pv.li(rays, streams)
        pv.check_errors()
        return out, draws, streams["end_draw"].copy(), pv.march_kernel_name()
    finally:
        pv.close()


@pytest.fixture(scope="module")
def li_params():
    s, p, rays, streams, c = load_li_case("grid16")
    return p


# ------------------------------------------------------------------------------------------------------------------ leg A
def test_set_scene_takes_kind_4_and_checks_its_arguments(pvol, li_params):
    pv = pvol.PhotonVolume(li_params)
    try:
        pv.set_scene(abi.SceneHolder(_exp_scene()))   # PVOL_E_UNSUPPORTED before the medium existed
        S, p, rays, streams, c = load_li_case("trans_grid16")
        before = pv.transmittance(rays, streams.copy())
        # a rejected scene leaves the previous one in place
        for bad in ([1, 0, 0, 0, 0], [np.nan, 0, 0, 1, 0], [1, np.inf, 0, 1, 0], None):
            h = abi.SceneHolder(_exp_scene(a=0.25, b=2.0))
            if bad is None:
                h.scene.volume.density = None
            else:
                h.density[:] = bad
            with pytest.raises(pvol.PvolError) as e:
                pv.set_scene(h)
            assert e.value.status == abi.PVOL_E_INVALID
        np.testing.assert_array_equal(pv.transmittance(rays, streams.copy()), before)
    finally:
        pv.close()


def test_transmittance_equals_the_ones_grid_bit_for_bit(pvol):
    S, p, rays, streams, c = load_li_case("trans_grid16")
    res = []
    for scene in (_grid_twin(), _exp_scene()):
        pv = pvol.PhotonVolume(p)
        try:
            pv.set_scene(abi.SceneHolder(scene))
            st = streams.copy()
            res.append((pv.transmittance(rays, st), st["end_draw"].copy()))
        finally:
            pv.close()
    assert (res[0][0] < 1).any()
    np.testing.assert_array_equal(res[1][0], res[0][0])
    np.testing.assert_array_equal(res[1][1], res[0][1])


@pytest.fixture(scope="module")
def ones_grid_oracle(orc, li_params):
    """The oracle's Li() of the lattice on the ones-grid, computed once."""
    s = _grid_twin()
    o = orc.Oracle(abi.SceneHolder(s), li_params)
    o.set_photons(*load_photons("grid16"))
    rays, streams = _lattice()
    ref, rdraws = o.li_batch(rays, streams, n_threads=8)
    return ref, rdraws, streams["end_draw"].copy()


@pytest.mark.parametrize("env,kernel", [({}, "li_group_kernel"), ({"PVOL_FORCE_SEQ": "1"}, "li_seq_kernel"), ({"PVOL_NO_GROUP": "1"}, "li_replay_kernel")],
                         ids=["default", "force_seq", "no_group"])
def test_li_equals_the_ones_grid_bit_for_bit(pvol, li_params, ones_grid_oracle, env, kernel):
    ph = load_photons("grid16")
    g_out, g_draws, g_end, g_kernel = _li(pvol, _grid_twin(), li_params, ph, env)
    e_out, e_draws, e_end, e_kernel = _li(pvol, _exp_scene(), li_params, ph, env)
    assert g_kernel == e_kernel == kernel
    assert np.linalg.norm(g_out[:, :30], axis=1).min() > 0 and (g_out[:, 30:] < 1).all()
    if kernel == "li_group_kernel":
        again = _li(pvol, _grid_twin(), li_params, ph, env)[0]   # the VolumeGrid against itself: the same bound, no tighter
        print("values that differ: ones-grid run twice %d, twin %d of %d" % (
            _same_up_to_addition_order(again[:, :30], g_out[:, :30], LATTICE_TERMS),
            _same_up_to_addition_order(e_out[:, :30], g_out[:, :30], LATTICE_TERMS), g_out[:, :30].size))
        np.testing.assert_array_equal(again[:, 30:], g_out[:, 30:])
        np.testing.assert_array_equal(e_out[:, 30:], g_out[:, 30:])
    else:
        np.testing.assert_array_equal(e_out, g_out)
    np.testing.assert_array_equal(e_draws, g_draws)
    np.testing.assert_array_equal(e_end, g_end)
    # the twin is tied to the reference, not only to itself: the ones-grid against the oracle (bars of test_gpu_group.py)
    ref, rdraws, rend = ones_grid_oracle
    assert (g_draws == rdraws).all() and (g_end == rend).all()
    floor = 1e-6 * float(np.abs(ref[:, :30]).max())
    assert rel_l2(g_out[:, :30], ref[:, :30], floor=floor).max() <= TOL
    np.testing.assert_allclose(g_out[:, 30:], ref[:, 30:], rtol=1e-5, atol=1e-7)


def test_li_with_a_half_equals_the_half_grid(pvol, li_params):
    """a is not ignored: 0.5 * expf(-0 * h) is exactly 0.5, and so is every lerp of a grid of 0.5."""
    ph = load_photons("grid16")
    g = _li(pvol, _grid_twin(0.5), li_params, ph)
    e = _li(pvol, _exp_scene(a=0.5), li_params, ph)
    one = _li(pvol, _exp_scene(), li_params, ph)
    assert e[3] == g[3] == "li_group_kernel"
    _same_up_to_addition_order(e[0][:, :30], g[0][:, :30], LATTICE_TERMS)
    np.testing.assert_array_equal(e[0][:, 30:], g[0][:, 30:])
    np.testing.assert_array_equal(e[1], g[1])
    np.testing.assert_array_equal(e[2], g[2])
    assert (e[0][:, 30:] > one[0][:, 30:]).all()   # half the density: every ray's transmittance is larger


def test_preprocess_equals_the_ones_grid_bit_for_bit(pvol):
    res = []
    for scene in (_grid_twin(), _exp_scene()):
        p = abi.params_from_blob(scene, n_volume_photons=4000)
        pv = pvol.PhotonVolume(p)
        try:
            pv.set_scene(abi.SceneHolder(scene))
            pv.preprocess(16)
            res.append((pv.download_photons(), pv.shoot_stats()))
        finally:
            pv.close()
    assert len(res[0][0][0]) >= 4000
    for x, y in zip(res[1][0], res[0][0]):
        np.testing.assert_array_equal(x, y)
    assert res[1][1] == res[0][1]


def _render(torch, pv, cam, film, smp, tasks, n):
    dev = torch.device("cuda:0")
    pixels = torch.zeros((film.y_resolution, film.x_resolution, 4), dtype=torch.float32, device=dev)
    rays = torch.zeros((n, 48), dtype=torch.uint8, device=dev)
    xy = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    xyz = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    streams = torch.zeros((len(tasks), 32), dtype=torch.uint8, device=dev)
    pv.render_tasks(cam, film, smp, tasks, pixels.data_ptr(), abi.RenderDebug(rays.data_ptr(), xy.data_ptr(), xyz.data_ptr(), streams.data_ptr()))
    torch.cuda.synchronize()
    pv.check_errors()
    return pixels.cpu().numpy(), xyz.cpu().numpy(), streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)["end_draw"].copy()


def test_render_tasks_equal_the_ones_grid_bit_for_bit(pvol, torch_cuda, orc, li_params):
    xres = yres = 32
    spp, ntasks = 4, 4
    s = _grid_twin()
    cam = abi.perspective_camera(float(s["camera.fov"][0]), xres, yres, s["camera.c2w"])
    film = abi.make_film(xres, yres, pvol.gaussian_filter_table())
    smp = abi.make_sampler(xres, yres, spp, ntasks)
    tasks = np.arange(ntasks, dtype=np.uint32)
    n = pvol.render_sample_count(smp, tasks)
    ph = load_photons("grid16")
    res = []
    for scene in (s, _exp_scene(), s):   # the ones-grid a second time: its own repeat
        pv = pvol.PhotonVolume(li_params)
        try:
            pv.set_scene(abi.SceneHolder(scene))
            pv.upload_photons(*ph)
            res.append(_render(torch_cuda, pv, cam, film, smp, tasks, n))
            assert pv.march_kernel_name() == "li_group_kernel"
        finally:
            pv.close()
    assert np.abs(res[0][0][..., :3]).max() > 0
    for other, what in ((res[2], "ones-grid run twice"), (res[1], "twin")):
        # X, Y, Z per sample: positive weights times li_group_kernel's radiance; film: positive filter weights times those
        nd = (_same_up_to_addition_order(other[1][:, :3], res[0][1][:, :3], FRAME_TERMS),
              _same_up_to_addition_order(other[0], res[0][0], FRAME_TERMS + FILM_TERMS))
        print("%s: %d XYZ values and %d film values differ" % (what, nd[0], nd[1]))
        np.testing.assert_array_equal(other[1][:, 3], res[0][1][:, 3])      # T.y per sample
        np.testing.assert_array_equal(other[2], res[0][2])                  # stream positions
    # the ones-grid against the oracle's SamplerRendererTask loop (bars of test_gpu_render.py)
    o = orc.Oracle(abi.SceneHolder(s), li_params)
    o.set_photons(*ph)
    r = orc.render_tasks(o, cam, film, smp, tasks, n_threads=8)
    pixels, xyz, end = res[0]
    np.testing.assert_array_equal(end, r["end_draws"])
    ref = r["xyzT"].astype(np.float64)
    scale = max(np.abs(ref[:, :3]).max(), 1e-30)
    err = np.linalg.norm(xyz[:, :3] - ref[:, :3], axis=1) / np.maximum(np.linalg.norm(ref[:, :3], axis=1), 1e-6 * scale)
    assert err.max() <= 1e-4, "per-sample XYZ rel L2 %.3g" % err.max()
    np.testing.assert_allclose(xyz[:, 3], ref[:, 3], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(pixels, r["pixels"], rtol=1e-4, atol=1e-5 * np.abs(r["pixels"]).max())


# ------------------------------------------------------------------------------------------------------------------ leg B
def _rot_z(deg, t):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4)
    m[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    m[:3, 3] = t
    return m


R2 = float(np.sqrt(2.0))
# name, updir as given, extent (a box of height 2 along updir), volume_to_world,
# the ray along updir through the whole box (origin, direction; volume space), the ray across updir at height 0.7 and its length inside
CONFIGS = [
    ("up_y", (0, 1, 0), (0, 0, 0, 1, 2, 1), np.eye(4), ((.5, -1, .5), (0, 1, 0)), ((-1, .7, .5), (1, 0, 0)), 1.0),
    ("up_y_unnormalised", (0, 3, 0), (0, 0, 0, 1, 2, 1), np.eye(4), ((.5, -1, .5), (0, 1, 0)), ((-1, .7, .5), (1, 0, 0)), 1.0),
    ("oblique", (1, 1, 0), (0, 0, 0, R2, R2, 1), np.eye(4), ((-1, -1, .5), (1 / R2, 1 / R2, 0)),
     ((.7 / R2 - 2 / R2, .7 / R2 + 2 / R2, .5), (1 / R2, -1 / R2, 0)), 1.4),
    ("rotated_volume", (0, 1, 0), (0, 0, 0, 1, 2, 1), _rot_z(30.0, (0.4, -0.3, 1.1)), ((.5, -1, .5), (0, 1, 0)), ((-1, .7, .5), (1, 0, 0)), 1.0),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_optical_depth_against_closed_form(pvol, cfg):
    """b = 1.5, a = 1, a box of height 2 along updir, stepsize 0.01: Transmittance() steps by s = 0.04 with one drawn offset.
    Along updir through the whole box tau = sigma_t a (1 - e^(-b L)) / b with L = 2; across updir at height h tau = sigma_t a e^(-b h) L.
    The stepped sum of a monotone integrand with one offset differs from the integral by at most s x (its largest value)
    = s sigma_t a (max density = 1): that is the bar on tau = -log T, per bin."""
    name, up, extent, v2w, along, across, across_len = cfg
    a, b, h, s_step = 1.0, 1.5, 0.7, 0.04
    scene = _exp_scene(a, b, up)
    scene["vol.extent"] = np.array(extent, np.float32)
    scene["vol.v2w"] = v2w.astype(np.float32).reshape(16)
    scene["vol.w2v"] = np.linalg.inv(v2w).astype(np.float32).reshape(16)
    p = abi.params_from_blob(scene, step_size=0.01)
    o = np.array([along[0], across[0]], np.float64)
    d = np.array([along[1], across[1]], np.float64)
    ow = (v2w[:3, :3] @ o.T).T + v2w[:3, 3]   # the rays are stated in volume space
    dw = (v2w[:3, :3] @ d.T).T
    rays = abi.make_rays(ow.astype(np.float32), dw.astype(np.float32), np.zeros(2, np.float32), np.full(2, 10.0, np.float32), np.zeros(2, np.float32))
    streams = abi.make_streams(np.array([5], np.uint32), np.array([2], np.uint32))
    pv = pvol.PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        T = pv.transmittance(rays, streams).astype(np.float64)
    finally:
        pv.close()
    sig_t = (scene["vol.sigma_a"] + scene["vol.sigma_s"]).astype(np.float64)
    want = np.stack([sig_t * a * (1 - np.exp(-b * 2.0)) / b, sig_t * a * np.exp(-b * h) * across_len])
    got = -np.log(T)
    bound = s_step * sig_t * a * 1.0
    print(name, "tau/sigma_t got", (got / sig_t)[:, 0], "want", (want / sig_t)[:, 0], "bound", s_step)
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()


# ------------------------------------------------------------------------------------------------------------------ leg C
def _resampled_grid(n, a, b):
    """The exponential density along the volume's z at the centres of a 1 x 1 x n VolumeGrid."""
    s = dict(load_scene("volumescene_grid16"))
    z0, z1 = float(s["vol.extent"][2]), float(s["vol.extent"][5])
    height = (np.arange(n) + .5) / n * (z1 - z0)
    s["vol.dims"] = np.array([1, 1, n], np.int32)
    s["vol.density"] = (a * np.exp(-b * height)).astype(np.float32)
    return s


def test_li_with_falloff_against_the_oracle_on_a_resampled_grid(pvol, orc, li_params):
    """updir along the volume's z, a = 1, b = 1 (the density falls from 1 to e^-10 over the extent; sigma_t 0.15 x step 0.15: no step
    comes near the roulette).  The oracle renders the lattice on the density resampled to 1 x 1 x 256 and 1 x 1 x 512; its own
    256-vs-512 difference bounds the discretisation error of the finer grid (trilinear error falls about 4x per doubling).  Bar per
    ray: ||device - oracle512|| <= ||oracle256 - oracle512|| + 1e-4 ||oracle512||.  Stream positions are equal (the draw count depends
    only on where the density is non-zero).
    Measured: the oracle's 256-vs-512 difference is at most 2.8e-4 of a ray's radiance (median 8.6e-5) and at most 1.2e-6
    absolute on T."""
    a, b = 1.0, 1.0
    ph = load_photons("grid16")
    rays, streams = _lattice()
    refs = []
    for n in (256, 512):
        o = orc.Oracle(abi.SceneHolder(_resampled_grid(n, a, b)), li_params)
        o.set_photons(*ph)
        st = streams.copy()
        o.counters(reset=True)
        refs.append(o.li_batch(rays, st, n_threads=8) + (st["end_draw"].copy(),))
        # no step reached the roulette: every draw of the batch is one of Li()'s fixed ones -- 4 scrambles a ray, 6 shuffle draws and
        # one tau() offset a step, one Transmittance() offset per unoccluded shadow ray (the roulette would add one per step it met)
        k = o.counters()
        assert int(refs[-1][1].sum()) == 4 * k["n_rays"] + 7 * k["n_steps"] + k["n_shadow_unoccluded"], k
        o.close()
    (r256, d256, e256), (r512, d512, e512) = refs
    got, draws, end, kernel = _li(pvol, _exp_scene(a, b, (0, 0, 1)), li_params, ph)
    assert kernel == "li_group_kernel"
    assert (draws == d512).all() and (end == e512).all() and (e256 == e512).all()
    for sl, what in ((slice(0, 30), "Lv"), (slice(30, 60), "T")):
        own = np.linalg.norm(r256[:, sl].astype(np.float64) - r512[:, sl], axis=1)
        norm = np.linalg.norm(r512[:, sl].astype(np.float64), axis=1)
        err = np.linalg.norm(got[:, sl].astype(np.float64) - r512[:, sl], axis=1)
        print(what, "oracle 256-vs-512 max rel %.3g median rel %.3g; device-vs-512 max rel %.3g" %
              ((own / norm).max(), np.median(own / norm), (err / norm).max()))
        assert (norm > 0).all()
        assert (err <= own + TOL * norm).all(), (what, float((err / (own + TOL * norm)).max()))


# ------------------------------------------------------------------------------------------------------------- shooter, b != 0
def test_shooter_statistics_with_falloff_against_the_oracle(pvol, orc):
    """updir along the volume's z, a = 1, b = 0.2, only the volume store wanted: 1 024 tasks shoot one block of 4 096 paths each (the
    shoot ends after the first round, so both sides follow the same 4 194 304 paths up to one-ulp decisions).  Device on the
    exponential medium against the oracle on the density resampled to 1 x 1 x 512: stored volume photons per shot path, and the
    mean height of a stored photon.  Margin: four times the oracle's own standard deviation of the statistic over four disjoint
    task ranges of this shoot (tasks 0-255, 256-511, 512-767, 768-1023; a shoot of the first n tasks is a prefix of the whole one, so
    shoots of 256, 512, 768 and 1 024 tasks give the ranges).  Measured on the CPU:
        photons per path  8.2254e-4 overall; ranges 7.8773e-4, 8.1921e-4, 8.2684e-4, 8.5640e-4; standard deviation 2.821e-5
        mean height       3.2216 overall;    ranges 3.1433, 3.3310, 3.2689, 3.1434;             standard deviation 0.09388
    A wrong sign of b or pMax as the origin multiplies the density by up to e^2 and moves the rate by far more than the 14 % the
    margin allows."""
    SD_RATE, SD_HEIGHT = 2.821e-5, 0.09388
    n_tasks, block = 1024, 4096
    a, b = 1.0, 0.2
    over = dict(n_volume_photons=1, n_caustic_photons=0, n_indirect_photons=0)
    grid = _resampled_grid(512, a, b)
    z0 = float(grid["vol.extent"][2])
    w2v = grid["vol.w2v"].reshape(4, 4)

    def stats(st, P):
        height = P.astype(np.float64) @ w2v[2, :3] + w2v[2, 3] - z0
        return st["stored_volume"] / st["paths"], float(height.mean())
    o = orc.Oracle(abi.SceneHolder(grid), abi.params_from_blob(grid, **over))
    assert o.shoot(n_tasks, 8, block) == 0
    rst = o.shoot_stats()
    want = stats(rst, o.get_photons()[0])
    o.close()
    scene = _exp_scene(a, b, (0, 0, 1))
    pv = pvol.PhotonVolume(abi.params_from_blob(scene, **over))
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.preprocess(n_tasks, block)
        gst = pv.shoot_stats()
        got = stats(gst, pv.download_photons()[0])
    finally:
        pv.close()
    print("photons per path: device %.4e oracle %.4e; mean height: device %.4f oracle %.4f" % (got[0], want[0], got[1], want[1]))
    assert gst["paths"] == rst["paths"] == n_tasks * block
    assert rst["stored_volume"] > 3000
    assert abs(got[0] - want[0]) <= 4 * SD_RATE
    assert abs(got[1] - want[1]) <= 4 * SD_HEIGHT


def test_render_pbrt_renders_the_fog_fixture(torch_cuda):
    """tools/render_pbrt.py on tests/golden/scenes/fog_exponential.pbrt, as the README's line runs it: scene file -> shoot -> frame.
    The surface term is refused on a density region, so the image is the fog's own radiance: finite, and lit over most of the frame."""
    import importlib.util
    from conftest import GOLD, ROOT
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(ROOT, "tools", "render_pbrt.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    img, info = tool.render_scene_file(os.path.join(GOLD, "scenes", "fog_exponential.pbrt"), 64, 64, 4, shoot_tasks=64, log=lambda *a: None)
    assert img.shape == (64, 64, 3) and np.isfinite(img).all()
    assert info["photons"] >= 4000 and not info["surface_integrator"]
    assert (img.max(axis=2) > 0).mean() > 0.5
