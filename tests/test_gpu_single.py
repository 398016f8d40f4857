"""VolumeIntegrator "single" on the device (pvol_set_volume_integrator, csrc/pvol_single.hip) against tests/single_ref.py,
the numpy restatement of single.cpp:66-139 that test_single_ref.py ties to the reference.  Bars: draw counts, stream ends and the
final RNG state exact; Lv and T within 1e-4 relative L2 per ray (the floor of tests/test_gpu_parity.py).  Then the render driver by
composition: its samples are pvol_li_batch's on its own rays and streams, with the surface term in front where that is on."""
import os

import numpy as np
import pytest

import single_ref
from conftest import abi, load_li_case, load_render_case, load_scene

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _pvol():
    import importlib
    return importlib.import_module("cs348b-pbrt_amd.pvol")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def context(s, step_size, env=None):
    """A context over the scene blob under SINGLE; `env`: knobs the context reads when it is created."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        pv = _pvol().PhotonVolume(abi.params_from_blob(s, step_size=float(step_size)))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.set_volume_integrator("single")
        assert pv.volume_integrator() == "single"
    except Exception:
        pv.close()
        raise
    return pv


def reference(orc, s, step_size, rays, streams, **kw):
    o = orc.Oracle(abi.SceneHolder(s), abi.params_from_blob(s, step_size=float(step_size)))
    infos = {}
    out = single_ref.li_batch(s, step_size, rays, streams, single_ref.oracle_occlusion(o), infos=infos, **kw)
    o.close()
    return out + ([infos[i] for i in range(len(rays))],)


def check(pv, s, rays, streams, ref, kernel=None):
    """Both output kinds of one batch against the restatement; returns the largest error and the draws."""
    out_ref, draws_ref, ends_ref = ref[0], ref[1], ref[2]
    st = streams.copy()
    out, draws = pv.li(rays, st)
    if kernel:
        assert pv.march_kernel_name() == kernel
    np.testing.assert_array_equal(draws, draws_ref)
    np.testing.assert_array_equal(st["end_draw"], ends_ref)
    err = single_ref.row_error(out, out_ref).max()
    st2 = streams.copy()
    xyz, draws2 = pv.li(rays, st2, abi.OUT_XYZ)
    np.testing.assert_array_equal(draws2, draws_ref)
    np.testing.assert_array_equal(st2["end_draw"], ends_ref)
    ref_xyz = single_ref.xyz_rows(s, out_ref)
    floor = 1e-6 * max(float(np.abs(ref_xyz[:, :3]).max()), 1e-30)
    e_xyz = (np.linalg.norm(xyz[:, :3] - ref_xyz[:, :3], axis=1) / np.maximum(np.linalg.norm(ref_xyz[:, :3], axis=1), floor)).max()
    e_ty = (np.abs(xyz[:, 3] - ref_xyz[:, 3]) / np.maximum(np.abs(ref_xyz[:, 3]), 1e-30)).max()
    print("single vs restatement: %d rays, spectral %.3g, XYZ %.3g, T.y %.3g" % (len(rays), err, e_xyz, e_ty))
    assert err <= TOL and e_xyz <= TOL and e_ty <= TOL
    return max(err, e_xyz, e_ty), draws


def one_light(s, i):
    """The scene with light i alone."""
    s = dict(s)
    n = len(s["lights.kind"])
    for k, w in (("lights.kind", 1), ("lights.pos", 3), ("lights.dir", 3), ("lights.l2w", 16), ("lights.w2l", 16), ("lights.intensity", 30), ("lights.cos", 2)):
        s[k] = np.ascontiguousarray(np.asarray(s[k]).reshape(n, w)[i:i + 1].reshape(-1))
    return s


# ---------------------------------------------------------------- march lengths and streams (volumescene_h: one distant light)
STEP = 0.05   # 129 march steps fit the room's length


def march_rays():
    """130 rays in streams of 1, 64 and 65.  World = volume - (0, 0.5, -3.5); the extent is [-10, 5] x [0, 5] x [-5, 5] in volume space.
    Rays along +x from inside the extent cut to 1, 63, 64, 65 and 129 march steps (maxt = 0.05 k - 0.01); one that misses the extent,
    one with t1 == t0 (it ends where it would enter), one entering from outside; the rest short rays in all directions."""
    rng = np.random.RandomState(11)
    o, d, maxt = [], [], []
    for k in (1, 63, 64, 65, 129):
        o.append([-9.5, 2.0, 3.5]); d.append([1, 0, 0]); maxt.append(STEP * k - 0.01)
    o.append([-12.0, 2.0, 3.5]); d.append([-1, 0, 0]); maxt.append(50.0)       # misses
    o.append([-11.0, 2.0, 3.5]); d.append([1, 0, 0]); maxt.append(1.0)         # t1 == t0 == 1
    o.append([-11.0, 2.0, 3.5]); d.append([1, 0, 0]); maxt.append(1.0 + 0.32)  # from outside, 7 steps
    while len(o) < 130:
        v = rng.normal(size=3)
        o.append([rng.uniform(-9, 4), rng.uniform(0, 4), rng.uniform(-1, 8)]); d.append(v / np.linalg.norm(v)); maxt.append(rng.uniform(0.02, 0.33))
    n = len(o)
    rays = abi.make_rays(np.array(o, np.float32), np.array(d, np.float32), np.zeros(n, np.float32), np.array(maxt, np.float32),
                         rng.uniform(0, 1, n).astype(np.float32), 0.0, rng.randint(0, 40, n).astype(np.uint32))
    return rays, abi.make_streams([5, 6, 7], [1, 64, 65], [0, 17, 1000])


@pytest.fixture(scope="module")
def march_case(orc):
    s = load_scene("volumescene_h")
    rays, streams = march_rays()
    return s, rays, streams, reference(orc, s, STEP, rays, streams)


def test_march_lengths_streams_and_both_output_kinds(march_case):
    s, rays, streams, ref = march_case
    steps = [i["steps"] for i in ref[4]]
    assert steps[:8] == [1, 63, 64, 65, 129, 0, 0, 7]
    # steps shadowed by the room's triangles beside lit ones
    assert sum(i["shadowed"] for i in ref[4]) > 20 and sum(i["unoccluded"] for i in ref[4]) > 100
    assert ref[1][5] == 0 and ref[1][6] == 0 and (ref[0][5:7, 30:] == 1).all()   # a miss and t1 == t0: T = 1, nothing drawn
    pv = context(s, STEP)
    try:
        check(pv, s, rays, streams, ref, "single_par_kernel")
        a, _ = pv.li(rays, streams.copy())
        b, _ = pv.li(rays, streams.copy())
        assert a.tobytes() == b.tobytes()   # two runs byte-equal
    finally:
        pv.close()


def test_sequential_form_on_the_same_batch(march_case):
    s, rays, streams, ref = march_case
    pv = context(s, STEP, {"PVOL_FORCE_SEQ": "1"})
    try:
        check(pv, s, rays, streams, ref, "single_seq_kernel")
    finally:
        pv.close()


# ---------------------------------------------------------------- lights
def golden_rays(case, n_streams=2, per_stream=24):
    """Camera rays of a golden Li() case in fresh streams."""
    _, _, rays, _, _ = load_li_case(case)
    rays = rays[:n_streams * per_stream].copy()
    return rays, abi.make_streams(list(range(3, 3 + n_streams)), [per_stream] * n_streams, 0)


def spot_rays(s, n=24):
    """Rays that cross the spot light's cone at right angles to its axis, 1.6 cone radii to either side of it: black samples
    outside (spot.cpp:60-69 returns 0 below cosTotalWidth), the falloff ramp, the full cone."""
    rng = np.random.RandomState(5)
    pos = np.asarray(s["lights.pos"][:3], np.float64)
    axis = np.asarray(s["lights.w2l"], np.float64).reshape(4, 4)[2, :3]
    axis /= np.linalg.norm(axis)
    tan = np.tan(np.arccos(float(s["lights.cos"][0])))
    o, d, maxt = [], [], []
    for i in range(n):
        perp = np.cross(axis, rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        h = rng.uniform(1.0, 3.0)
        R = 1.6 * h * tan
        o.append(pos + axis * h - perp * R); d.append(perp); maxt.append(2 * R)
    return abi.make_rays(np.array(o, np.float32), np.array(d, np.float32), np.zeros(n, np.float32), np.array(maxt, np.float32),
                         rng.uniform(0, 1, n).astype(np.float32), 0.0, rng.randint(0, 9, n).astype(np.uint32))


def lights_cases():
    vh = load_scene("volumescene_h")
    none = dict(vh)
    for k in ("lights.kind", "lights.pos", "lights.dir", "lights.l2w", "lights.w2l", "lights.intensity", "lights.cos"):
        none[k] = np.asarray(vh[k])[:0]
    black = dict(vh)
    black["vol.sigma_s"] = np.zeros(30, np.float32)
    return {"point": (one_light(load_scene("sphereroom"), 1), "sph"), "spot": (one_light(load_scene("pinkfloyd"), 0), "pf"),
            "distant": (vh, "vh"), "none": (none, "vh"), "black_sigma_s": (black, "vh")}


@pytest.mark.parametrize("name", ["point", "spot", "distant", "none", "black_sigma_s"])
def test_lights(orc, name):
    s, case = lights_cases()[name]
    step = float(s["params.f"][0]) * (3.0 if case != "vh" else 1.0)   # the 0.05 of the prism and sphere rooms tripled: fewer steps, same paths
    rays, streams = golden_rays(case)
    if name == "spot":   # the prism's spot is 0.8 degrees wide: steps of 0.004 across a cone a few hundredths wide
        step, rays, streams = 0.004, spot_rays(s), abi.make_streams([3, 4], [12, 12], 0)
    ref = reference(orc, s, step, rays, streams)
    infos = ref[4]
    if name == "spot":   # the cone's edge crosses the rays: black samples (they draw nothing) beside lit ones on the same ray
        assert sum(i["black"] > 0 and i["unoccluded"] > 0 for i in infos) >= 12
    if name in ("point", "distant"):
        assert sum(i["unoccluded"] for i in infos) > 0
    if name in ("none", "black_sigma_s"):
        assert sum(i["unoccluded"] for i in infos) == 0 and (ref[0][:, :30] == 0).all() and (ref[0][:, 30:] < 1).any()
    pv = context(s, step)
    try:
        check(pv, s, rays, streams, ref, "single_par_kernel")
    finally:
        pv.close()


# ---------------------------------------------------------------- the roulette
def roulette_case_inputs():
    """sigma x 4 (sigma_t = 0.6 over a room 15 long: optical diameter 11.2 along x); rays along +x long enough for the accumulated Tr.y()
    to fall below 1e-3 (from 11.5 on), in two streams."""
    s = dict(load_scene("volumescene_h"))
    s["vol.sigma_a"] = (np.asarray(s["vol.sigma_a"]) * 4).astype(np.float32)
    s["vol.sigma_s"] = (np.asarray(s["vol.sigma_s"]) * 4).astype(np.float32)
    rng = np.random.RandomState(3)
    n = 24
    o = np.stack([np.full(n, -9.9), rng.uniform(0.5, 3.5, n), rng.uniform(0.0, 6.0, n)], 1).astype(np.float32)
    d = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    maxt = np.concatenate([rng.uniform(11.6, 13.5, n - 4), rng.uniform(2.0, 9.0, 4)]).astype(np.float32)   # the last four never get there
    rays = abi.make_rays(o, d, np.zeros(n, np.float32), maxt, rng.uniform(0, 1, n).astype(np.float32), 0.0, rng.randint(0, 9, n).astype(np.uint32))
    return s, rays, abi.make_streams([21, 22], [12, 12], [0, 5])


def test_roulette_killed_and_surviving_rays_both_paths(orc):
    s, rays, streams = roulette_case_inputs()
    step = float(s["params.f"][0])
    ref = reference(orc, s, step, rays, streams)
    infos = ref[4]
    killed = [i["killed"] for i in infos]
    survived = [i["tests"] > 0 and not i["killed"] for i in infos]
    assert sum(killed) >= 3 and sum(survived) >= 3 and sum(i["tests"] == 0 for i in infos) >= 4
    # no step's Tr.y() sits within 1e-4 of the threshold: the device's fast exponential cannot flip a comparison
    assert min(i["margin"] for i in infos) > 1e-4
    assert (ref[0][np.array(killed), 30:] == 0).all()
    seq = context(s, step, {"PVOL_FORCE_SEQ": "1"})
    try:
        _, d_seq = check(seq, s, rays, streams, ref, "single_seq_kernel")
    finally:
        seq.close()
    par = context(s, step)   # the ray-parallel form raises the redo flag and the sequential one redoes the batch
    try:
        _, d_par = check(par, s, rays, streams, ref)
        assert d_par.tobytes() == d_seq.tobytes()
    finally:
        par.close()


# ---------------------------------------------------------------- other media and entry points
def exponential_scene():
    s = dict(load_scene("volumescene_grid16"))
    s["vol.kind"] = np.array([abi.VOLUME_EXPONENTIAL], np.int32)
    del s["vol.density"]
    s["vol.exp"] = np.array([1.6, 0.45], np.float32)
    s["vol.updir"] = np.array([0, 2, 0], np.float32)
    return s


@pytest.mark.parametrize("name", ["two_lights", "grid16", "exponential"])
def test_other_media_take_the_sequential_form(orc, name):
    s, case = {"two_lights": (load_scene("pinkfloyd"), "pf"), "grid16": (load_scene("volumescene_grid16"), "grid16"),
               "exponential": (exponential_scene(), "grid16")}[name]
    step = float(s["params.f"][0]) * (3.0 if name == "two_lights" else 1.0)
    rays, streams = golden_rays(case)
    ref = reference(orc, s, step, rays, streams)
    assert sum(i["unoccluded"] for i in ref[4]) > 0
    pv = context(s, step)
    try:
        check(pv, s, rays, streams, ref, "single_seq_kernel")
    finally:
        pv.close()


def test_li_and_li_many_equal_a_lone_call_and_leave_the_reference_state(orc):
    """pvol_li with the caller's live MT19937 state, alone, through pvol_li_many and through the coalescer: the same bytes, and the
    state single.cpp would leave."""
    s = load_scene("pinkfloyd")
    step = float(s["params.f"][0]) * 3.0
    rays, _ = golden_rays("pf", 1, 6)
    states = np.stack([single_ref.MT(seed=100 + i).state() for i in range(len(rays))])
    for st, k in zip(states, (0, 5, 623, 624, 300, 17)):   # live states at various positions
        st[624] = k
    streams = abi.make_streams([0] * len(rays), [1] * len(rays), 0)
    zero_skip = rays.copy()
    zero_skip["rng_skip"] = 0   # pvol_li's contract: the state is the stream's position
    ref = reference(orc, s, step, zero_skip, streams, states=states)
    pv = context(s, step)
    try:
        lone = []
        for i in range(len(rays)):
            mt = states[i, :624].copy()
            Lv, T, mti = pv.li_single(zero_skip[i:i + 1], mt, int(states[i, 624]))
            lone.append((Lv, T, mt, mti))
            np.testing.assert_array_equal(np.concatenate([mt, [mti]]).astype(np.uint32), ref[3][i])
        got = np.stack([np.concatenate([a, b]) for a, b, _, _ in lone])
        assert single_ref.row_error(got, ref[0]).max() <= TOL
        mt = np.ascontiguousarray(states[:, :624].copy())
        Lv, T, mti, status = pv.li_many(zero_skip, mt, states[:, 624].astype(np.int32))
        assert (status == abi.PVOL_OK).all()
        for i, (a, b, m, k) in enumerate(lone):
            assert Lv[i].tobytes() == a.tobytes() and T[i].tobytes() == b.tobytes() and mt[i].tobytes() == m.tobytes() and int(mti[i]) == k
        pv.set_li_coalescing(4)
        mt0 = states[0, :624].copy()
        a, b, k = pv.li_single(zero_skip[0:1], mt0, int(states[0, 624]))
        assert a.tobytes() == lone[0][0].tobytes() and b.tobytes() == lone[0][1].tobytes() and mt0.tobytes() == lone[0][2].tobytes() and k == lone[0][3]
    finally:
        pv.close()


def test_transmittance_is_the_same_function_under_both_integrators():
    s, p, rays, streams, c = load_li_case("trans_vh")
    pv = context(s, p.step_size)
    try:
        a = pv.transmittance(rays, streams.copy())
        pv.set_volume_integrator("photonvolume")
        b = pv.transmittance(rays, streams.copy())
        assert a.tobytes() == b.tobytes() and (a < 1).any()
    finally:
        pv.close()


# ---------------------------------------------------------------- the render driver, by composition
def _render(torch, pv, cam, film, smp, tasks, n, surf=False):
    dev = torch.device("cuda:0")
    pixels = torch.zeros((film.y_resolution, film.x_resolution, 4), dtype=torch.float32, device=dev)
    rays = torch.zeros((max(n, 1), 48), dtype=torch.uint8, device=dev)
    xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    xyz = torch.zeros((max(n, 1), 4), dtype=torch.float32, device=dev)
    sxyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    streams = torch.zeros((len(tasks), 32), dtype=torch.uint8, device=dev)
    dbg = abi.RenderDebug(rays.data_ptr(), xy.data_ptr(), xyz.data_ptr(), streams.data_ptr(), sxyz.data_ptr() if surf else None)
    pv.render_tasks(cam, film, smp, tasks, pixels.data_ptr(), dbg)
    torch.cuda.synchronize()
    pv.check_errors()
    return {"pixels": pixels.cpu().numpy(), "rays": rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)[:n], "xyzT": xyz.cpu().numpy()[:n],
            "surf_xyz": sxyz.cpu().numpy()[:n], "streams": streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)}


def _li_on_render_records(pv, r):
    """pvol_li_batch (XYZ) on the rays and streams a render left: streams restart where the tasks started."""
    counts = r["streams"]["n_rays"]
    st = abi.make_streams(r["streams"]["seed"], counts, r["streams"]["start_draw"])
    out, draws = pv.li(r["rays"], st, abi.OUT_XYZ)
    return out, draws, st


def _xyz_err(got, ref):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    floor = 1e-6 * max(float(np.abs(ref).max()), 1e-30)
    return (np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), floor)).max()


def test_render_without_the_surface_integrator(torch_cuda):
    """Camera rays, rng_skip, draw counts and stream ends of a render under SINGLE are the default integrator's on the same context
    (no ray can reach the roulette: the pre-pass counts 4 + 6n + n + u under both); every sample is pvol_li_batch's."""
    s, p, cam, film, smp, c = load_render_case("vh")
    n = len(c["samples.time"])
    pv = _pvol().PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(s))
        base = _render(torch_cuda, pv, cam, film, smp, c["tasks"], n)
        np.testing.assert_array_equal(base["streams"]["end_draw"], c["task.end_draw"])
        pv.set_volume_integrator("single")
        r = _render(torch_cuda, pv, cam, film, smp, c["tasks"], n)
        assert pv.march_kernel_name() == "single_par_kernel"
        assert r["rays"].tobytes() == base["rays"].tobytes() and r["streams"].tobytes() == base["streams"].tobytes()
        out, draws, st = _li_on_render_records(pv, r)
        np.testing.assert_array_equal(st["end_draw"], r["streams"]["end_draw"])
        pv.set_volume_integrator("photonvolume")
        _, draws0, _ = _li_on_render_records(pv, base)
        np.testing.assert_array_equal(draws, draws0)
        err = _xyz_err(r["xyzT"][:, :3], out[:, :3])
        print("render under single vs pvol_li_batch on its records: %d samples, max rel L2 %.3g" % (n, err))
        assert err <= TOL and np.abs(out[:, :3]).max() > 0
        assert np.abs(r["pixels"]).max() > 0
    finally:
        pv.close()


def test_render_with_the_surface_integrator(torch_cuda):
    """sigma_a and sigma_s flat across the bins, so that T is one number per ray: the surface term is the default render's, and every
    sample is T * surf_xyz + Lvi with T and Lvi from pvol_li_batch under SINGLE."""
    from conftest import GOLD, blob
    s, p, cam, film, smp, c = load_render_case("vh_surf")
    s = dict(s)
    s["vol.sigma_a"] = np.full(30, float(np.mean(s["vol.sigma_a"])), np.float32)
    s["vol.sigma_s"] = np.full(30, float(np.mean(s["vol.sigma_s"])), np.float32)
    cb = blob.load(os.path.join(GOLD, "caustic_vh.bin"))
    n = len(c["samples.time"])
    pv = _pvol().PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.set_surface_integrator(int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), 5, bool(c["surf.params.i"][1]),
                                  (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), int(cb["n_paths"][0]))
        base = _render(torch_cuda, pv, cam, film, smp, c["tasks"], n, surf=True)
        pv.set_volume_integrator("single")
        r = _render(torch_cuda, pv, cam, film, smp, c["tasks"], n, surf=True)
        assert r["rays"].tobytes() == base["rays"].tobytes() and r["streams"].tobytes() == base["streams"].tobytes()
        assert r["surf_xyz"].tobytes() == base["surf_xyz"].tobytes() and (r["surf_xyz"].sum(1) > 0).mean() > 0.5
        out, _, st = _li_on_render_records(pv, r)
        np.testing.assert_array_equal(st["end_draw"], r["streams"]["end_draw"])
        y_ones = float(np.asarray(s["cie.y"], np.float64).sum() * 300.0 / (106.856895 * 30))
        T = out[:, 3].astype(np.float64) / y_ones
        want = T[:, None] * r["surf_xyz"].astype(np.float64) + out[:, :3]
        err = _xyz_err(r["xyzT"][:, :3], want)
        print("render under single with the surface term vs T * Ls + Lvi: %d samples, max rel L2 %.3g" % (n, err))
        assert err <= TOL
    finally:
        pv.close()


# ---------------------------------------------------------------- pvol_radiance_batch, by composition
WANT = ("surf_xyz", "t_hit", "draws", "surf_draws", "n_segments")


def _caller_rays(c, n, surf):
    """The first n camera samples of a render capture as the caller's own rays (rng_skip: the sampler's draws alone), one stream."""
    skip = c["rays.skip"].astype(np.int64) - (c["surf.draws"].astype(np.int64) if surf else 0)
    rays = abi.make_rays(c["rays.o"].reshape(-1, 3), c["rays.d"].reshape(-1, 3), c["rays.t"][0::2], np.inf, c["samples.scatter"],
                         c["samples.time"], skip.astype(np.uint32))[:n].copy()
    assert int(c["task.n_samples"][0]) >= n
    return rays, abi.make_streams(c["tasks"][:1], [n], 0)


def _radiance_composition(pv, s, rays, streams, surf):
    """pvol_radiance_batch under SINGLE beside the default integrator's on the same context, and beside pvol_li_batch under SINGLE on
    the clipped rays behind the surface draws."""
    st0 = streams.copy()
    base = pv.radiance_batch(rays, st0, abi.OUT_XYZ, WANT)
    pv.set_volume_integrator("single")
    st1 = streams.copy()
    r = pv.radiance_batch(rays, st1, abi.OUT_XYZ, WANT)
    assert pv.march_kernel_name() == "single_par_kernel"
    for k in ("t_hit", "draws", "surf_draws", "n_segments", "surf_xyz"):
        assert r[k].tobytes() == base[k].tobytes(), k
    np.testing.assert_array_equal(st1["end_draw"], st0["end_draw"])
    assert (r["surf_xyz"].sum(1) > 0).any() if surf else (r["surf_xyz"] == 0).all()
    clipped = rays.copy()
    clipped["maxt"] = r["t_hit"]
    clipped["rng_skip"] = rays["rng_skip"] + r["surf_draws"]
    st2 = streams.copy()
    out, draws = pv.li(clipped, st2, abi.OUT_XYZ)
    np.testing.assert_array_equal(draws, r["draws"])
    np.testing.assert_array_equal(st2["end_draw"], st1["end_draw"])
    y_ones = float(np.asarray(s["cie.y"], np.float64).sum() * 300.0 / (106.856895 * 30))
    T = out[:, 3].astype(np.float64) / y_ones
    want = T[:, None] * r["surf_xyz"].astype(np.float64) + out[:, :3]
    err = _xyz_err(r["L"][:, :3], want)
    np.testing.assert_allclose(r["L"][:, 3], out[:, 3], rtol=1e-4, atol=1e-7)
    print("pvol_radiance_batch under single, %d rays, surface %s: max rel L2 %.3g" % (len(rays), surf, err))
    assert err <= TOL and np.abs(out[:, :3]).max() > 0


@pytest.mark.parametrize("n", [64, 65])
def test_radiance_batch_without_the_surface_integrator(torch_cuda, n):
    s, p, cam, film, smp, c = load_render_case("vh")
    rays, streams = _caller_rays(c, n, False)
    pv = _pvol().PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(s))
        _radiance_composition(pv, s, rays, streams, False)
    finally:
        pv.close()


@pytest.mark.parametrize("n", [64, 65])
def test_radiance_batch_with_the_surface_integrator(torch_cuda, n):
    """sigma flat across the bins, so that T is one number per ray: L = T * surf_xyz + Lvi."""
    from conftest import GOLD, blob
    s, p, cam, film, smp, c = load_render_case("vh_surf")
    s = dict(s)
    s["vol.sigma_a"] = np.full(30, float(np.mean(s["vol.sigma_a"])), np.float32)
    s["vol.sigma_s"] = np.full(30, float(np.mean(s["vol.sigma_s"])), np.float32)
    cb = blob.load(os.path.join(GOLD, "caustic_vh.bin"))
    rays, streams = _caller_rays(c, n, True)
    pv = _pvol().PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.set_surface_integrator(int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), 5, bool(c["surf.params.i"][1]),
                                  (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), int(cb["n_paths"][0]))
        _radiance_composition(pv, s, rays, streams, True)
    finally:
        pv.close()


# ---------------------------------------------------------------- the render tool on the fixture
def test_render_tool_renders_the_fog_room_without_a_shoot(torch_cuda):
    import importlib.util
    from conftest import GOLD, ROOT
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(ROOT, "tools", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    log = []
    img, info = rp.render_scene_file(os.path.join(GOLD, "scenes", "single", "fog_room_single.pbrt"), log=lambda *x: log.append(" ".join(map(str, x))))
    assert info["volume_integrator"] == "single" and info["kernel"] == "single_par_kernel" and not info["surface_integrator"]
    assert info["photons"] == 0 and info["caustic_photons"] == 0 and info["indirect_photons"] == 0
    assert any("0 volume, 0 caustic, 0 indirect photons from 0 paths" in line for line in log)   # nothing was shot
    assert img.shape == (48, 48, 3) and np.isfinite(img).all() and (img.mean(axis=(0, 1)) > 0.01).all()


# ---------------------------------------------------------------- refusals
def _refused_li(pvol, pv, rays, streams):
    """pvol_li_batch answers PVOL_E_UNSUPPORTED and writes neither output nor the stream table."""
    out = np.full((len(rays), 60), 7.0, np.float32)
    draws = np.full(len(rays), 7, np.uint32)
    st = streams.copy()
    st["end_draw"] = 77
    keep = st.copy()
    import ctypes as C
    rc = pvol.lib().pvol_li_batch(pv._h, rays.ctypes.data, len(rays), st.ctypes.data, len(st), abi.OUT_SPECTRAL,
                                  out.ctypes.data_as(C.POINTER(C.c_float)), draws.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == abi.PVOL_E_UNSUPPORTED and (out == 7.0).all() and (draws == 7).all() and st.tobytes() == keep.tobytes()


def _refused_render(torch, pvol, pv, cam, film, smp, tasks, n):
    """The render driver answers PVOL_E_UNSUPPORTED and touches neither the film nor a debug record."""
    dev = torch.device("cuda:0")
    pixels = torch.full((film.y_resolution, film.x_resolution, 4), 7.0, dtype=torch.float32, device=dev)
    bufs = [torch.full(shape, 7, dtype=torch.uint8, device=dev) for shape in ((n, 48), (n, 8), (n, 16), (len(tasks), 32), (n, 12))]
    dbg = abi.RenderDebug(*[b.data_ptr() for b in bufs])
    with pytest.raises(pvol.PvolError) as e:
        pv.render_tasks(cam, film, smp, tasks, pixels.data_ptr(), dbg)
    assert e.value.status == abi.PVOL_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((pixels == 7.0).all()) and all(bool((b == 7).all()) for b in bufs)


def test_refusals_leave_the_outputs_untouched_and_a_good_render_follows(torch_cuda):
    import ctypes as C
    pvol = _pvol()
    s, p, cam, film, smp, c = load_render_case("vh")
    n = len(c["samples.time"])
    rays, streams = golden_rays("vh", 1, 8)
    # a rainbow medium: every entry point that marches
    rb = context(load_scene("volumescene_rainbow"), 0.15)
    try:
        _refused_li(pvol, rb, rays, streams)
        _refused_render(torch_cuda, pvol, rb, cam, film, smp, c["tasks"], n)
        rb.set_volume_integrator("photonvolume")   # the photon integrator still serves it
        rb.li(rays, streams.copy())
    finally:
        rb.close()
    # the render driver's limit: two lights; a density region -- pvol_li_batch serves both
    for scene in ("pinkfloyd", "volumescene_grid16"):
        q = context(load_scene(scene), 0.15)
        try:
            _refused_render(torch_cuda, pvol, q, cam, film, smp, c["tasks"], n)
            q.li(rays, streams.copy())
        finally:
            q.close()
    # a specular material with the surface integrator on: the prism room with its spot light alone
    q = context(one_light(load_scene("pinkfloyd"), 0), 0.15)
    try:
        _render(torch_cuda, q, cam, film, smp, c["tasks"], n)      # surface integrator off: served
        q.set_surface_integrator(50, 0.1)
        _refused_render(torch_cuda, pvol, q, cam, film, smp, c["tasks"], n)
        L = np.full((len(rays), 60), 3.0, np.float32)
        st = streams.copy()
        rc = pvol.lib().pvol_radiance_batch(q._h, rays.ctypes.data, len(rays), st.ctypes.data, len(st), abi.OUT_SPECTRAL, C.byref(abi.RadianceOut(L=L.ctypes.data)))
        assert rc == abi.PVOL_E_UNSUPPORTED and (L == 3.0).all() and st.tobytes() == streams.tobytes()
        q.set_surface_integrator(off=True)
        _render(torch_cuda, q, cam, film, smp, c["tasks"], n)
    finally:
        q.close()
    # a medium in which a ray can reach the roulette (R'): sigma x 4
    dense, _, _ = roulette_case_inputs()
    q = context(dense, 0.15)
    try:
        _refused_render(torch_cuda, pvol, q, cam, film, smp, c["tasks"], n)
    finally:
        q.close()
    # the final gather for caller rays, whatever else the call is -- then a good render on the same context
    pv = context(s, p.step_size)
    try:
        L = np.full((len(rays), 60), 3.0, np.float32)
        st = streams.copy()
        u = np.zeros((len(rays), 2, 3), np.float32)
        g = abi.GatherParams(max_dist=0.5, n_samples=2, cos_gather_angle=0.98, u_bsdf=u.ctypes.data, u_photon=u.ctypes.data)
        gout = abi.RadianceGatherOut(L=L.ctypes.data)
        rc = pvol.lib().pvol_radiance_gather_batch(pv._h, rays.ctypes.data, len(rays), st.ctypes.data, len(st), abi.OUT_SPECTRAL, C.byref(g), C.byref(gout))
        assert rc == abi.PVOL_E_UNSUPPORTED and (L == 3.0).all() and st.tobytes() == streams.tobytes()
        r = _render(torch_cuda, pv, cam, film, smp, c["tasks"], n)
        np.testing.assert_array_equal(r["streams"]["end_draw"], c["task.end_draw"])
        assert np.abs(r["pixels"]).max() > 0
    finally:
        pv.close()


def test_unknown_kind_and_getter(torch_cuda):
    import ctypes as C
    pvol = _pvol()
    s = load_scene("volumescene_h")
    pv = pvol.PhotonVolume(abi.params_from_blob(s))
    try:
        assert pv.volume_integrator() == "photonvolume"   # the default at pvol_create
        L = pvol.lib()
        assert L.pvol_set_volume_integrator(pv._h, 2) == abi.PVOL_E_INVALID and L.pvol_set_volume_integrator(pv._h, -1) == abi.PVOL_E_INVALID
        assert L.pvol_get_volume_integrator(pv._h, None) == abi.PVOL_E_INVALID
        assert pv.volume_integrator() == "photonvolume"
        with pytest.raises(ValueError):
            pv.set_volume_integrator("emission")
        pv.set_volume_integrator("single")
        assert pv.volume_integrator() == "single"
    finally:
        pv.close()
