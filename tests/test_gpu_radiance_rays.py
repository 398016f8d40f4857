"""pvol_radiance_batch on the device: SamplerRenderer::Li for rays the caller brings -- Scene::Intersect clip, surface
integrator with its specular recursion, volume Li(), T * Ls + Lvi -- against the reference's own records.

The committed surface captures hold, per camera sample, the ray, its scatter and time samples, rays.skip (sampler draws + the whole
surface tree), surf.draws, surf.xyz and xyzT, and per task the sample count and the stream's end.  rays.skip - surf.draws is the
caller's own rng_skip (tests/test_radiance_rays.py), so a capture is the entry point's input and every one of its outputs.

Bars: t_hit, surf_draws, n_segments and end_draw exact; radiance <= 1e-4 with test_gpu_render._rel_l2 (per-row norm, floor of 1e-4 x
the largest reference component).  No sample is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

from conftest import RENDER_SPECULAR_CASES, RENDER_SURF_CASES, abi, load_scene
from specular_depth_cases import DEPTH_CAPTURES
from test_gpu_render import _check_surface_capture, _make, _pvol, _rel_l2, _render_surface, _restore, _surface_context
from test_gpu_specular_depth import _capture_context

pytestmark = pytest.mark.gpu

WANT = abi.RADIANCE_WANT
F = np.float32
SURF_CAPTURES = ["vh_surf", "vh_surf64", "pf_surf", "sph_surf", "sph_surf_d1", "sph_surf_d2", "sphkr_surf_d3", "sphkr_surf_d5"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _context(name):
    """A context set up as the capture `name` was made, and the capture."""
    if name in DEPTH_CAPTURES:
        pv, cam, film, smp, c = _capture_context(name)
    else:
        cases = RENDER_SURF_CASES if name in RENDER_SURF_CASES else RENDER_SPECULAR_CASES
        pv, cam, film, smp, c = _surface_context(name, cases, cases[name][1])
    return pv, c


def _scene(name):
    cases = DEPTH_CAPTURES if name in DEPTH_CAPTURES else RENDER_SURF_CASES if name in RENDER_SURF_CASES else RENDER_SPECULAR_CASES
    return load_scene(cases[name][0])


def _input(c, surf=True):
    """The caller's rays and streams of a capture: rng_skip is what the sampler drew, the surface side taken out."""
    skip = c["rays.skip"].astype(np.int64) - (c["surf.draws"].astype(np.int64) if surf else 0)
    assert (skip >= 0).all()
    rays = abi.make_rays(c["rays.o"].reshape(-1, 3), c["rays.d"].reshape(-1, 3), c["rays.t"][0::2], np.inf, c["samples.scatter"],
                         c["samples.time"], skip.astype(np.uint32))
    streams = abi.make_streams(c["tasks"], c["task.n_samples"], 0)
    assert len(rays) == int(c["task.n_samples"].sum())
    return rays, streams


_RUNS = {}


def _run(name):
    """The XYZ call on the capture's input, once per capture, shared and read-only."""
    if name not in _RUNS:
        pv, c = _context(name)
        try:
            rays, streams = _input(c)
            r = pv.radiance_batch(rays, streams, abi.OUT_XYZ, WANT)
            f, i = pv.probe_hits(rays, 0)
        finally:
            pv.close()
        r["end_draw"] = streams["end_draw"].copy()
        r["probe_t"] = np.where(i[:, 0] > 0, f[:, 0], np.inf).astype(F)
        r["glass"] = (i[:, 0] > 0) & (_scene(name)["mats.kind"][i[:, 2]] == abi.MATERIAL_GLASS)
        for v in r.values():
            v.setflags(write=False)
        _RUNS[name] = (r, c, rays)
    return _RUNS[name]


def _check_capture(r, c, end_draw=True):
    np.testing.assert_array_equal(r["t_hit"], c["rays.t"][1::2])
    np.testing.assert_array_equal(r["surf_draws"], c["surf.draws"])
    if end_draw:
        np.testing.assert_array_equal(r["end_draw"], c["task.end_draw"])
    err = _rel_l2(r["L"][:, :3], c["xyzT"].reshape(-1, 4)[:, :3])
    print("T * Ls + Lvi rel L2 max %.3g" % err.max())
    assert err.max() <= 1e-4, "T * Ls + Lvi per-ray rel L2 %.3g at %d" % (err.max(), err.argmax())
    err = _rel_l2(r["surf_xyz"], c["surf.xyz"].reshape(-1, 3))
    print("Ls rel L2 max %.3g" % err.max())
    assert err.max() <= 1e-4, "surface Li per-ray rel L2 %.3g at %d" % (err.max(), err.argmax())


# ---------------------------------------------------------------- case 1: the eight surface captures
@pytest.mark.parametrize("name", SURF_CAPTURES)
def test_surface_captures(torch_cuda, name):
    r, c, rays = _run(name)
    assert 1296 <= len(rays) <= 8000
    _check_capture(r, c)
    np.testing.assert_allclose(r["L"][:, 3], c["xyzT"].reshape(-1, 4)[:, 3], rtol=1e-4, atol=1e-6)   # T.y
    np.testing.assert_array_equal(r["t_hit"], r["probe_t"])
    # Which rays spawn: the issue's rule is "n_segments > 0 exactly where surf.draws > 151".  The captures do not bear it out everywhere:
    # a spawned ray that ends inside the glass or leaves the scene meets no matte leaf, and its tree draws 23 to ~100 numbers where a
    # matte hit draws 150 -- 15 samples of pf_surf (the CPU oracle, which reproduces the capture's rays.skip bit for bit, counts 356
    # samples with spawned rays there, 341 of them above 151) and every glass sample of sph_surf_d2.  Asked instead, and no less: every
    # sample above 151 spawns; a sample spawns exactly when its closest hit is glass and maxspeculardepth > 1 (the device's own hit
    # routine, which tests/test_gpu_hit_probe.py holds to the reference); whoever spawns below 151 draws fewer than any matte hit (144).
    big = c["surf.draws"] > 151
    spawned = r["n_segments"] > 0
    if name == "sph_surf_d1":
        assert not spawned.any() and not big.any()
    else:
        np.testing.assert_array_equal(spawned, r["glass"])
        assert spawned[big].all()
        assert (c["surf.draws"][spawned & ~big] < 144).all()
        assert spawned.sum() > 20 or name.startswith("vh_")   # volumescene has no glass
        if name not in ("pf_surf", "sph_surf_d2"):
            np.testing.assert_array_equal(spawned, big)        # the issue's rule as it stands
    # every draw of every stream accounted for, ray by ray
    own = rays["rng_skip"].astype(np.uint64)
    per_ray = own + r["surf_draws"] + r["draws"]
    ends = np.add.reduceat(per_ray, np.concatenate([[0], np.cumsum(c["task.n_samples"])[:-1]]).astype(np.int64))
    np.testing.assert_array_equal(ends, c["task.end_draw"])


# ---------------------------------------------------------------- case 2: SPECTRAL output of the same call
@pytest.mark.parametrize("name", ["vh_surf", "pf_surf"])
def test_spectral_output_projects_to_the_xyz_output(torch_cuda, name):
    r, c, rays = _run(name)
    pv, _ = _context(name)
    try:
        _, streams = _input(c)
        rs = pv.radiance_batch(rays, streams, abi.OUT_SPECTRAL, WANT)
    finally:
        pv.close()
    cases = RENDER_SURF_CASES if name in RENDER_SURF_CASES else RENDER_SPECULAR_CASES
    s = load_scene(cases[name][0])
    cie = np.stack([s["cie.x"], s["cie.y"], s["cie.z"]]).astype(np.float64)
    scale = float(s["xyz_scale"][0])
    xyz = rs["L"][:, :30].astype(np.float64) @ cie.T * scale
    err = _rel_l2(xyz, r["L"][:, :3])
    assert err.max() <= 1e-5, "projection of the 30 bins against the XYZ call: %.3g" % err.max()
    ty = rs["L"][:, 30:].astype(np.float64) @ cie[1] * scale
    np.testing.assert_allclose(ty, r["L"][:, 3], rtol=1e-5, atol=1e-7)
    for k in ("t_hit", "draws", "surf_draws", "n_segments"):
        np.testing.assert_array_equal(rs[k], r[k])
    np.testing.assert_array_equal(streams["end_draw"], c["task.end_draw"])


# ---------------------------------------------------------------- case 3: no surface integrator
@pytest.mark.parametrize("name", ["vh", "grid16", "sph"])
def test_without_a_surface_integrator(torch_cuda, name):
    pv, s, p, cam, film, smp, c, old = _make(name)
    try:
        rays, streams = _input(c, surf=False)
        r = pv.radiance_batch(rays, streams, abi.OUT_XYZ, WANT)
        ref = c["xyzT"].reshape(-1, 4)
        err = _rel_l2(r["L"][:, :3], ref[:, :3])
        assert err.max() <= 1e-4, "Lvi per-ray rel L2 %.3g at %d" % (err.max(), err.argmax())
        np.testing.assert_allclose(r["L"][:, 3], ref[:, 3], rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(streams["end_draw"], c["task.end_draw"])
        assert (r["surf_draws"] == 0).all() and (r["n_segments"] == 0).all() and (r["surf_xyz"] == 0).all()
        np.testing.assert_array_equal(r["t_hit"], c["rays.t"][1::2])
        if name == "grid16":   # a surface integrator over a VolumeGrid: refused, outputs untouched
            pv.set_surface_integrator(50, 0.1)
            L = np.full((len(rays), 4), 7, F)
            t = np.full(len(rays), 7, F)
            st = abi.make_streams(c["tasks"], c["task.n_samples"], 0)
            st["end_draw"] = 77
            out = abi.RadianceOut(L=L.ctypes.data, t_hit=t.ctypes.data)
            rc = _pvol().lib().pvol_radiance_batch(pv._h, rays.ctypes.data, len(rays), st.ctypes.data, len(st), abi.OUT_XYZ, C.byref(out))
            assert rc == abi.PVOL_E_UNSUPPORTED
            assert (L == 7).all() and (t == 7).all() and (st["end_draw"] == 77).all()
    finally:
        pv.close()
        _restore(old)


# ---------------------------------------------------------------- case 4: order
def test_order_of_the_rays_does_not_reach_a_result(torch_cuda):
    """vh_surf: one light over a homogeneous extent, so no drawn value reaches a result.  The rays of each stream reversed, and all
    rays in a single stream: per ray the same radiance (the capture's bar), the same surf_draws and t_hit."""
    r, c, rays = _run("vh_surf")
    pv, _ = _context("vh_surf")
    try:
        first = np.concatenate([[0], np.cumsum(c["task.n_samples"])]).astype(np.int64)
        perm = np.concatenate([np.arange(first[i + 1] - 1, first[i] - 1, -1) for i in range(len(first) - 1)])
        assert sorted(perm.tolist()) == list(range(len(rays))) and perm[0] == first[1] - 1
        _, streams = _input(c)
        rr = pv.radiance_batch(rays[perm], streams, abi.OUT_XYZ, WANT)
        inv = np.argsort(perm)
        rr = {k: v[inv] for k, v in rr.items()}
        _check_capture(rr, c, end_draw=False)
        np.testing.assert_array_equal(streams["end_draw"], c["task.end_draw"])   # the same draws in another order
        one = abi.make_streams([3], [len(rays)], 0)
        r1 = pv.radiance_batch(rays, one, abi.OUT_XYZ, WANT)
        _check_capture(r1, c, end_draw=False)
        assert int(one["end_draw"][0]) == int(c["task.end_draw"].sum())
    finally:
        pv.close()


# ---------------------------------------------------------------- case 5: rays no camera makes, on sphereroom
def test_rays_no_camera_makes(torch_cuda):
    r, c, rays = _run("sph_surf")
    pv, _ = _context("sph_surf")
    try:
        def call(rr, seed=5, kind=abi.OUT_XYZ):
            st = abi.make_streams([seed], [len(rr)], 0)
            out = pv.radiance_batch(rr, st, kind, WANT)
            out["end_draw"] = st["end_draw"].copy()
            return out
        # a ray that leaves the scene: the room has no ceiling
        up = abi.make_rays(F([[0, 0, 0]]), F([[0, 1, 0]]), 0.0, np.inf, 0.5, 0.25, 3)
        f, i = pv.probe_hits(up, 0)
        assert i[0, 0] == 0
        o = call(up)
        assert np.isinf(o["t_hit"][0]) and o["surf_draws"][0] == 0 and o["n_segments"][0] == 0 and (o["surf_xyz"] == 0).all()
        assert int(o["end_draw"][0]) == 3 + int(o["draws"][0])
        # a ray that points at a matte wall, ending 1e-3 before it: no surface term, the volume term of pvol_li_batch on the same ray
        wall = int(np.flatnonzero((c["surf.draws"] <= 151) & (c["surf.draws"] > 0) & (c["surf.xyz"].reshape(-1, 3).sum(1) > 0))[0])
        t_wall = float(c["rays.t"][1::2][wall])
        short = rays[wall:wall + 1].copy()
        short["maxt"] = F(t_wall - 1e-3)
        o = call(short)
        assert o["t_hit"][0] == short["maxt"][0] and o["surf_draws"][0] == 0 and (o["surf_xyz"] == 0).all()
        st = abi.make_streams([5], [1], 0)
        li, li_draws = pv.li(short, st, abi.OUT_XYZ)
        assert _rel_l2(o["L"][:, :3], li[:, :3]).max() <= 1e-5 and abs(o["L"][0, 3] - li[0, 3]) <= 1e-5 * li[0, 3]
        assert o["draws"][0] == li_draws[0] and int(o["end_draw"][0]) == int(st["end_draw"][0])
        # the same ray to infinity: the wall's radiance on top, and the surface integrator's draws
        full = short.copy()
        full["maxt"] = np.inf
        of = call(full)
        assert of["t_hit"][0] == F(t_wall) and of["surf_draws"][0] == c["surf.draws"][wall] > 0
        assert of["L"][0, :3].sum() > o["L"][0, :3].sum() and of["surf_xyz"][0].sum() > 0
        # a ray starting inside the glass ball (radius 0.6 about (-1, 1, 3.5)): it meets the glass from within
        inside = abi.make_rays(F([[-1, 1, 3.5]]), F([[0, 0, 1]]), 0.0, np.inf, 0.5, 0.25, 0)
        f, i = pv.probe_hits(inside, 0)
        oi = call(inside)
        assert i[0, 0] == 1 and oi["t_hit"][0] == f[0, 0] <= F(0.6001) and oi["n_segments"][0] >= 1 and oi["surf_draws"][0] >= 6
        assert np.isfinite(oi["L"]).all() and oi["L"][0, 3] > 0
        # n_rays in {1, 63, 64, 65}: the head of task 5's stream is the head of the capture, one stream holding one ray included
        own = rays["rng_skip"].astype(np.uint64)
        for n in (1, 63, 64, 65):
            o = call(rays[:n], seed=int(c["tasks"][0]))
            for k in ("t_hit", "surf_draws", "n_segments", "draws"):
                np.testing.assert_array_equal(o[k], r[k][:n])
            assert _rel_l2(o["L"][:, :3], c["xyzT"].reshape(-1, 4)[:n, :3]).max() <= 1e-4
            assert int(o["end_draw"][0]) == int((own[:n] + r["surf_draws"][:n] + r["draws"][:n]).sum())
    finally:
        pv.close()


# ---------------------------------------------------------------- case 6: slices, host and device form, repeats
def _device_call(torch, pv, rays, streams, kind):
    dev = torch.device("cuda:0")
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 48).copy()).to(dev)
    d_streams = torch.from_numpy(streams.view(np.uint8).reshape(len(streams), 32).copy()).to(dev)
    d = {"L": torch.zeros((n, 60 if kind == abi.OUT_SPECTRAL else 4), dtype=torch.float32, device=dev),
         "surf_xyz": torch.zeros((n, 3), dtype=torch.float32, device=dev), "t_hit": torch.zeros(n, dtype=torch.float32, device=dev)}
    for k in ("draws", "surf_draws", "n_segments"):
        d[k] = torch.zeros(n, dtype=torch.int32, device=dev)
    pv.radiance_batch_device(d_rays.data_ptr(), n, d_streams.data_ptr(), len(streams), kind, d["L"].data_ptr(),
                             hip_stream=torch.cuda.current_stream().cuda_stream, **{k: d[k].data_ptr() for k in WANT})
    torch.cuda.synchronize()
    pv.check_errors()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    for k in ("draws", "surf_draws", "n_segments"):
        out[k] = out[k].view(np.uint32)
    out["end_draw"] = d_streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)["end_draw"].copy()
    return out


def _same(a, b, tol=5e-6):
    for k in ("t_hit", "draws", "surf_draws", "n_segments", "end_draw"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("L", "surf_xyz"):
        ref = np.abs(b[k]).astype(np.float64)
        err = np.abs(a[k].astype(np.float64) - b[k]) / np.maximum(ref, 1e-4 * ref.max())
        assert err.max() <= tol, "%s differs by %.3g relative" % (k, err.max())


def test_slices_and_forms_agree(torch_cuda):
    """pf_surf (356 rays own trees) with the scratch bound lowered to what 640 rays need when none spawns: a slice is a candidate of 640
    rays cut back to the run whose counted blocks fit, so at least five slices, the first boundary inside the first stream (676 rays).
    Every integer equals the unsliced call, L within 5e-6 relative (the bar between repeats)."""
    r, c, rays = _run("pf_surf")
    pvol = _pvol()
    pv, _ = _context("pf_surf")
    try:
        per = abi.RADIANCE_RAY_SCRATCH + abi.RADIANCE_CALLER_SCRATCH   # a ray that spawns nothing
        m = 640
        assert pvol.lib().pvol_radiance_slice(0, per * m) == m
        assert -(-len(rays) // m) >= 3 and m < int(c["task.n_samples"][0])
        trees = int((r["n_segments"][:m] > 0).sum() + (r["n_segments"][1352:1352 + m] > 0).sum())
        assert trees > 0   # some candidate has to be cut back
        _, streams = _input(c)
        pv.radiance_set_scratch_bound(per * m)
        sliced = pv.radiance_batch(rays, streams, abi.OUT_XYZ, WANT)
        sliced["end_draw"] = streams["end_draw"].copy()
        _same(sliced, r)
        dev_sliced = _device_call(torch_cuda, pv, rays, _input(c)[1], abi.OUT_XYZ)
        _same(dev_sliced, r)
        pv.radiance_set_scratch_bound(per * 64)   # 43 slices or more, of 64 rays and fewer (one ray a slice would be 2 704 synchronisations)
        _same(_device_call(torch_cuda, pv, rays, _input(c)[1], abi.OUT_XYZ), r)
        pv.radiance_set_scratch_bound(0)
        dev = _device_call(torch_cuda, pv, rays, _input(c)[1], abi.OUT_XYZ)
        _same(dev, r)
        _same(_device_call(torch_cuda, pv, rays, _input(c)[1], abi.OUT_XYZ), dev)
        _check_capture(dev, c)
    finally:
        pv.close()


# ---------------------------------------------------------------- case 7: what does not change
def test_rejected_calls_write_nothing_and_the_render_is_undisturbed(torch_cuda):
    r, c, rays = _run("vh_surf")
    L = _pvol().lib()
    pv, cam, film, smp, c = _surface_context("vh_surf", RENDER_SURF_CASES, "vh")
    try:
        n = len(rays)
        bufs = {k: np.full((n, 4), 7, F) for k in ("L", "surf_xyz", "t_hit", "draws", "surf_draws", "n_segments")}
        out = abi.RadianceOut(**{k: v.ctypes.data for k, v in bufs.items()})
        _, streams = _input(c)
        streams["end_draw"] = 77

        def untouched():
            return all((v == 7).all() for v in bufs.values()) and (streams["end_draw"] == 77).all()
        call = L.pvol_radiance_batch
        assert call(None, rays.ctypes.data, n, streams.ctypes.data, len(streams), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_E_INVALID
        assert call(pv._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), 2, C.byref(out)) == abi.PVOL_E_INVALID
        assert call(pv._h, None, n, streams.ctypes.data, len(streams), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_E_INVALID
        assert call(pv._h, rays.ctypes.data, n, None, len(streams), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_E_INVALID
        assert call(pv._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), abi.OUT_XYZ, None) == abi.PVOL_E_INVALID
        no_l = abi.RadianceOut(t_hit=bufs["t_hit"].ctypes.data)
        assert call(pv._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), abi.OUT_XYZ, C.byref(no_l)) == abi.PVOL_E_INVALID
        bad = streams.copy()
        bad["n_rays"][0] -= 1   # the streams no longer partition the rays
        bad_before = bad.copy()
        assert call(pv._h, rays.ctypes.data, n, bad.ctypes.data, len(bad), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_E_INVALID
        assert (bad == bad_before).all()
        assert call(pv._h, rays.ctypes.data, 0, streams.ctypes.data, len(streams), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_OK
        assert call(pv._h, rays.ctypes.data, n, streams.ctypes.data, 0, abi.OUT_XYZ, C.byref(out)) == abi.PVOL_OK
        assert untouched()
        bare = _pvol().PhotonVolume(abi.params_from_blob(load_scene("volumescene_h")))
        try:
            assert call(bare._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), abi.OUT_XYZ, C.byref(out)) == abi.PVOL_E_NO_SCENE
        finally:
            bare.close()
        assert untouched()
        # a radiance call, then a render through the tile driver on the same context: its scratch and segment pool are its own
        _, streams = _input(c)
        got = pv.radiance_batch(rays, streams, abi.OUT_XYZ, WANT)
        got["end_draw"] = streams["end_draw"].copy()
        _check_capture(got, c)
        rr = _render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], n)
        _check_surface_capture(rr, c, film)
        np.testing.assert_array_equal(rr["rays"]["rng_skip"].astype(np.int64) - got["surf_draws"], rays["rng_skip"])
    finally:
        pv.close()
