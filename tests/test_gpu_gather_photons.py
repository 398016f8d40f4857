"""The final gather's sampling half on the device: pvol_gather_photons* and pvol_gather_directions* through the C
ABI against tests/gather_ref.py.  Index arrays, d2, found and rounds are compared for equality, ties included; wi, pdfs and weights
to 1e-4 relative L2 (floor 1e-6 of the largest), leaving out at most 0.5 % of the samples, those whose decision the yardstick sees
within 1e-5 of its threshold."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import abi

import gather_ref as gr
from test_gather_photons import doubled_set, lattice_set, planar_set

pytestmark = pytest.mark.gpu
F = np.float32
K = gr.K
SCENES = os.path.join(os.path.dirname(__file__), "golden", "indirect")


@pytest.fixture(scope="module")
def pvol():
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1
    return m


def _bare_context(pvol):
    p = abi.Params()
    pvol.lib().pvol_default_params(C.byref(p))
    return pvol.PhotonVolume(p)   # no scene: pvol_build_gather_map_arrays needs none


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _d2(P, q):
    dv = np.asarray(P, F) - np.asarray(q, F)
    return (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]


def _assert_lookup_equal(got, want, what):
    for g, w, name in zip(got, want, ("index", "d2", "found", "rounds")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differs for %d of %d queries, first %d: got %s want %s" % (what, name, bad.size, len(g), bad[0], g[bad[0]], w[bad[0]])


class RandomCase:
    """5 000 uniform photons plus a 3 000-photon clump (sigma 0.01); 1 000 queries, half near photons, half uniform.  The yardstick's
    lookups are computed once per max_dist and shared."""

    def __init__(self):
        rng = np.random.default_rng(20261019)
        clump = F([0.3, 0.6, 0.4]) + rng.normal(size=(3000, 3)) * 0.01
        self.P = np.concatenate([rng.random((5000, 3)), clump]).astype(F)[rng.permutation(8000)]
        self.W = _unit(rng.normal(size=(8000, 3)))
        near = self.P[rng.integers(0, 8000, 500)] + rng.normal(size=(500, 3)).astype(F) * F(0.004)
        self.Q = np.concatenate([near, rng.random((500, 3))]).astype(F)
        self.tree = gr.Tree(self.P)
        self._ref = {}

    def ref(self, max_dist, count=None):
        key = (max_dist, count)
        if key not in self._ref:
            self._ref[key] = self.tree.lookup_many(self.Q[:count], max_dist)
        return self._ref[key]


@pytest.fixture(scope="module")
def random_case():
    return RandomCase()


# ---------------------------------------------------------------------------------------------- 1. ladder
@pytest.mark.parametrize("n", [50, 51, 64])
def test_ladder_of_small_maps_and_rounds(pvol, n):
    """A map of exactly 50 photons (no pop ever happens), of 51, and of 64 on a jittered 4 x 4 x 4 lattice; from the centre the
    yardstick shows rounds = 1, rounds = 2 with 49 photons in the first ball, and rounds >= 4 with an empty first ball."""
    rng = np.random.default_rng(n)
    if n == 64:
        g = (np.arange(4) + 0.5) / 4
        P = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (64, 3))).astype(F)
    else:
        P = rng.random((n, 3)).astype(F)
    W = _unit(rng.normal(size=(n, 3)))
    T = gr.Tree(P)
    q0 = F([0.5, 0.5, 0.5])
    d2 = np.sort(_d2(P, q0))
    assert len(np.unique(d2)) == n
    Q = np.concatenate([[q0], [P[7]], [[100, 100, 100]], rng.random((5, 3))]).astype(F)
    md_two = float(np.sqrt(np.float64(d2[49])) * 0.9995)
    md_far = float(np.sqrt(np.float64(d2[0])) / 4)
    cases = []
    for max_dist, want_rounds in ((2.0, 1), (md_two, 2), (md_far, None)):
        ref = T.lookup_many(Q, max_dist)
        first_ball = int((_d2(P, q0) < F(max_dist) * F(max_dist)).sum())
        if want_rounds == 1:
            assert ref[3][0] == 1 and first_ball == n
        elif want_rounds == 2:
            assert ref[3][0] == 2 and first_ball == 49
        else:
            assert ref[3][0] >= 4 and first_ball == 0
        assert (ref[2] == K).all()
        assert ref[3][2] > ref[3][0]   # the far query needs more doublings than the centre
        cases.append((max_dist, ref))
    pv = _bare_context(pvol)
    try:
        assert pv.build_gather_map((P, W)) == n
        for max_dist, ref in cases:
            _assert_lookup_equal(pv.gather_photons(Q, max_dist), ref, "n %d max_dist %g" % (n, max_dist))
    finally:
        pv.close()


# ---------------------------------------------------------------------------------------------- 2. random
@pytest.mark.parametrize("max_dist", [0.02, 0.2])
def test_random_map_with_a_clump(pvol, random_case, max_dist):
    rc = random_case
    ref = rc.ref(max_dist)
    assert (ref[2] == K).all() and ref[3].min() == 1
    if max_dist == 0.02:
        assert ref[3].max() >= 3   # sparse places double more than once
    pv = _bare_context(pvol)
    try:
        pv.build_gather_map((rc.P, rc.W))
        _assert_lookup_equal(pv.gather_photons(rc.Q, max_dist), ref, "random max_dist %g" % max_dist)
    finally:
        pv.close()


# ---------------------------------------------------------------------------------------------- 3. ties, decided
def _tie_case(name):
    rng = np.random.default_rng(33)
    if name == "planar":
        P = planar_set(rng)
        on_grid = np.concatenate([np.full((40, 1), 5.0), rng.integers(0, 32, (40, 2)) / 32.0], axis=1)
        Q = np.concatenate([P[:40], on_grid, P[:20] + F([0.25, 0, 0])]).astype(F)
    elif name == "doubled":
        P = doubled_set(rng)
        Q = np.concatenate([P[:60], rng.random((40, 3))]).astype(F)
    else:
        P = lattice_set(8)
        Q = np.concatenate([P[rng.integers(0, len(P), 80)], P[:20] + F(1 / 16)]).astype(F)
    return P.astype(F), Q


@pytest.mark.parametrize("name", ["planar", "doubled", "lattice"])
def test_ties_are_decided_exactly(pvol, name):
    P, Q = _tie_case(name)
    W = _unit(np.random.default_rng(4).normal(size=(len(P), 3)))
    T = gr.Tree(P)
    tied_queries = tied_at_50 = 0
    for q in Q:
        d2 = np.sort(_d2(P, q))
        tied_queries += int(len(np.unique(d2[:60])) < 60)
        tied_at_50 += int(d2[49] == d2[50])
    # equal d2 for most queries; at the 50th place too, except in the doubled set, whose twins pair up as (49th, 50th), (51st, 52nd)
    assert tied_queries >= len(Q) // 2 and (tied_at_50 >= 10 or name == "doubled"), (tied_queries, tied_at_50)
    refs = [(md, T.lookup_many(Q, md)) for md in (0.1, 0.4)]
    pv = _bare_context(pvol)
    try:
        pv.build_gather_map((P, W))
        for md, ref in refs:
            assert (ref[2] == K).all()
            _assert_lookup_equal(pv.gather_photons(Q, md), ref, "%s max_dist %g" % (name, md))
    finally:
        pv.close()


# ---------------------------------------------------------------------------------------------- 4. end to end
def test_kept_indirect_store_end_to_end(pvol, orc):
    """room_indirect.pbrt at the sizes of test_gpu_surface_indirect.py's end-to-end test: the map from the store the shoot kept,
    queried at the oracle's hits of one camera ray per pixel at 48 x 32; the yardstick runs on the downloaded store."""
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    scene = ps.load(os.path.join(SCENES, "room_indirect.pbrt"))
    xres, yres = 48, 32
    params = abi.params_from_blob(scene, n_volume_photons=20000, keep_surface_photons=1)
    cam = abi.perspective_camera(float(scene["camera.fov"][0]), xres, yres, scene["camera.c2w"])
    xy = np.stack(np.meshgrid(np.arange(xres) + 0.5, np.arange(yres) + 0.5), -1).reshape(-1, 2).astype(F)
    rays = orc.camera_rays(cam, xy)
    holder = abi.SceneHolder(scene)
    f, _ = orc.Oracle(holder, params).hits(rays["o"], rays["d"], rays["mint"], np.full(len(rays), np.inf, F))
    hit = (f[:, 0] != 0) & (f[:, 1] != 0)
    Q = np.ascontiguousarray(f[hit, 3:6], F)
    assert len(Q) > 1000
    max_dist = 0.5
    pv = pvol.PhotonVolume(params)
    try:
        pv.set_scene(holder)
        pv.preprocess(64)
        ip, iw, ia, ipaths = pv.surface_photons(2)
        assert len(ip) >= 2000
        T = gr.Tree(ip)
        ref = T.lookup_many(Q, max_dist)
        assert (ref[2] == K).all()
        assert pv.build_gather_map() == len(ip)
        got = pv.gather_photons(Q, max_dist)
        _assert_lookup_equal(got, ref, "room_indirect")
        print("room_indirect: %d indirect photons, %d queries, rounds %d..%d" % (len(ip), len(Q), ref[3].min(), ref[3].max()))
    finally:
        pv.close()


# ---------------------------------------------------------------------------------------------- 5. directions
def _frames(rng, count):
    """Random frames: nn, dpdu orthogonal to it (scaled: the constructor normalises), ng = +nn, -nn or tilted by up to ~35 degrees;
    wo on both sides of the surface."""
    nn = _unit(rng.normal(size=(count, 3)))
    t = rng.normal(size=(count, 3))
    dpdu = (t - (t * nn).sum(1, keepdims=True) * nn) * rng.uniform(0.5, 3.0, (count, 1))
    kind = np.arange(count) % 3
    tilted = _unit(nn + 0.7 * rng.uniform(-1, 1, (count, 3)))
    ng = np.where((kind == 0)[:, None], nn, np.where((kind == 1)[:, None], -nn, tilted))
    wo = _unit(rng.normal(size=(count, 3)))
    return np.concatenate([nn, dpdu, ng], axis=1).astype(F), wo


def _rel(a, b, floor):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim == 1:
        a, b = a[:, None], b[:, None]
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), floor)


@pytest.mark.parametrize("n_samples,angle", [(1, 10.0), (16, 10.0), (1, 60.0), (16, 60.0)])
def test_directions_and_weights(pvol, random_case, n_samples, angle):
    rc = random_case
    count, max_dist = 512, 0.2
    rng = np.random.default_rng(int(1000 * angle) + n_samples)
    frames, wo = _frames(rng, count)
    u_b, u_p = rng.random((count, n_samples, 3)).astype(F), rng.random((count, n_samples, 3)).astype(F)
    cos_g = pvol.gather_cos_angle(angle)
    assert cos_g == gr.cos_gather_angle(angle)
    index = rc.ref(max_dist)[0][:count]
    want_b, want_p, margin_b, margin_p = gr.directions(rc.W, index, frames, wo, cos_g, u_b, u_p)
    # what the yardstick alone says about its inputs, before the GPU is touched
    skip_b, skip_p = margin_b < 1e-5, margin_p < 1e-5
    total = 2 * count * n_samples
    assert skip_b.sum() + skip_p.sum() <= 0.005 * total, (int(skip_b.sum()), int(skip_p.sum()), total)
    assert 0 < want_p["valid"].sum() < count * n_samples            # invalid samples occur: photons arrive from both sides
    assert (want_b["valid"] == 0).any() and (want_b["valid"] == 1).any()   # the tilted ng turns some BSDF samples black
    assert (wo * frames[:, 0:3]).sum(1).min() < 0 < (wo * frames[:, 0:3]).sum(1).max()
    n_in_cone = np.round(want_p["photon_pdf"][want_p["valid"] == 1] * K * (2 * np.pi * (1 - cos_g)))
    assert n_in_cone.min() >= 1
    if angle == 60.0:
        assert n_in_cone.max() > 1                                   # cones overlap: counts exceed 1
    pv = _bare_context(pvol)
    try:
        pv.build_gather_map((rc.P, rc.W))
        got_b, got_p = pv.gather_directions(rc.Q[:count], frames, wo, max_dist, cos_g, u_b, u_p)
    finally:
        pv.close()
    worst = {}
    for name, got, want, skip in (("bsdf", got_b, want_b, skip_b), ("photon", got_p, want_p, skip_p)):
        keep = ~skip
        np.testing.assert_array_equal(got["photon_index"], want["photon_index"], err_msg=name)   # photonNum and the chosen photon: exact
        np.testing.assert_array_equal(got["valid"][keep], want["valid"][keep], err_msg=name)
        g, w = got[keep], want[keep]
        assert np.isfinite(g["wi"]).all()
        for field in ("wi", "weight", "bsdf_pdf", "photon_pdf"):
            fin = np.isfinite(w[field]).reshape(len(w), -1).all(axis=1)
            floor = 1e-6 * float(np.abs(w[field][fin]).max())
            err = _rel(g[field][fin], w[field][fin], floor)
            worst[name + "." + field] = float(err.max())
            np.testing.assert_array_equal(np.isfinite(g[field]).reshape(len(g), -1).all(axis=1), fin)
    print("directions n_samples %d angle %g: left out %d of %d; largest errors %s" % (
        n_samples, angle, int(skip_b.sum() + skip_p.sum()), total, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1e-4, worst


# ---------------------------------------------------------------------------------------------- 6. forms and life cycle
def _device_lookup(pv, torch, Q, max_dist):
    n = len(Q)
    dq = torch.from_numpy(np.ascontiguousarray(Q, F)).cuda()
    di = torch.full((n, K), 7, dtype=torch.int32, device="cuda")
    dd = torch.full((n, K), -1.0, dtype=torch.float32, device="cuda")
    df = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dr = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    pv.gather_photons_device(dq.data_ptr(), n, max_dist, di.data_ptr(), dd.data_ptr(), df.data_ptr(), dr.data_ptr(), 0)
    torch.cuda.synchronize()
    return (di.cpu().numpy().view(np.uint32), dd.cpu().numpy(), df.cpu().numpy().view(np.uint32), dr.cpu().numpy().view(np.uint32))


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_forms_and_life_cycle(pvol, random_case):
    import torch
    rc = random_case
    count, max_dist = 256, 0.2
    Q = rc.Q[:count].copy()
    ref = tuple(x[:count] for x in rc.ref(max_dist))
    rng = np.random.default_rng(6)
    frames, wo = _frames(rng, count)
    u_b, u_p = rng.random((count, 4, 3)).astype(F), rng.random((count, 4, 3)).astype(F)
    cos_g = pvol.gather_cos_angle(10.0)
    pv = _bare_context(pvol)
    try:
        # before any build
        assert pv.gather_map_count() == 0
        with pytest.raises(pvol.PvolError) as e:
            pv.gather_photons(Q, max_dist)
        assert e.value.status == abi.PVOL_E_INVALID
        assert pv.build_gather_map((rc.P, rc.W)) == len(rc.P)
        host = pv.gather_photons(Q, max_dist)
        _assert_lookup_equal(host, ref, "host form")
        # host and device entry points are byte-equal; two runs are byte-equal (no atomics are involved)
        assert _same(_device_lookup(pv, torch, Q, max_dist), host)
        assert _same(pv.gather_photons(Q, max_dist), host)
        dirs = pv.gather_directions(Q, frames, wo, max_dist, cos_g, u_b, u_p)
        assert _same(pv.gather_directions(Q, frames, wo, max_dist, cos_g, u_b, u_p), dirs)
        d_in = [torch.from_numpy(np.ascontiguousarray(x, F)).cuda() for x in (Q, frames, wo, u_b, u_p)]
        d_out = [torch.full((count, 4, 8), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        pv.gather_directions_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), count, max_dist, 4, cos_g, d_in[3].data_ptr(),
                                    d_in[4].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), 0)
        torch.cuda.synchronize()
        assert _same([t.cpu().numpy() for t in d_out], dirs)
        # a non-finite query ends with found < 50, a zeroed tail, and PVOL_OK; its neighbours are untouched
        Qn = Q[:8].copy()
        Qn[1] = [np.nan, 0.5, 0.5]
        Qn[4] = [0.5, np.inf, 0.5]
        Qn[6] = [3e38, -3e38, 3e38]   # finite, but every d2 overflows to +inf
        gi, gd, gf, gr_ = pv.gather_photons(Qn, max_dist)
        for bad in (1, 4, 6):
            assert gf[bad] < K and (gi[bad, gf[bad]:] == 0).all() and (gd[bad, gf[bad]:] == 0).all()
            assert gf[bad] == 0 and 1 <= gr_[bad] <= 300
        ok = [0, 2, 3, 5, 7]
        assert _same([x[ok] for x in (gi, gd, gf, gr_)], [x[ok] for x in host])
        db, dp = pv.gather_directions(Qn, frames[:8], wo[:8], max_dist, cos_g, u_b[:8], u_p[:8])
        for bad in (1, 4, 6):
            assert (db["valid"][bad] == 0).all() and (dp["valid"][bad] == 0).all() and (db["weight"][bad] == 0).all()
        # rejected calls leave the previous map answering with the same bytes
        nan_p = rc.P.copy()
        nan_p[100, 2] = np.nan
        for arrays, status in (((nan_p, rc.W), abi.PVOL_E_INVALID), ((rc.P[:49], rc.W[:49]), abi.PVOL_E_UNSUPPORTED)):
            with pytest.raises(pvol.PvolError) as e:
                pv.build_gather_map(arrays)
            assert e.value.status == status
            assert pv.gather_map_count() == len(rc.P) and _same(pv.gather_photons(Q, max_dist), host)
        with pytest.raises(pvol.PvolError) as e:
            pv.build_gather_map()   # this context kept no stores
        assert e.value.status == abi.PVOL_E_INVALID
        for bad_dist in (0.0, float("nan"), 1e-30):
            with pytest.raises(pvol.PvolError) as e:
                pv.gather_photons(Q, bad_dist)
            assert e.value.status == abi.PVOL_E_INVALID
        with pytest.raises(pvol.PvolError) as e:
            pv.gather_directions(Q, frames, wo, max_dist, 1.0, u_b, u_p)
        assert e.value.status == abi.PVOL_E_INVALID
        assert _same(pv.gather_photons(Q, max_dist), host)
        # replacement: the map of the first 4 000 photons answers as its own yardstick does
        half = gr.Tree(rc.P[:4000])
        ref_half = half.lookup_many(Q[:64], max_dist)
        assert pv.build_gather_map((rc.P[:4000], rc.W[:4000])) == 4000
        _assert_lookup_equal(pv.gather_photons(Q[:64], max_dist), ref_half, "replaced map")
        assert not _same([x[:64] for x in host], ref_half)
    finally:
        pv.close()


def test_a_new_shoot_drops_the_map(pvol):
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    scene = ps.load(os.path.join(SCENES, "room_indirect.pbrt"))
    params = abi.params_from_blob(scene, n_volume_photons=2000, keep_surface_photons=1)
    rng = np.random.default_rng(8)
    P, W = rng.random((200, 3)).astype(F), _unit(rng.normal(size=(200, 3)))
    Q = rng.random((16, 3)).astype(F)
    pv = pvol.PhotonVolume(params)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.build_gather_map((P, W))
        assert pv.gather_photons(Q, 0.3)[2].tolist() == [K] * 16
        pv.preprocess(8)
        assert pv.gather_map_count() == 0
        with pytest.raises(pvol.PvolError) as e:
            pv.gather_photons(Q, 0.3)
        assert e.value.status == abi.PVOL_E_INVALID
        if len(pv.surface_photons(2)[0]) >= K:
            assert pv.build_gather_map() == len(pv.surface_photons(2)[0])
            assert (pv.gather_photons(Q, 0.3)[2] == K).all()
    finally:
        pv.close()
