"""Radiance photons on the device: pvol_compute_radiance* against the numpy restatement of ComputeRadianceTask
(radiance_ref.py; the oracle does not know the task), and pvol_radiance_lookup* against the restatement's nearest facing photon.
Bars: Lo <= 1e-4 relative L2 over the 30 bins per radiance photon (floor: 1e-6 of the largest value); lookups exact.  Every test
checks its inputs for exact float32 ties on the CPU before it touches the GPU (DESIGN.md 2 "Ties")."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import abi, load_scene

import radiance_ref as rr

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def pvol():
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1
    return m


def _bare_context(pvol):
    p = abi.Params()
    pvol.lib().pvol_default_params(C.byref(p))
    return pvol.PhotonVolume(p)   # no scene: pvol_compute_radiance_arrays needs none


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _check_lo(got, ref, what):
    err = rr.lo_error(got, ref)
    print("%s: max rel L2 of Lo %.3g over %d radiance photons" % (what, float(err.max()) if err.size else 0.0, len(err)))
    assert np.isfinite(got).all()
    assert err.size == 0 or err.max() <= 1e-4


# ---------------------------------------------------------------------------------------------- 1. counts ladder
def _ladder_map(m, rng, max_dist):
    """m photons at distinct distances inside the ball around the origin, one at exactly max_dist^2, five beyond."""
    radii = (0.04 + 0.8 * (np.arange(m) + 0.5) / max(m, 1)) * max_dist
    P = _unit(rng.normal(size=(m, 3))) * radii[:, None].astype(F32)
    P = np.concatenate([P, [[max_dist, 0, 0]], _unit(rng.normal(size=(5, 3))) * F32(max_dist) * np.linspace(1.05, 2.0, 5)[:, None]]).astype(F32)
    W = _unit(rng.normal(size=(len(P), 3)) + [0, 0, 0.2])
    W[:, 2] = np.where(np.arange(len(P)) % 2 == 0, np.abs(W[:, 2]), -np.abs(W[:, 2]))   # half above, half below the plane
    rank = np.argsort(rr.d2_f32(P, np.zeros(3, F32)))
    for r in rank[1:3]:   # the second and third nearest lie IN the plane: Dot == 0 exactly, they count for neither side
        W[r] = [1, 0, 0] if r % 2 else [0, -1, 0]
    A = (rng.random((len(P), 30)) + 0.1).astype(F32)
    perm = rng.permutation(len(P))
    return P[perm], W[perm], A[perm]


@pytest.mark.parametrize("k", [1, 50])
def test_counts_ladder_pins_md2_and_the_strict_visit_test(pvol, k):
    rng = np.random.default_rng(100 + k)
    max_dist = 0.25
    md2 = F32(max_dist) * F32(max_dist)
    rp_p, rp_n = np.zeros((1, 3), F32), np.array([[0, 0, 1]], F32)
    rho_r, rho_t = (rng.random((1, 30)) + 0.1).astype(F32), (rng.random((1, 30)) + 0.1).astype(F32)
    cases = []
    for m in sorted({0, 1, k - 1, k, k + 1, 3 * k}):
        P, W, A = _ladder_map(m, rng, max_dist)
        d2 = rr.d2_f32(P, rp_p[0])
        assert int((d2 < md2).sum()) == m and int((d2 == md2).sum()) == 1 and int((d2 > md2).sum()) == 5
        assert len(np.unique(d2)) == len(d2)   # no tie
        dots = rr.dot_f32(rp_n[0], W)
        assert int((dots == 0).sum()) == 2 and (dots > 0).sum() >= 2 and (dots < 0).sum() >= 2
        maps = [None, (P, W, A, 7), (np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 30), F32), 0)]
        ref, ties = rr.compute_lo(maps, rp_p, rp_n, rho_r, rho_t, k, max_dist)
        assert not ties.any()
        cases.append((m, maps, ref))
    pv = _bare_context(pvol)
    for m, maps, ref in cases:
        pv.compute_radiance(k, max_dist, maps=maps, radiance=(rp_p, rp_n, rho_r, rho_t))
        gp, gn, lo = pv.radiance_lo()
        assert (gp == rp_p).all() and (gn == rp_n).all()
        _check_lo(lo, ref, "ladder k=%d m=%d" % (k, m))
        if m == 0:
            assert (lo == 0).all()
    pv.close()


# ---------------------------------------------------------------------------------------------- 2. random maps
@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(4242)
    max_dist = 0.15
    centre = np.array([0.5, 0.5, 0.5])
    direct = (rng.random((700, 3)).astype(F32), _unit(rng.normal(size=(700, 3))), rng.random((700, 30)).astype(F32), 1234)
    pin = np.concatenate([rng.random((2000, 3)), centre + _unit(rng.normal(size=(3000, 3))) * (0.02 * rng.random((3000, 1)) ** (1 / 3))]).astype(F32)
    perm = rng.permutation(5000)
    indirect = (pin[perm], _unit(rng.normal(size=(5000, 3))), rng.random((5000, 30)).astype(F32), 977)
    caustic = (np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 30), F32), 0)
    n = 1003
    rp_p = rng.random((n, 3))
    rp_p[:12] = centre + _unit(rng.normal(size=(12, 3))) * 0.02 * rng.random((12, 1))   # inside the clump: 3 000 photons within 0.3 max_dist
    rp_p[12:20] = 1.0 + max_dist + 0.3 * rng.random((8, 3)) + 0.05     # more than max_dist outside every map's box
    rp_p[20:30, 0] = 1.0 + 0.3 * max_dist * rng.random(10)             # just outside
    rp_p[30:40, 2] = -0.3 * max_dist * rng.random(10)
    rp_p = rp_p.astype(F32)
    rp_n = _unit(rng.normal(size=(n, 3)))
    rho_r, rho_t = rng.random((n, 30)).astype(F32), rng.random((n, 30)).astype(F32)
    rho_r[rng.random(n) < 0.15] = 0
    rho_t[rng.random(n) < 0.4] = 0
    rho_r[5] = 0
    rho_t[6] = 0
    rho_r[40:44] = 0
    rho_t[40:44] = 0    # both black
    assert max(np.sqrt(rr.d2_f32(indirect[0], q)[np.argsort(rr.d2_f32(indirect[0], q))[2999]]) for q in rp_p[:12]) < 0.3 * max_dist
    return [caustic, direct, indirect], (rp_p, rp_n, rho_r, rho_t), max_dist


@pytest.mark.parametrize("k", [1, 8, 50, 300])
def test_random_maps_match_the_restatement(pvol, random_case, k):
    maps, rad, max_dist = random_case
    ref, ties = rr.compute_lo(maps, rad[0], rad[1], rad[2], rad[3], k, max_dist)
    assert not ties.any()
    assert (ref[12:20] == 0).all() and (ref[40:44] == 0).all() and (ref.sum(axis=1) > 0).sum() > 800
    pv = _bare_context(pvol)
    pv.compute_radiance(k, max_dist, maps=maps, radiance=rad)
    gp, gn, lo = pv.radiance_lo()
    assert (gp == rad[0]).all() and (gn == rad[1]).all()
    _check_lo(lo, ref, "random maps k=%d" % k)
    assert (lo[12:20] == 0).all() and (lo[40:44] == 0).all()
    pv.close()


# ---------------------------------------------------------------------------------------------- 3. end to end
def _shoot(pvol):
    s = load_scene("volumescene_h")
    h = abi.SceneHolder(s)
    p = abi.params_from_blob(s, n_volume_photons=150, keep_surface_photons=1, n_indirect_photons=40, n_caustic_photons=100, final_gather=1)
    pv = pvol.PhotonVolume(p)
    pv.set_scene(h)
    pv.preprocess(2)
    return pv, h


@pytest.mark.parametrize("max_dist", [0.1, 0.5])
def test_end_to_end_over_the_kept_stores(pvol, max_dist):
    """The stores and radiance photons of a device shoot, downloaded, feed the restatement: shooter rounding does not enter.  At
    maxdist 0.1 every ball of this shoot holds fewer than 50 photons; at 0.5 (the scene file's own maxdist) most direct-map balls
    hold more and some fewer."""
    pv, h = _shoot(pvol)
    maps = []
    for kind in range(3):
        P, W, A, n_paths = pv.surface_photons(kind)
        maps.append((P, W, A, n_paths) if len(P) else None)
    rad = pv.radiance_photons()
    assert len(rad[0]) > 100 and maps[1] is not None
    ref, ties = rr.compute_lo(maps, rad[0], rad[1], rad[2], rad[3], 50, max_dist)
    assert ties.sum() <= 0.01 * ties.size
    keep = ~ties.any(axis=1)
    md2 = F32(max_dist) * F32(max_dist)
    counts = np.array([int((rr.d2_f32(maps[1][0], q) < md2).sum()) for q in rad[0]])
    print("direct-map ball counts at maxdist %g: min %d median %d max %d" % (max_dist, counts.min(), np.median(counts), counts.max()))
    assert (counts < 50).any()
    if max_dist == 0.5:
        assert (counts > 50).any()
    pv.compute_radiance(50, max_dist)
    gp, gn, lo = pv.radiance_lo()
    assert (gp == rad[0]).all() and (gn == rad[1]).all()
    assert (lo.sum(axis=1) > 0).any()
    _check_lo(lo[keep], ref[keep], "end to end maxdist %g" % max_dist)
    pv.close()


# ---------------------------------------------------------------------------------------------- 4. lookup
def _lo_through_the_abi(pv, rp_p, rp_n, rng):
    """Distinct Lo rows for any radiance photons: six photons facing along the axes, seen by every radiance photon (a huge maxdist),
    and a random rho_r per radiance photon."""
    n = len(rp_p)
    P = (rng.random((6, 3)) * 0.01).astype(F32)
    W = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    A = (rng.random((6, 30)) + 0.5).astype(F32)
    rho_r = (rng.random((n, 30)) + 0.05).astype(F32)
    pv.compute_radiance(6, 1000.0, maps=[None, (P, W, A, 3), None], radiance=(rp_p, rp_n, rho_r, np.zeros((n, 30), F32)))
    gp, gn, lo = pv.radiance_lo()
    assert (gp == rp_p).all() and (gn == rp_n).all()
    assert len(np.unique(lo, axis=0)) == n and (lo.sum(axis=1) > 0).all()   # a wrong winner shows
    return lo


def _lookup_both_ways(pv, q_p, q_n):
    import torch
    lo, found = pv.radiance_lookup(q_p, q_n)
    dp, dn = torch.from_numpy(q_p).cuda(), torch.from_numpy(q_n).cuda()
    dlo = torch.full((len(q_p), 30), -1.0, dtype=torch.float32, device="cuda")
    dfound = torch.full((len(q_p),), 7, dtype=torch.int32, device="cuda")
    pv.radiance_lookup_device(dp.data_ptr(), dn.data_ptr(), len(q_p), dlo.data_ptr(), dfound.data_ptr(), 0)
    torch.cuda.synchronize()
    assert dlo.cpu().numpy().tobytes() == lo.tobytes() and dfound.cpu().numpy().astype(np.uint32).tobytes() == found.tobytes()
    return lo, found


def _expected(rp_p, rp_n, q_p, q_n):
    want = np.full(len(q_p), -1)
    for i in range(len(q_p)):
        want[i], tie = rr.nearest_facing(rp_p, rp_n, q_p[i], q_n[i])
        assert not tie
    return want


def _check_lookup(lo, found, want, rows):
    assert ((want >= 0).astype(np.uint32) == found).all()
    ref = np.where((want >= 0)[:, None], rows[np.maximum(want, 0)], F32(0))
    assert ref.astype(F32).tobytes() == lo.tobytes()


def test_lookup_returns_the_nearest_facing_photon(pvol):
    rng = np.random.default_rng(77)
    n = 1003
    rp_p = rng.random((n, 3))
    rp_n = _unit(rng.normal(size=(n, 3)))
    rp_p[:300, 2], rp_n[:300] = 0.25, [0, 0, 1]      # two parallel planes with opposite normals
    rp_p[300:600, 2], rp_n[300:600] = 0.75, [0, 0, -1]
    rp_p, rp_n = rp_p.astype(F32), rp_n.astype(F32)
    m = 4133
    q_p = (rng.random((m, 3)) * 1.4 - 0.2)
    q_p[:40] = (rng.random((40, 3)) - 0.5) * 200.0     # far outside the grid's box
    q_p[40:60] = rp_p[:20] + F32(1e-3)                 # next to a photon
    q_p, q_n = q_p.astype(F32), _unit(rng.normal(size=(m, 3)))
    q_n[60:200] = [0, 0, 1]
    q_n[200:340] = [0, 0, -1]
    want = _expected(rp_p, rp_n, q_p, q_n)
    assert (want >= 0).all()
    pv = _bare_context(pvol)
    rows = _lo_through_the_abi(pv, rp_p, rp_n, rng)
    lo, found = _lookup_both_ways(pv, q_p, q_n)
    _check_lookup(lo, found, want, rows)
    pv.close()


def test_lookup_with_no_facing_photon_and_a_map_of_one(pvol):
    rng = np.random.default_rng(78)
    n = 1500
    rp_p = rng.random((n, 3)).astype(F32)
    rp_n = np.tile(np.array([[0, 0, 1]], F32), (n, 1))
    q_p = (rng.random((300, 3)) * 1.2 - 0.1).astype(F32)
    q_n = np.tile(np.array([[0, 0, -1]], F32), (300, 1))
    q_n[150:] = _unit(rng.normal(size=(150, 3)) + [0, 0, 0.5])
    q_p[297:300] = [[1e30, 0, 0], [0, -3e38, 0], [2e19, 2e19, 2e19]]   # every d2 overflows: nothing is nearer than inf (kdtree.h:181)
    q_n[297:300] = [0, 0, 1]
    want = _expected(rp_p, rp_n, q_p, q_n)
    assert (want[:150] == -1).all() and (want[150:] >= 0).any() and (want[297:300] == -1).all()
    pv = _bare_context(pvol)
    rows = _lo_through_the_abi(pv, rp_p, rp_n, rng)
    lo, found = _lookup_both_ways(pv, q_p, q_n)
    _check_lookup(lo, found, want, rows)
    assert (found[:150] == 0).all() and (lo[:150] == 0).all()   # after a sweep of the whole grid
    # a map of one photon
    one_p, one_n = np.array([[0.3, 0.4, 0.5]], F32), np.array([[0, 1, 0]], F32)
    rows = _lo_through_the_abi(pv, one_p, one_n, rng)
    want = _expected(one_p, one_n, q_p, q_n)
    assert (want == 0).any() and (want == -1).any()
    lo, found = _lookup_both_ways(pv, q_p, q_n)
    _check_lookup(lo, found, want, rows)
    # no radiance photon at all: PVOL_OK, count 0, nothing found
    pv.compute_radiance(50, 0.1, maps=[None, None, None], radiance=(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 30), F32), np.zeros((0, 30), F32)))
    assert pv.radiance_lo_count() == 0
    lo, found = _lookup_both_ways(pv, q_p, q_n)
    assert (found == 0).all() and (lo == 0).all()
    pv.close()


def test_lookup_with_photons_on_cell_boundaries_of_a_long_grid(pvol):
    """A thin slab far from the origin: about 500 cells along x, a photon on every nominal cell boundary lo + i * cell from
    i = 100 on (the cell size restated from DESIGN.md 17: sqrt(2 S / n), S the box's surface area), where the fp32 cell
    assignment may put a photon either side.  Queries sit 0.3 cell either side of each and elsewhere: the shell walk's distance bound
    must not end before the cell that really holds the nearest photon."""
    rng = np.random.default_rng(79)
    n = 20000
    rp_p = np.empty((n, 3))
    rp_p[:, 0] = 16.0 + rng.random(n)
    rp_p[:, 1:] = 0.01 * rng.random((n, 2))
    rp_p[0], rp_p[1] = [16.0, 0.0, 0.0], [17.0, 0.01, 0.01]
    rp_p = rp_p.astype(F32)
    ext = rp_p.max(axis=0).astype(np.float64) - rp_p.min(axis=0)
    ext = np.maximum(ext, 1e-3 * ext.max())
    cell = F32(np.sqrt(2.0 * 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]) / n))
    assert 480 <= int(ext[0] / cell) + 1 <= 520
    idx = np.arange(100, int(ext[0] / cell) + 1)          # every cell boundary from the 100th to the last
    m = len(idx)
    rp_p[2:2 + m, 0] = (F32(16.0) + idx.astype(F32) * cell).astype(F32)
    assert m > 350 and rp_p[:, 0].max() == F32(17.0) and rp_p[:, 0].min() == F32(16.0)
    rp_n = _unit(rng.normal(size=(n, 3)))
    on = slice(2, 2 + m)
    q_p = np.concatenate([rp_p[on] + [0.3 * cell, 0, 0], rp_p[on] - [0.3 * cell, 0, 0], rp_p[on],
                          np.column_stack([15.9 + 1.2 * rng.random(600), 0.03 * rng.random((600, 2)) - 0.01])]).astype(F32)
    q_n = np.concatenate([rp_n[on], rp_n[on], -rp_n[on], _unit(rng.normal(size=(600, 3)))]).astype(F32)
    want = _expected(rp_p, rp_n, q_p, q_n)
    assert (want >= 0).all() and (want[:2 * m] != np.tile(np.arange(2, 2 + m), 2)).any() and (want[:2 * m] == np.tile(np.arange(2, 2 + m), 2)).any()
    pv = _bare_context(pvol)
    rows = _lo_through_the_abi(pv, rp_p, rp_n, rng)
    lo, found = _lookup_both_ways(pv, q_p, q_n)
    _check_lookup(lo, found, want, rows)
    pv.close()


# ---------------------------------------------------------------------------------------------- 5. life cycle
def test_life_cycle(pvol):
    pv, h = _shoot(pvol)
    q_p, q_n = np.zeros((3, 3), F32), np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], F32)
    assert pv.radiance_lo_count() == 0
    with pytest.raises(pvol.PvolError) as e:
        pv.radiance_lookup(q_p, q_n)     # before any compute
    assert e.value.status == abi.PVOL_E_INVALID
    pv.compute_radiance(50, 0.5)
    n = pv.radiance_lo_count()
    assert n == len(pv.radiance_photons()[0]) > 0
    first = pv.radiance_lo()
    look = pv.radiance_lookup(q_p, q_n)
    pv.compute_radiance(50, 0.5)
    second = pv.radiance_lo()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))   # no atomics: bit for bit
    for args, status in [((0, 0.5), abi.PVOL_E_INVALID), ((577, 0.5), abi.PVOL_E_UNSUPPORTED), ((50, float("nan")), abi.PVOL_E_INVALID),
                         ((50, 0.0), abi.PVOL_E_INVALID)]:
        with pytest.raises(pvol.PvolError) as e:
            pv.compute_radiance(*args)
        assert e.value.status == status
    bad = (np.full((2, 3), np.inf, F32), np.zeros((2, 3), F32), np.ones((2, 30), F32), np.ones((2, 30), F32))
    with pytest.raises(pvol.PvolError) as e:
        pv.compute_radiance(50, 0.5, maps=[None, None, None], radiance=bad)
    assert e.value.status == abi.PVOL_E_INVALID
    third = pv.radiance_lo()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, third))    # refusals leave the result in place
    again = pv.radiance_lookup(q_p, q_n)
    assert again[0].tobytes() == look[0].tobytes() and again[1].tobytes() == look[1].tobytes()
    pv.compute_radiance(8, 0.1)                                             # a second compute replaces the first
    assert pv.radiance_lo_count() == n and pv.radiance_lo()[2].tobytes() != first[2].tobytes()
    pv.preprocess(2)                                                        # a new shoot drops it
    assert pv.radiance_lo_count() == 0
    with pytest.raises(pvol.PvolError) as e:
        pv.radiance_lookup(q_p, q_n)
    assert e.value.status == abi.PVOL_E_INVALID
    pv.close()
    # without kept stores there is nothing to compute from
    s = load_scene("volumescene_h")
    p = abi.params_from_blob(s, n_volume_photons=150, n_indirect_photons=40, n_caustic_photons=100)
    pv = pvol.PhotonVolume(p)
    pv.set_scene(abi.SceneHolder(s))
    with pytest.raises(pvol.PvolError) as e:
        pv.compute_radiance(50, 0.1)
    assert e.value.status == abi.PVOL_E_INVALID
    pv.close()
