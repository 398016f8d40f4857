"""Radiance photons without a GPU: the yardstick of test_gpu_radiance_photons.py -- sort by d2, take n_lookup --
equals a literal transcription of PhotonProcess (core/photonshooter.h:186-203) whatever order the photons are visited in, and
every status of pvol_compute_radiance / pvol_compute_radiance_arrays / pvol_radiance_lookup* is decided by pure host code
(pvol_check_radiance, exported next to pvol_plan_batch)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT, abi

import radiance_ref as rr

OK, INVALID, UNSUPPORTED = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_UNSUPPORTED


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def test_sorting_equals_photon_process_in_any_visiting_order():
    """A kd-tree hands PhotonProcess the photons in an order that depends on the tree; whatever the order, the heap ends with the
    n_lookup nearest and md2 is the n_lookup-th smallest d2 (or max_dist^2 with fewer photons in the ball)."""
    rng = np.random.default_rng(20260417)
    lookups = regimes = 0
    seen = set()
    for case in range(60):
        n = int(rng.integers(1, 400))
        P = rng.random((n, 3)).astype(np.float32)
        max_dist = float(rng.choice([0.1, 0.25, 0.6]))
        for q in rng.random((5, 3)).astype(np.float32):
            d2 = rr.d2_f32(P, q)
            assert len(np.unique(d2)) == len(d2)   # no tie anywhere, so one valid answer
            for k in (1, 7, 50):
                idx, md2, tie = rr.knn(d2, k, max_dist)
                assert not tie
                inside = int((d2 < np.float32(max_dist) * np.float32(max_dist)).sum())
                seen.add("fewer" if inside < k else "exactly" if inside == k else "more")
                for _ in range(3):
                    got, gmd2 = rr.photon_process(d2, rng.permutation(n), k, max_dist)
                    assert got == set(int(i) for i in idx)
                    assert gmd2 == md2 and gmd2.dtype == np.float32
                lookups += 1
    assert lookups >= 300 and {"fewer", "more"} <= seen


def test_md2_in_the_three_regimes():
    P = np.zeros((6, 3), np.float32)
    P[:, 0] = [0.01, 0.02, 0.03, 0.04, 0.05, 0.2]
    d2 = rr.d2_f32(P, np.zeros(3, np.float32))
    m2 = np.float32(0.1) * np.float32(0.1)
    for k, want_n, want_md2 in [(7, 5, m2), (5, 5, d2[4]), (3, 3, d2[2])]:
        idx, md2, tie = rr.knn(d2, k, 0.1)
        assert len(idx) == want_n and md2 == want_md2 and not tie
        assert rr.photon_process(d2, range(6), k, 0.1) == (set(int(i) for i in idx), md2)
    # a photon at exactly max_dist^2 is not visited (kdtree.h:180 is a strict <)
    P[5, 0] = 0.1
    d2 = rr.d2_f32(P, np.zeros(3, np.float32))
    assert d2[5] == m2 and 5 not in rr.knn(d2, 7, 0.1)[0]


def _arrays(n, rng, n_paths=10):
    p, w, a = rng.random((n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32), rng.random((n, 30)).astype(np.float32)
    return p, w, a, n_paths


def _check(pvol, what=1, have_ctx=1, have_state=0, n_lookup=50, max_dist=0.1, maps=(None, None, None), rp=None, count=None, out=(1, 1), host=1):
    f32p = C.POINTER(C.c_float)
    ptrs, keep = pvol.photon_arrays(list(maps))
    arrs = [None] * 4
    n = 0
    if rp is not None:
        arrs = [None if x is None else np.ascontiguousarray(x, np.float32) for x in rp]
        n = max(x.size // w for x, w in zip(arrs, (3, 3, 30, 30)) if x is not None)
    if count is not None:
        n = count
    a = [None if x is None else x.ctypes.data_as(f32p) for x in arrs]
    return pvol.lib().pvol_check_radiance(what, have_ctx, have_state, n_lookup, max_dist, ptrs, a[0], a[1], a[2], a[3], n, out[0] or None, out[1] or None, host)


def test_every_status_without_a_device(pvol):
    rng = np.random.default_rng(3)
    good_map = _arrays(20, rng)
    rp = [rng.random((5, 3)), rng.random((5, 3)), rng.random((5, 30)), rng.random((5, 30))]
    assert _check(pvol, maps=(good_map, None, good_map), rp=rp) == OK
    assert _check(pvol, rp=rp) == OK                      # three NULL maps: EPhoton's `if (!map) return 0`
    assert _check(pvol, maps=(good_map, None, None)) == OK   # zero radiance photons
    assert _check(pvol, have_ctx=0, rp=rp) == INVALID        # NULL ctx
    for i in range(4):                                       # a NULL array with a count > 0
        bad = list(rp)
        bad[i] = None
        assert _check(pvol, rp=bad, count=5) == INVALID
    for i in range(3):                                       # ... inside a map too
        ptrs, _ = pvol.photon_arrays([None, None, None])
        full = [x.ctypes.data_as(C.POINTER(C.c_float)) for x in good_map[:3]]
        pa = abi.PhotonArray(*[None if j == i else full[j] for j in range(3)], 20, 10)
        ptrs[1] = C.pointer(pa)
        assert pvol.lib().pvol_check_radiance(1, 1, 0, 50, 0.1, ptrs, None, None, None, None, 0, None, None, 1) == INVALID
    assert _check(pvol, n_lookup=0, rp=rp) == INVALID
    assert _check(pvol, n_lookup=-3, rp=rp) == INVALID
    for md in (0.0, -0.1, float("nan"), float("inf")):
        assert _check(pvol, max_dist=md, rp=rp) == INVALID
        assert _check(pvol, what=0, have_state=1, max_dist=md) == INVALID
    assert _check(pvol, maps=(None, good_map[:3] + (0,), None), rp=rp) == INVALID   # n > 0 with n_paths == 0
    assert _check(pvol, maps=(None, (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 30)), 0), None), rp=rp) == OK   # n == 0: no map
    for which in range(3):                                   # a non-finite value in a map ...
        for v in (np.nan, np.inf):
            m = [np.array(x, np.float32) for x in good_map[:3]]
            m[which][7, 1] = v
            assert _check(pvol, maps=(None, None, tuple(m) + (10,)), rp=rp) == INVALID
    for which in range(4):                                   # ... or in the radiance photons
        bad = [np.array(x, np.float32) for x in rp]
        bad[which][3, 2] = -np.inf
        assert _check(pvol, rp=bad) == INVALID
    assert _check(pvol, n_lookup=576, rp=rp) == OK
    assert _check(pvol, n_lookup=577, rp=rp) == UNSUPPORTED
    assert _check(pvol, what=0, have_state=1, n_lookup=577) == UNSUPPORTED
    assert _check(pvol, n_lookup=577, max_dist=0.0, rp=rp) == INVALID   # an invalid argument wins over the bound
    # pvol_compute_radiance: needs the stores of a pvol_preprocess that ran with keep_surface_photons
    assert _check(pvol, what=0, have_state=0) == INVALID
    assert _check(pvol, what=0, have_state=1) == OK
    assert _check(pvol, what=0, have_ctx=0, have_state=1) == INVALID
    # lookups: only after a compute; NULL arrays with a count; non-finite queries through the host entry
    q = [rng.random((4, 3)), rng.random((4, 3)), None, None]
    assert _check(pvol, what=2, have_state=0, rp=q) == INVALID
    assert _check(pvol, what=2, have_state=1, rp=q) == OK
    assert _check(pvol, what=2, have_ctx=0, have_state=1, rp=q) == INVALID
    assert _check(pvol, what=2, have_state=1, count=0) == OK
    assert _check(pvol, what=2, have_state=1, rp=[q[0], None, None, None], count=4) == INVALID
    assert _check(pvol, what=2, have_state=1, rp=q, out=(0, 1)) == INVALID
    assert _check(pvol, what=2, have_state=1, rp=q, out=(1, 0)) == INVALID
    bad = [np.array(q[0], np.float32), np.array(q[1], np.float32), None, None]
    bad[1][2, 0] = np.nan
    assert _check(pvol, what=2, have_state=1, rp=bad) == INVALID
    assert _check(pvol, what=2, have_state=1, rp=bad, host=0) == OK   # device pointers cannot be read here


def test_entry_points_reject_a_null_context(pvol):
    L = pvol.lib()
    n = C.c_uint32()
    assert L.pvol_compute_radiance(None, 50, 0.1) == INVALID
    assert L.pvol_compute_radiance_arrays(None, 50, 0.1, None, None, None, None, None, 0) == INVALID
    assert L.pvol_radiance_lo_count(None, C.byref(n)) == INVALID
    assert L.pvol_download_radiance_lo(None, None, None, None, 0) == INVALID
    assert L.pvol_radiance_lookup(None, None, None, 0, None, None) == INVALID
    assert L.pvol_radiance_lookup_device(None, None, None, 0, None, None, None) == INVALID
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    assert "pvol_check_radiance" not in text and "pvol_compute_radiance_arrays" in text   # a test entry like pvol_check_scene, not ABI
    assert C.sizeof(abi.PhotonArray) == 32
