"""The final gather's sampling half without a GPU: the yardstick's heap routines and tree are pinned to the C++
library that builds the oracle (tests/heap_probe.cpp), the host tree builder (pvol_gather_tree_build) equals the yardstick's tree
field for field, and every status of the gather entry points is decided by pure host code (pvol_check_gather)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, abi

import gather_ref as gr

OK, INVALID, UNSUPPORTED, NO_DEVICE = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_UNSUPPORTED, abi.PVOL_E_NO_DEVICE
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def planar_set(rng, n=600):
    """x = 5 exactly; y and z on multiples of 1/32, so that coordinates, positions and distances repeat."""
    P = (rng.integers(0, 32, (n, 3)) / 32.0).astype(np.float32)
    P[:, 0] = 5.0
    return P


def doubled_set(rng, n=500):
    P = rng.random((n, 3)).astype(np.float32)
    return np.concatenate([P, P])


def lattice_set(m=8):
    g = np.arange(m, dtype=np.float32) / np.float32(8.0)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def test_heap_and_tree_transcriptions_equal_the_real_library(tmp_path):
    """About 200 sequences of (d2, id) through std::make_heap / pop_heap / push_heap, k in {1, 2, 3, 50}, with and without repeated
    d2: the final arrays equal the Python transcription's element for element.  And trees from std::nth_element under CompareNode's
    order on point sets with duplicated coordinates: the node order equals the yardstick's."""
    exe = tmp_path / "heap_probe"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "heap_probe.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(20261019)
    lines, want = [], []
    for case in range(208):
        k = (1, 2, 3, 50)[case % 4]
        m = int(rng.integers(0, 4 * k + 40))
        d2 = rng.random(m).astype(np.float32)
        if case % 3 == 0 and m:   # repeated d2: a few distinct values only
            d2 = rng.choice(d2[:max(1, m // 6)], m).astype(np.float32)
        ids = rng.permutation(4 * m + 1)[:m]
        lines.append("H %d %d" % (k, m))
        lines += ["%d %d" % (b, i) for b, i in zip(_bits(d2), ids)]
        h, _ = gr.photon_process([(float(v), int(i)) for v, i in zip(d2, ids)], k, float("inf"))
        want.append([len(h)] + [x for v, i in h for x in (int(np.float32(v).view(np.uint32)), i)])
    sets = [rng.random((n, 3)).astype(np.float32) for n in (1, 2, 3, 7, 50, 51, 333)]
    sets += [planar_set(rng), doubled_set(rng), lattice_set(6), np.round(rng.random((700, 3)) * 4).astype(np.float32) / 4]
    for P in sets:
        lines.append("T %d" % len(P))
        lines += ["%d %d %d" % tuple(r) for r in _bits(P)]
        nd, _ = gr.build_tree(P)
        want.append([len(P)] + [int(x) for r in nd for x in (r["index"], r["split_axis"], r["has_left_child"], r["right_child"])])
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(want)
    for got, w in zip(out, want):
        assert [int(x) for x in got.split()] == w
    heaps = want[:208]
    assert sum(1 for w in heaps if w[0] == 50) > 30 and sum(1 for w in heaps if w[0] < 50 and w[0] > 3) > 5   # full heaps and short arrays


TREE_SETS = ["r1", "r2", "r3", "r50", "r51", "r1000", "r20000", "planar", "doubled", "lattice"]


def tree_set(name):
    rng = np.random.default_rng(77)
    if name[0] == "r":
        return rng.random((int(name[1:]), 3)).astype(np.float32)
    return {"planar": lambda: planar_set(rng), "doubled": lambda: doubled_set(rng), "lattice": lattice_set}[name]()


@pytest.mark.parametrize("name", TREE_SETS)
def test_host_tree_equals_the_yardstick(pvol, name):
    P = tree_set(name)
    want, want_depth = gr.build_tree(P)
    got, depth = pvol.gather_tree(P)
    assert got.dtype == pvol.GATHER_NODE_DTYPE == gr.NODE_DTYPE
    for f in gr.NODE_DTYPE.names:
        np.testing.assert_array_equal(got[f].view(np.uint32) if got[f].dtype == np.float32 else got[f],
                                      want[f].view(np.uint32) if want[f].dtype == np.float32 else want[f], err_msg=f)
    n = len(P)
    assert depth == want_depth and 1 <= depth <= int(np.floor(np.log2(n))) + 1 <= 25
    np.testing.assert_array_equal(np.sort(got["index"]), np.arange(n))
    np.testing.assert_array_equal(got["p"], P[got["index"]])


def test_tree_builder_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/pvol_gather_tree.h is plain C++: a stand-alone program of its own (tests/gather_tree_main.cpp) builds a 100 000-point
    tree under -fsanitize=address,undefined and checks the invariants a lookup relies on."""
    exe = tmp_path / "gather_tree_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "gather_tree_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "100000"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok 100000 points"), r.stdout + r.stderr


def test_tree_hook_statuses(pvol):
    L = pvol.lib()
    d = C.c_int32()
    P = np.random.default_rng(1).random((4, 3)).astype(np.float32)
    buf = np.zeros(4, pvol.GATHER_NODE_DTYPE)
    assert L.pvol_gather_tree_build(P.ctypes.data_as(f32p), 4, buf.ctypes.data, C.byref(d)) == OK
    assert L.pvol_gather_tree_build(None, 4, buf.ctypes.data, C.byref(d)) == INVALID
    assert L.pvol_gather_tree_build(P.ctypes.data_as(f32p), 4, None, C.byref(d)) == INVALID
    assert L.pvol_gather_tree_build(P.ctypes.data_as(f32p), 4, buf.ctypes.data, None) == INVALID
    assert L.pvol_gather_tree_build(P.ctypes.data_as(f32p), 0, buf.ctypes.data, C.byref(d)) == UNSUPPORTED
    bad = P.copy()
    bad[2, 1] = np.nan
    assert L.pvol_gather_tree_build(bad.ctypes.data_as(f32p), 4, buf.ctypes.data, C.byref(d)) == INVALID


def _check(pvol, what, have_ctx=1, have_state=1, store_n=1000, indirect=None, host=1, **kw):
    """pvol_check_gather with every pointer of the call non-NULL unless kw says otherwise (a pointer given as None is NULL)."""
    keep = []
    a = pvol.GatherCheck()
    dummy = np.zeros(64, np.float32)
    ptr = dummy.ctypes.data_as(f32p)
    if indirect is not None:
        p, w = (np.ascontiguousarray(x, np.float32) for x in indirect[:2])
        n = indirect[2] if len(indirect) > 2 else len(p)
        pa = abi.PhotonArray(p.ctypes.data_as(f32p) if p.size else None, w.ctypes.data_as(f32p) if w.size else None, None, n, 0)
        keep += [p, w, pa]
        a.indirect = C.pointer(pa)
    a.count, a.max_dist, a.n_samples, a.cos_gather_angle = kw.get("count", 4), kw.get("max_dist", 0.1), kw.get("n_samples", 16), kw.get("cos", 0.98)
    for name in ("p", "frames", "wo", "u_bsdf", "u_photon"):
        setattr(a, name, ptr if kw.get(name, 1) is not None else None)
    for name in ("out_index", "out_d2", "out_found", "out_rounds", "out_bsdf", "out_photon"):
        setattr(a, name, dummy.ctypes.data if kw.get(name, 1) is not None else None)
    return pvol.lib().pvol_check_gather(what, have_ctx, have_state, store_n, C.byref(a), host)


def test_every_status_without_a_device(pvol):
    rng = np.random.default_rng(5)
    P, W = rng.random((60, 3)).astype(np.float32), rng.random((60, 3)).astype(np.float32)
    # builds from the kept store
    assert _check(pvol, 0) == OK
    assert _check(pvol, 0, have_ctx=0) == INVALID
    assert _check(pvol, 0, have_state=0) == INVALID                  # no kept stores
    assert _check(pvol, 0, store_n=49) == UNSUPPORTED                # photonmap.cpp:194 would not terminate
    assert _check(pvol, 0, store_n=50) == OK
    assert _check(pvol, 0, store_n=0) == UNSUPPORTED
    assert _check(pvol, 0, store_n=(1 << 24)) == OK
    assert _check(pvol, 0, store_n=(1 << 24) + 1) == UNSUPPORTED
    assert _check(pvol, 0, have_state=0, store_n=10) == INVALID      # two faults: the invalid argument wins over the bound
    assert pvol.lib().pvol_check_gather(0, 1, 1, 1000, None, 0) == OK   # a build from the store has no arguments
    assert pvol.lib().pvol_check_gather(1, 1, 0, 0, None, 1) == INVALID
    assert _check(pvol, 4) == INVALID and _check(pvol, -1) == INVALID
    # builds from arrays (have_state plays no part)
    assert _check(pvol, 1, have_state=0, indirect=(P, W)) == OK
    assert _check(pvol, 1, have_ctx=0, indirect=(P, W)) == INVALID
    assert _check(pvol, 1, have_state=0) == INVALID                  # NULL indirect
    assert _check(pvol, 1, indirect=(P, np.zeros((0, 3)), 60)) == INVALID   # NULL wi with n > 0
    assert _check(pvol, 1, indirect=(np.zeros((0, 3)), W, 60)) == INVALID   # NULL p
    assert _check(pvol, 1, indirect=(P[:49], W[:49])) == UNSUPPORTED
    assert _check(pvol, 1, indirect=(P[:50], W[:50])) == OK
    assert _check(pvol, 1, indirect=(np.zeros((0, 3)), np.zeros((0, 3)), 0)) == UNSUPPORTED   # an empty map
    for which in range(2):
        for v in (np.nan, np.inf, -np.inf):
            bad = [P.copy(), W.copy()]
            bad[which][17, 2] = v
            assert _check(pvol, 1, indirect=tuple(bad)) == INVALID
            assert _check(pvol, 1, indirect=(bad[0][:40], bad[1][:40])) == INVALID   # two faults: non-finite and too few
            assert _check(pvol, 1, indirect=tuple(bad), host=0) == OK               # device pointers cannot be read here
    # lookups
    for what in (2, 3):
        assert _check(pvol, what) == OK
        assert _check(pvol, what, have_ctx=0) == INVALID
        assert _check(pvol, what, have_state=0) == INVALID           # before any build
        for md in (0.0, -0.1, float("nan"), float("inf"), 1e-30):    # 1e-30 ** 2 is 0 in fp32: the doubling would never leave it
            assert _check(pvol, what, max_dist=md) == INVALID
        assert _check(pvol, what, max_dist=1e-20) == OK
        assert _check(pvol, what, p=None) == INVALID
        assert _check(pvol, what, p=None, count=0) == OK
        assert _check(pvol, what, have_state=0, max_dist=0.0) == INVALID
    for name in ("out_index", "out_d2", "out_found", "out_rounds"):
        assert _check(pvol, 2, **{name: None}) == INVALID
        assert _check(pvol, 3, **{name: None}) == OK                 # not an argument of the directions call
    for name in ("frames", "wo", "u_bsdf", "u_photon", "out_bsdf", "out_photon"):
        assert _check(pvol, 3, **{name: None}) == INVALID
        assert _check(pvol, 3, count=0, **{name: None}) == OK
        assert _check(pvol, 2, **{name: None}) == OK
    for ns in (0, -1, 257):
        assert _check(pvol, 3, n_samples=ns) == INVALID
        assert _check(pvol, 2, n_samples=ns) == OK
    assert _check(pvol, 3, n_samples=1) == OK and _check(pvol, 3, n_samples=256) == OK
    for c in (1.0, -1.0, 1.5, float("nan")):
        assert _check(pvol, 3, cos=c) == INVALID
    assert _check(pvol, 3, cos=-0.5) == OK and _check(pvol, 3, cos=0.0) == OK


def test_entry_points_without_a_context_or_device(pvol):
    L = pvol.lib()
    n = C.c_uint32()
    assert L.pvol_build_gather_map(None) == INVALID
    assert L.pvol_build_gather_map_arrays(None, None) == INVALID
    assert L.pvol_gather_map_count(None, C.byref(n)) == INVALID
    assert L.pvol_gather_photons(None, None, 0, 0.1, None, None, None, None) == INVALID
    assert L.pvol_gather_photons_device(None, None, 0, 0.1, None, None, None, None, None) == INVALID
    assert L.pvol_gather_directions(None, None, None, None, 0, 0.1, 16, 0.9, None, None, None, None) == INVALID
    assert L.pvol_gather_directions_device(None, None, None, None, 0, 0.1, 16, 0.9, None, None, None, None, None) == INVALID
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    for name in ("pvol_check_gather(", "pvol_gather_tree_build("):   # test entries like pvol_check_scene, not ABI
        assert name not in text
    assert C.sizeof(pvol.GatherCheck) == 112
    if L.pvol_device_count() == 0:   # no context can exist without a device: creation itself answers PVOL_E_NO_DEVICE
        p = abi.Params()
        L.pvol_default_params(C.byref(p))
        h = C.c_void_p()
        assert L.pvol_create(C.byref(p), C.byref(h)) == NO_DEVICE


def test_cos_gather_angle_helper(pvol):
    for ga in (10.0, 60.0, 0.5, 89.0):
        assert pvol.gather_cos_angle(ga) == gr.cos_gather_angle(ga)
        assert abs(pvol.gather_cos_angle(ga) - np.cos(np.radians(ga))) < 1e-6
    assert pvol.gather_cos_angle(10.0) == float(np.float32(np.cos(np.float64(np.float32(np.float32(np.pi) / np.float32(180)) * np.float32(10)))))


def test_yardstick_lookup_is_the_k_nearest_set():
    """The yardstick's own sanity: whatever the heap order, the 50 it returns are the 50 nearest (tie-free input) and rounds follow
    the doubling."""
    rng = np.random.default_rng(9)
    P = rng.random((400, 3)).astype(np.float32)
    T = gr.Tree(P)
    for q in rng.random((20, 3)).astype(np.float32):
        dv = P - q
        d2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
        idx, dd, found, rounds = T.lookup(q, 0.05)
        assert found == 50 and len(np.unique(d2)) == len(d2)
        assert set(idx.tolist()) == set(np.argsort(d2)[:50].tolist())
        np.testing.assert_array_equal(dd, d2[idx])
        assert dd[0] == dd.max()
        r = 1
        while (d2 < np.float32(0.05) * np.float32(0.05) * np.float32(2.0) ** (r - 1)).sum() < 50:
            r += 1
        assert rounds == r
