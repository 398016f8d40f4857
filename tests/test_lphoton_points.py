"""pvol_lphoton_batch without a GPU: the numpy yardstick (lphoton_ref.py) against the oracle's LPhoton at explicit
points, what the GPU tests rest on (no boundary ties, enough full lookups, sparse and outside points in every case), every status of
pvol_check_lphoton in its order, the slice planner, the entry points without a context and the exported symbols."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

from conftest import abi

import lphoton_cases as cases
import lphoton_ref as ref

OK, INVALID, NO_SCENE = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_NO_SCENE
F = np.float32


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


ALL = [(s, t, k, d) for s, t in cases.SCENES + [cases.GRID_SCENE] for k, d in cases.PAIRS]


@pytest.mark.parametrize("scene_name,tag,nused,maxdist", ALL, ids=["%s-k%d" % (t, k) for s, t, k, d in ALL])
def test_yardstick_equals_the_oracle(orc, scene_name, tag, nused, maxdist):
    """1e-5 per query: the float64 sum against the oracle's float32 one measured 1.0e-6 at worst (HG, k = 50), a margin of ten for
    other seeds.  The VolumeGrid case takes sigma_s(p) from the yardstick's own trilinear density."""
    scene, photons, q, w, want = cases.case(scene_name, tag, nused, maxdist)
    o = orc.Oracle(abi.SceneHolder(scene), cases.params(scene, nused, maxdist))
    try:
        o.set_photons(*photons)
        got = o.lphoton_batch(q, w)
    finally:
        o.close()
    err = ref.rel_l2(want["L"], got)
    full = int((want["n_found"] == nused).sum())
    outside = ~ref.Medium(scene).inside(q)
    print("%s k=%d maxdist=%g: largest error %.3g, median %.3g, %d full, %d below 10, %d outside, %d ties"
          % (tag, nused, maxdist, err.max(), np.median(err), full, int((want["n_found"] < 10).sum()), int(outside.sum()), int(want["tie"].sum())))
    assert err.max() <= 1e-5
    assert ((got != 0).any(axis=1) == (want["L"] != 0).any(axis=1)).all()
    # what the GPU tests rest on
    assert not want["tie"].any()
    assert full >= len(q) // 4
    assert (want["n_found"] < 10).any() and (want["n_found"] == 0).any()
    assert outside.any() and (want["L"][outside] == 0).all()
    assert (want["L"] != 0).any()


def test_yardstick_selection_on_a_hand_made_map():
    """Ties in photon order, the strict d2 < maxdist^2, radius2 of a sparse lookup."""
    pp = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 0, -1], [0, 3, 0]], F)
    kept, n_found, r2, tie = ref.select(pp, np.zeros((1, 3), F), 3, 2.0)
    assert kept[0].tolist() == [0, 1, 2] and n_found[0] == 3 and r2[0] == 1 and tie[0]          # four at distance 1: a boundary tie
    kept, n_found, r2, tie = ref.select(pp, np.zeros((1, 3), F), 4, 2.0)
    assert kept[0].tolist() == [0, 1, 2, 4] and r2[0] == 1 and not tie[0]                       # (2, 0, 0) is AT maxdist: not inside
    kept, n_found, r2, tie = ref.select(pp, np.zeros((1, 3), F), 5, 2.0)
    assert n_found[0] == 4 and r2[0] == 1 and not tie[0]
    kept, n_found, r2, tie = ref.select(pp, np.full((1, 3), 50, F), 5, 2.0)
    assert n_found[0] == 0 and r2[0] == 0 and len(kept[0]) == 0


def _check(pvol, have_ctx=1, have_scene=1, g=0.0, null=(), n=4, kind=abi.OUT_SPECTRAL, args=True):
    buf = np.zeros(64, F)
    a = abi.LPhotonCheck()
    for name in ("p", "w", "out"):
        setattr(a, name, None if name in null else buf.ctypes.data)
    a.n, a.output_kind = n, kind
    return pvol.lib().pvol_check_lphoton(have_ctx, C.byref(a) if args else None, have_scene, g)


def test_every_status_in_its_order(pvol):
    assert _check(pvol) == OK
    assert _check(pvol, kind=abi.OUT_XYZ) == OK
    assert _check(pvol, null=("w",)) == OK                      # g == 0 reads no direction
    assert _check(pvol, g=0.6) == OK
    assert _check(pvol, n=0, null=("p", "w", "out"), g=0.6) == OK   # n == 0 does nothing
    # 1. no context
    assert _check(pvol, have_ctx=0) == INVALID
    assert _check(pvol, args=False) == INVALID
    # 2. the arguments
    assert _check(pvol, null=("p",)) == INVALID
    assert _check(pvol, null=("out",)) == INVALID
    assert _check(pvol, null=("w",), g=0.6) == INVALID
    assert _check(pvol, null=("w",), g=-0.2) == INVALID
    assert _check(pvol, kind=2) == INVALID
    assert _check(pvol, kind=-1) == INVALID
    assert _check(pvol, kind=7, n=0) == INVALID
    # 3. no scene
    assert _check(pvol, have_scene=0) == NO_SCENE
    # two faults at once: the earlier one in the order is reported
    assert _check(pvol, have_ctx=0, have_scene=0, null=("p",)) == INVALID
    assert _check(pvol, have_scene=0, null=("p",)) == INVALID
    assert _check(pvol, have_scene=0, kind=5) == INVALID
    assert _check(pvol, have_scene=0, null=("w",)) == NO_SCENE   # without a scene there is no g to ask for a direction
    assert _check(pvol, have_scene=0, n=0) == NO_SCENE


def test_slice_planner(pvol):
    f = pvol.lib().pvol_lphoton_slice
    per, top = abi.LPHOTON_POINT_SCRATCH, abi.LPHOTON_SCRATCH_BYTES
    assert f(0) == top // per == 1 << 22
    assert f(top) == f(top + 1) == f(1 << 40) == top // per     # the hook only lowers the bound
    assert f(per * 64) == 64 and f(per * 64 + per - 1) == 64
    assert f(per * 127) == 64 and f(per * 128) == 128            # whole runs of 64 where that many fit
    assert f(per * 50) == 50 and f(per * 63) == 63               # below one run: what fits
    assert f(per) == 1 and f(1) == 1 and f(per - 1) == 1         # never fewer than one
    for bound in (per * 1000, per * 4097, 12345678):
        n = f(bound)
        assert n * per <= bound and n % 64 == 0 and (n + 64) * per > bound


def test_entry_points_without_a_context(pvol):
    L = pvol.lib()
    buf = np.full(64, 7, F)
    p = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pvol_lphoton_batch(None, p, p, 2, abi.OUT_SPECTRAL, p, None, None) == INVALID
    assert L.pvol_lphoton_batch_device(None, buf.ctypes.data, buf.ctypes.data, 2, abi.OUT_XYZ, buf.ctypes.data, None, None, None) == INVALID
    assert L.pvol_lphoton_batch(None, None, None, 0, abi.OUT_SPECTRAL, None, None, None) == INVALID
    assert L.pvol_lphoton_set_scratch_bound(None, 1024) == INVALID
    assert (buf == 7).all()


def test_symbols_are_exported(pvol):
    assert "pvol_lphoton_batch" in pvol.EXPORTS and "pvol_lphoton_batch_device" in pvol.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", pvol.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("pvol_lphoton_batch", "pvol_lphoton_batch_device", "pvol_check_lphoton", "pvol_lphoton_slice", "pvol_lphoton_set_scratch_bound"):
        assert sym in names, sym
    assert pvol.lib().pvol_abi_version() == 3
