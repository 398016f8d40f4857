"""pvol_radiance_gather_batch without a GPU: every status of pvol_radiance_gather_check in its order, the slice planner
(n_samples shrinks a slice; pvol_radiance_slice's answers are what they were), the layouts of pvol_gather_params and
pvol_radiance_gather_out from a compiled C program, the entry points without a context and without a device, and the exports."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, abi, load_scene

OK, INVALID, NO_SCENE, UNSUPPORTED = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_NO_SCENE, abi.PVOL_E_UNSUPPORTED
NONE, HOMOGENEOUS, GRID, RAINBOW, EXPONENTIAL = 0, 1, 2, 3, 4   # pvol_volume_kind
F = np.float32


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _check(pvol, have_ctx=1, have_scene=1, vol=HOMOGENEOUS, surf=1, indirect=0, gather=1, rad=1, rad_n=100, null=(), n_rays=4, n_streams=2,
           kind=abi.OUT_SPECTRAL, args=True, max_dist=0.5, n_samples=4, cos=0.98):
    buf = np.zeros(64, F)
    out = abi.RadianceGatherOut()
    out.L = None if "L" in null else buf.ctypes.data
    g = abi.GatherParams(max_dist, n_samples, cos, None if "u_bsdf" in null else buf.ctypes.data, None if "u_photon" in null else buf.ctypes.data)
    a = abi.RadianceGatherCheck()
    a.rays = None if "rays" in null else buf.ctypes.data
    a.streams = None if "streams" in null else buf.ctypes.data
    a.n_rays, a.n_streams, a.output_kind = n_rays, n_streams, kind
    a.out = None if "out" in null else C.pointer(out)
    a.gather = None if "gather" in null else C.pointer(g)
    return pvol.lib().pvol_radiance_gather_check(have_ctx, C.byref(a) if args else None, have_scene, vol, surf, indirect, gather, rad, rad_n)


def test_every_status_in_its_order(pvol):
    for vol in (NONE, HOMOGENEOUS, RAINBOW):
        assert _check(pvol, vol=vol) == OK
    assert _check(pvol, kind=abi.OUT_XYZ) == OK
    assert _check(pvol, n_samples=1) == OK and _check(pvol, n_samples=256) == OK
    assert _check(pvol, n_rays=0, n_streams=0, null=("rays", "streams", "out", "u_bsdf", "u_photon")) == OK   # nothing to do
    assert _check(pvol, n_rays=0, null=("L", "u_bsdf")) == OK
    # 1. items 1 to 4 of pvol_radiance_batch_check
    assert _check(pvol, have_ctx=0) == INVALID
    assert _check(pvol, args=False) == INVALID
    assert _check(pvol, kind=2) == INVALID and _check(pvol, kind=-1) == INVALID
    assert _check(pvol, kind=9, n_rays=0, n_streams=0) == INVALID
    assert _check(pvol, null=("rays",)) == INVALID
    assert _check(pvol, null=("streams",)) == INVALID
    assert _check(pvol, null=("streams",), n_rays=0) == INVALID
    assert _check(pvol, null=("out",)) == INVALID
    assert _check(pvol, null=("L",)) == INVALID
    # 2. the gather's arguments
    assert _check(pvol, null=("gather",)) == INVALID
    assert _check(pvol, null=("gather",), n_rays=0, n_streams=0) == INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30):
        assert _check(pvol, max_dist=bad) == INVALID, bad
    for bad in (0, -3, 257):
        assert _check(pvol, n_samples=bad) == INVALID, bad
    for bad in (1.0, -1.0, 2.0, float("nan")):
        assert _check(pvol, cos=bad) == INVALID, bad
    assert _check(pvol, null=("u_bsdf",)) == INVALID
    assert _check(pvol, null=("u_photon",)) == INVALID
    # 3. no scene
    assert _check(pvol, have_scene=0) == NO_SCENE
    assert _check(pvol, have_scene=0, n_rays=0, n_streams=0) == NO_SCENE
    # 4. a density region, whether or not a surface integrator is on
    for vol in (GRID, EXPONENTIAL):
        assert _check(pvol, vol=vol) == UNSUPPORTED
        assert _check(pvol, vol=vol, surf=0) == UNSUPPORTED
    # 5. to 8.
    assert _check(pvol, surf=0) == INVALID
    assert _check(pvol, indirect=1) == INVALID and _check(pvol, indirect=50000) == INVALID
    assert _check(pvol, gather=0) == INVALID
    assert _check(pvol, rad=0) == INVALID
    assert _check(pvol, rad_n=0) == INVALID
    assert _check(pvol, rad_n=0, n_rays=0, n_streams=0) == INVALID
    # two faults at once: the earlier one in the order is reported.  INVALID stands on both sides of NO_SCENE and UNSUPPORTED, so the
    # order shows where a fault of group 2 meets a missing scene or a density region, and where those meet the faults of 5 to 8
    assert _check(pvol, have_ctx=0, have_scene=0) == INVALID
    assert _check(pvol, kind=5, have_scene=0) == INVALID
    assert _check(pvol, null=("L",), have_scene=0) == INVALID
    assert _check(pvol, null=("gather",), have_scene=0) == INVALID
    assert _check(pvol, n_samples=0, have_scene=0) == INVALID
    assert _check(pvol, null=("u_photon",), vol=GRID) == INVALID
    assert _check(pvol, cos=1.0, vol=GRID) == INVALID
    assert _check(pvol, have_scene=0, vol=GRID) == NO_SCENE
    assert _check(pvol, have_scene=0, surf=0, gather=0, rad=0) == NO_SCENE
    assert _check(pvol, vol=GRID, surf=0, indirect=9, gather=0, rad=0) == UNSUPPORTED
    assert _check(pvol, vol=EXPONENTIAL, gather=0) == UNSUPPORTED
    assert _check(pvol, surf=0, indirect=9, gather=0, rad=0) == INVALID


def test_batch_check_is_untouched(pvol):
    """pvol_radiance_batch_check still passes a density region without a surface integrator, which the gather's check refuses."""
    buf = np.zeros(64, F)
    out = abi.RadianceOut(L=buf.ctypes.data)
    a = abi.RadianceBatchCheck(buf.ctypes.data, buf.ctypes.data, 4, 2, abi.OUT_SPECTRAL, C.pointer(out))
    f = pvol.lib().pvol_radiance_batch_check
    assert f(1, C.byref(a), 1, GRID, 0) == OK and f(1, C.byref(a), 1, GRID, 1) == UNSUPPORTED and f(1, C.byref(a), 0, GRID, 1) == NO_SCENE


def test_slice_planner(pvol):
    f, old = pvol.lib().pvol_radiance_gather_slice, pvol.lib().pvol_radiance_slice
    ray, caller, top = abi.RADIANCE_RAY_SCRATCH, abi.RADIANCE_CALLER_SCRATCH, abi.RADIANCE_SCRATCH_BYTES
    assert abi.radiance_gather_scratch(1) == (3 + 9 + 3 + 30 + 1) * 4 + 30 * 4 + 4 + 2 * 12
    assert abi.radiance_gather_scratch(16) - abi.radiance_gather_scratch(15) == 2 * 3 * 4

    def per(ns):
        return ray + abi.radiance_gather_scratch(ns) + caller
    last = None
    for ns in (1, 3, 4, 16, 256):
        whole = top // per(ns)
        assert f(ns, 0) == f(ns, top) == f(ns, top + 1) == f(ns, 1 << 40) == whole - whole % 64   # the hook only lowers the bound
        assert f(ns, per(ns) * 64) == 64 and f(ns, per(ns) * 65 - 1) == 64
        assert f(ns, per(ns) * 127) == 64 and f(ns, per(ns) * 128) == 128      # whole runs of 64 where that many fit
        assert f(ns, per(ns) * 50) == 50 and f(ns, per(ns) * 63) == 63         # below one run: what fits
        assert f(ns, per(ns)) == 1 and f(ns, per(ns) - 1) == 1 and f(ns, 1) == 1
        for bound in (per(ns) * 1000, per(ns) * 4097 + 5, 123456789):
            n = f(ns, bound)
            assert n * per(ns) <= bound < (n + 64) * per(ns) and n % 64 == 0
        assert last is None or f(ns, 0) < last      # more samples, fewer rays in a slice
        assert f(ns, 0) < old(0, 0)                 # ... and always fewer than the call that does not gather
        last = f(ns, 0)
    assert f(256, 0) >= 30000                       # 256 samples: still launches of tens of thousands of rays
    # the existing planner's answers, as tests/test_radiance_rays.py pins them, restated from its formula
    for seg in (0, 2, 30):
        each = (seg + 1) * ray + caller
        whole = top // each
        assert old(seg, 0) == old(seg, top) == whole - whole % 64
        assert old(seg, each * 64) == 64 and old(seg, each * 50) == 50 and old(seg, 1) == 1
    assert ray == 324 and caller == 248 and old(0, 0) == 469248 and old(30, 0) == 26048
    # the cut's answers for the entry point that does not gather: blocks of 1, 3, 1, 7 ... under a budget of two rays
    offs = np.array([0, 1, 4, 5, 12], np.uint32)
    cut = pvol.lib().pvol_radiance_slice_cut
    assert cut(offs.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 5 * ray + 3 * caller) == 3
    assert cut(offs.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 12 * ray + 4 * caller) == 4
    assert cut(offs.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 1) == 1


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "rg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvol.h"\n#define O(t, m) offsetof(t, m)\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pvol_gather_params), O(pvol_gather_params, max_dist), O(pvol_gather_params, n_samples),'
                   "O(pvol_gather_params, cos_gather_angle), O(pvol_gather_params, u_bsdf), O(pvol_gather_params, u_photon));"
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pvol_radiance_gather_out), O(pvol_radiance_gather_out, L), O(pvol_radiance_gather_out, surf_xyz),'
                   "O(pvol_radiance_gather_out, t_hit), O(pvol_radiance_gather_out, draws), O(pvol_radiance_gather_out, surf_draws),"
                   "O(pvol_radiance_gather_out, n_segments), O(pvol_radiance_gather_out, gather_draws));"
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pvol_radiance_out), O(pvol_radiance_out, L), O(pvol_radiance_out, surf_xyz), O(pvol_radiance_out, t_hit),'
                   "O(pvol_radiance_out, draws), O(pvol_radiance_out, surf_draws), O(pvol_radiance_out, n_segments));"
                   'printf("%d %llu\\n", PVOL_ABI_VERSION, (unsigned long long)PVOL_RADIANCE_SCRATCH_BYTES);return 0;}\n')
    exe = tmp_path / "rg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    G, R, R0 = abi.GatherParams, abi.RadianceGatherOut, abi.RadianceOut
    assert lines[0] == [C.sizeof(G), G.max_dist.offset, G.n_samples.offset, G.cos_gather_angle.offset, G.u_bsdf.offset, G.u_photon.offset] == [32, 0, 4, 8, 16, 24]
    assert lines[1] == [C.sizeof(R)] + [getattr(R, n).offset for n, _ in R._fields_] == [56, 0, 8, 16, 24, 32, 40, 48]
    assert lines[2] == [C.sizeof(R0)] + [getattr(R0, n).offset for n, _ in R0._fields_] == [48, 0, 8, 16, 24, 32, 40]   # the old struct: unchanged
    assert lines[1][1:7] == lines[2][1:]            # pvol_radiance_out's members in their order
    assert lines[3] == [3, abi.RADIANCE_SCRATCH_BYTES]
    assert [n for n, _ in R._fields_][1:] == list(abi.RADIANCE_GATHER_WANT)


def test_entry_points_without_a_context(pvol):
    L = pvol.lib()
    buf = np.full(256, 7, F)
    out = abi.RadianceGatherOut(L=buf.ctypes.data, t_hit=buf.ctypes.data, gather_draws=buf.ctypes.data)
    g = abi.GatherParams(0.5, 2, 0.9, buf.ctypes.data, buf.ctypes.data)
    assert L.pvol_radiance_gather_batch(None, buf.ctypes.data, 2, buf.ctypes.data, 1, abi.OUT_SPECTRAL, C.byref(g), C.byref(out)) == INVALID
    assert L.pvol_radiance_gather_batch_device(None, buf.ctypes.data, 2, buf.ctypes.data, 1, abi.OUT_XYZ, C.byref(g), C.byref(out), None) == INVALID
    assert L.pvol_radiance_gather_batch(None, None, 0, None, 0, abi.OUT_SPECTRAL, None, None) == INVALID
    assert (buf == 7).all()


def test_fails_loudly_without_a_device(pvol):
    """No CPU path: without a HIP device no context can be made.  Where there is a device, a context without a scene answers
    PVOL_E_NO_SCENE, and a fault in the gather's arguments comes before that."""
    params = abi.params_from_blob(load_scene("volumescene_h"))
    if pvol.lib().pvol_device_count() < 1:
        with pytest.raises(pvol.PvolError) as e:
            pvol.PhotonVolume(params)
        assert e.value.status == abi.PVOL_E_NO_DEVICE
        return
    pv = pvol.PhotonVolume(params)
    try:
        rays = abi.make_rays(np.zeros((2, 3), F), np.tile(F([0, 0, 1]), (2, 1)), 0.0, np.inf, 0.5)
        u = np.zeros((2, 1, 3), F)
        with pytest.raises(pvol.PvolError) as e:
            pv.radiance_gather_batch(rays, abi.make_streams([0], [2]), 0.5, 0.9, u, u)
        assert e.value.status == NO_SCENE
        with pytest.raises(pvol.PvolError) as e:
            pv.radiance_gather_batch(rays, abi.make_streams([0], [2]), 0.0, 0.9, u, u)
        assert e.value.status == INVALID
    finally:
        pv.close()


def test_symbols_are_exported(pvol):
    assert "pvol_radiance_gather_batch" in pvol.EXPORTS and "pvol_radiance_gather_batch_device" in pvol.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", pvol.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("pvol_radiance_gather_batch", "pvol_radiance_gather_batch_device", "pvol_radiance_gather_check", "pvol_radiance_gather_slice",
                "pvol_radiance_batch", "pvol_radiance_batch_check", "pvol_final_gather_device"):
        assert sym in names, sym
    header = open(os.path.join(ROOT, "include", "pvol.h")).read()
    assert "pvol_radiance_gather_check" not in header.replace("(pvol_radiance_gather_check)", "")   # for the tests, not declared
    assert "int pvol_radiance_gather_batch(" in header and "int pvol_radiance_gather_batch_device(" in header
    assert pvol.lib().pvol_abi_version() == 3
    for name in ("radiance_gather_batch", "radiance_gather_batch_device"):
        assert hasattr(pvol.PhotonVolume, name)
