"""pvol_radiance_batch without a GPU: every status of pvol_radiance_batch_check in its order, the slice planner, the
layout of pvol_radiance_out against its ctypes mirror, the entry points without a context and without a device, the exported symbols,
and what the GPU tests rest on in the committed captures (rays.skip - surf.draws is the caller's own rng_skip)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import RENDER_SPECULAR_CASES, RENDER_SURF_CASES, ROOT, abi, load_render_case, load_scene

OK, INVALID, NO_SCENE, UNSUPPORTED = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_NO_SCENE, abi.PVOL_E_UNSUPPORTED
NONE, HOMOGENEOUS, GRID, RAINBOW, EXPONENTIAL = 0, 1, 2, 3, 4   # pvol_volume_kind
F = np.float32


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def _check(pvol, have_ctx=1, have_scene=1, vol=HOMOGENEOUS, surf=0, null=(), n_rays=4, n_streams=2, kind=abi.OUT_SPECTRAL, args=True):
    buf = np.zeros(64, F)
    out = abi.RadianceOut()
    out.L = None if "L" in null else buf.ctypes.data
    a = abi.RadianceBatchCheck()
    a.rays = None if "rays" in null else buf.ctypes.data
    a.streams = None if "streams" in null else buf.ctypes.data
    a.n_rays, a.n_streams, a.output_kind = n_rays, n_streams, kind
    a.out = None if "out" in null else C.pointer(out)
    return pvol.lib().pvol_radiance_batch_check(have_ctx, C.byref(a) if args else None, have_scene, vol, surf)


def test_every_status_in_its_order(pvol):
    assert _check(pvol) == OK
    assert _check(pvol, kind=abi.OUT_XYZ) == OK
    for vol in (NONE, HOMOGENEOUS, GRID, RAINBOW, EXPONENTIAL):
        assert _check(pvol, vol=vol) == OK                       # no surface integrator: every medium
    for vol in (NONE, HOMOGENEOUS, RAINBOW):
        assert _check(pvol, vol=vol, surf=1) == OK
    assert _check(pvol, n_rays=0, n_streams=0, null=("rays", "streams", "out")) == OK   # nothing to do
    assert _check(pvol, n_rays=0, null=("rays", "out")) == OK
    assert _check(pvol, n_rays=0, null=("L",)) == OK
    # 1. no context
    assert _check(pvol, have_ctx=0) == INVALID
    assert _check(pvol, args=False) == INVALID
    # 2. the output kind
    assert _check(pvol, kind=2) == INVALID
    assert _check(pvol, kind=-1) == INVALID
    assert _check(pvol, kind=9, n_rays=0, n_streams=0) == INVALID
    # 3. rays and streams
    assert _check(pvol, null=("rays",)) == INVALID
    assert _check(pvol, null=("streams",)) == INVALID
    assert _check(pvol, null=("streams",), n_rays=0) == INVALID
    # 4. the outputs
    assert _check(pvol, null=("out",)) == INVALID
    assert _check(pvol, null=("L",)) == INVALID
    # 5. no scene
    assert _check(pvol, have_scene=0) == NO_SCENE
    assert _check(pvol, have_scene=0, n_rays=0, n_streams=0) == NO_SCENE
    # 6. a surface integrator over a density region
    assert _check(pvol, vol=GRID, surf=1) == UNSUPPORTED
    assert _check(pvol, vol=EXPONENTIAL, surf=1) == UNSUPPORTED
    assert _check(pvol, vol=GRID, surf=1, n_rays=0, n_streams=0) == UNSUPPORTED
    # two faults at once: the earlier one in the order is reported
    assert _check(pvol, have_ctx=0, kind=5, have_scene=0) == INVALID
    assert _check(pvol, kind=5, have_scene=0) == INVALID
    assert _check(pvol, null=("rays",), have_scene=0) == INVALID
    assert _check(pvol, null=("L",), have_scene=0) == INVALID
    assert _check(pvol, null=("L",), vol=GRID, surf=1) == INVALID
    assert _check(pvol, have_scene=0, vol=GRID, surf=1) == NO_SCENE


def test_max_segments(pvol):
    f = pvol.lib().pvol_radiance_max_segments
    assert [f(1, d) for d in range(0, 7)] == [0, 0, 2, 6, 14, 30, 30]   # 2 + 4 + ... + 2^(d - 1); the walk stops at depth 5
    assert [f(0, d) for d in range(0, 7)] == [0] * 7                    # no glass, or no surface integrator: nothing is spawned


def test_slice_planner(pvol):
    f = pvol.lib().pvol_radiance_slice
    ray, caller, top = abi.RADIANCE_RAY_SCRATCH, abi.RADIANCE_CALLER_SCRATCH, abi.RADIANCE_SCRATCH_BYTES
    assert ray == 48 + 32 + 240 + 4 and caller == 240 + 8

    def per(seg):
        return (seg + 1) * ray + caller
    for seg in (0, 2, 30):
        whole = top // per(seg)
        assert f(seg, 0) == f(seg, top) == f(seg, top + 1) == f(seg, 1 << 40) == whole - whole % 64   # the hook only lowers the bound
        assert f(seg, per(seg) * 64) == 64 and f(seg, per(seg) * 65 - 1) == 64
        assert f(seg, per(seg) * 127) == 64 and f(seg, per(seg) * 128) == 128      # whole runs of 64 where that many fit
        assert f(seg, per(seg) * 50) == 50 and f(seg, per(seg) * 63) == 63         # below one run: what fits
        assert f(seg, per(seg)) == 1 and f(seg, per(seg) - 1) == 1 and f(seg, 1) == 1   # smaller than one ray's worst case: one ray
        for bound in (per(seg) * 1000, per(seg) * 4097 + 5, 123456789):
            n = f(seg, bound)
            assert n * per(seg) <= bound < (n + 64) * per(seg) and n % 64 == 0
    # a call that fits is one slice: 8 000 rays, the largest capture, under the default bound even at depth 5
    assert f(30, 0) >= 8000
    # a boundary inside a stream: 3 streams of 100 rays, slices of 64 -> the cuts 64, 128, 192, 256 fall inside streams 0, 1, 1, 2
    n = f(30, per(30) * 64)
    cuts = list(range(n, 300, n))
    assert n == 64 and [c // 100 for c in cuts] == [0, 1, 1, 2] and all(c % 100 for c in cuts)


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "ro.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvol.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %llu\\n",'
                   "sizeof(pvol_radiance_out),offsetof(pvol_radiance_out,L),offsetof(pvol_radiance_out,surf_xyz),offsetof(pvol_radiance_out,t_hit),"
                   "offsetof(pvol_radiance_out,draws),offsetof(pvol_radiance_out,surf_draws),offsetof(pvol_radiance_out,n_segments),"
                   "(unsigned long long)PVOL_RADIANCE_SCRATCH_BYTES);return 0;}\n")
    exe = tmp_path / "ro"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = abi.RadianceOut
    assert got == [C.sizeof(R), R.L.offset, R.surf_xyz.offset, R.t_hit.offset, R.draws.offset, R.surf_draws.offset, R.n_segments.offset,
                   abi.RADIANCE_SCRATCH_BYTES]
    assert [n for n, _ in R._fields_][1:] == list(abi.RADIANCE_WANT)


def test_entry_points_without_a_context(pvol):
    L = pvol.lib()
    buf = np.full(256, 7, F)
    out = abi.RadianceOut(L=buf.ctypes.data, t_hit=buf.ctypes.data)
    assert L.pvol_radiance_batch(None, buf.ctypes.data, 2, buf.ctypes.data, 1, abi.OUT_SPECTRAL, C.byref(out)) == INVALID
    assert L.pvol_radiance_batch_device(None, buf.ctypes.data, 2, buf.ctypes.data, 1, abi.OUT_XYZ, C.byref(out), None) == INVALID
    assert L.pvol_radiance_batch(None, None, 0, None, 0, abi.OUT_SPECTRAL, None) == INVALID
    assert L.pvol_radiance_set_scratch_bound(None, 1024) == INVALID
    assert (buf == 7).all()


def test_fails_loudly_without_a_device(pvol):
    """No CPU path: without a HIP device no context can be made, so the entry point is out of reach by construction.  Where there is
    a device, a context without a scene answers PVOL_E_NO_SCENE and writes nothing."""
    params = abi.params_from_blob(load_scene("volumescene_h"))
    if pvol.lib().pvol_device_count() < 1:
        with pytest.raises(pvol.PvolError) as e:
            pvol.PhotonVolume(params)
        assert e.value.status == abi.PVOL_E_NO_DEVICE
        return
    pv = pvol.PhotonVolume(params)
    try:
        rays = abi.make_rays(np.zeros((2, 3), F), np.tile(F([0, 0, 1]), (2, 1)), 0.0, np.inf, 0.5)
        with pytest.raises(pvol.PvolError) as e:
            pv.radiance_batch(rays, abi.make_streams([0], [2]))
        assert e.value.status == NO_SCENE
    finally:
        pv.close()


def test_symbols_are_exported(pvol):
    assert "pvol_radiance_batch" in pvol.EXPORTS and "pvol_radiance_batch_device" in pvol.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", pvol.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("pvol_radiance_batch", "pvol_radiance_batch_device", "pvol_radiance_batch_check", "pvol_radiance_slice",
                "pvol_radiance_max_segments", "pvol_radiance_set_scratch_bound"):
        assert sym in names, sym
    assert pvol.lib().pvol_abi_version() == 3
    for name in ("radiance_batch", "radiance_batch_device", "radiance_set_scratch_bound"):
        assert hasattr(pvol.PhotonVolume, name)


SURFACE_CAPTURES = [("vh_surf", RENDER_SURF_CASES, 619), ("vh_surf64", RENDER_SURF_CASES, 9619), ("pf_surf", RENDER_SPECULAR_CASES, 657),
                    ("sph_surf", RENDER_SPECULAR_CASES, 657)]


@pytest.mark.parametrize("name,cases,per_pixel", SURFACE_CAPTURES, ids=[c[0] for c in SURFACE_CAPTURES])
def test_captures_describe_the_callers_input(name, cases, per_pixel):
    """rays.skip - surf.draws takes two values: 0, and the sampler's per-pixel draw count at the first sample of a pixel.  That
    difference is the rng_skip the caller of pvol_radiance_batch passes, so the captures hold the entry point's input and outputs."""
    if name not in cases:
        pytest.skip("capture not among the render cases")
    c = load_render_case(name)[5]
    own = c["rays.skip"].astype(np.int64) - c["surf.draws"].astype(np.int64)
    assert set(np.unique(own).tolist()) == {0, per_pixel}
    assert int(c["task.n_samples"].sum()) == len(own) == len(c["samples.time"])
