"""CPU-side checks of the single-process multi-GPU entry points (pvol_preprocess_group, pvol_render_frame_group): declared,
exported, bound, and their argument checks run before any context or device is touched."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, abi


@pytest.fixture(scope="module")
def pvol():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def test_group_entry_points_are_declared_and_exported(pvol):
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    assert "int pvol_preprocess_group(pvol_ctx *const *ctxs, uint32_t n_ctx, uint32_t n_tasks, uint32_t block_paths);" in text
    assert "int pvol_render_frame_group(pvol_ctx *const *ctxs, uint32_t n_ctx, const pvol_camera *camera, const pvol_film *film," in text
    for name in ("pvol_preprocess_group", "pvol_render_frame_group"):
        assert hasattr(pvol.lib(), name) and name in pvol.EXPORTS
    assert callable(pvol.preprocess_group) and callable(pvol.render_frame_group)
    assert pvol.lib().pvol_abi_version() == 3


def test_group_calls_reject_bad_arguments_before_touching_anything(pvol):
    L = pvol.lib()
    bufs = [C.create_string_buffer(64) for _ in range(3)]   # never dereferenced: every call below fails its argument checks first
    a, b, c = (C.cast(x, C.c_void_p).value for x in bufs)
    ctxs = lambda *v: (C.c_void_p * max(len(v), 1))(*v)   # noqa: E731
    inv = abi.PVOL_E_INVALID
    # pvol_preprocess_group
    assert L.pvol_preprocess_group(None, 2, 16, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, b), 0, 16, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, b), 65, 16, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, None), 2, 16, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, b, a), 3, 16, 4096) == inv      # a context listed twice
    assert L.pvol_preprocess_group(ctxs(a, b), 2, 0, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, b), 2, 65537, 4096) == inv
    assert L.pvol_preprocess_group(ctxs(a, b), 2, 16, 0) == inv
    assert L.pvol_preprocess_group(ctxs(a, b), 2, 16, 4097) == inv
    # pvol_render_frame_group
    px = [C.create_string_buffer(4 * 4 * 4 + 16) for _ in range(3)]
    aligned = [(C.addressof(x) + 15) & ~15 for x in px]
    cam, smp = abi.Camera(), abi.Sampler()
    film = abi.make_film(2, 2, pvol.gaussian_filter_table())
    pix = lambda *v: (C.c_void_p * max(len(v), 1))(*v)   # noqa: E731
    good = pix(*aligned)
    R = L.pvol_render_frame_group
    assert R(None, 3, C.byref(cam), C.byref(film), C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, c), 0, C.byref(cam), C.byref(film), C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, c), 65, C.byref(cam), C.byref(film), C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, c), 3, None, C.byref(film), C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, c), 3, C.byref(cam), None, C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, c), 3, C.byref(cam), C.byref(film), None, good, None, None) == inv
    assert R(ctxs(a, b, c), 3, C.byref(cam), C.byref(film), C.byref(smp), None, None, None) == inv
    assert R(ctxs(a, None, c), 3, C.byref(cam), C.byref(film), C.byref(smp), good, None, None) == inv
    assert R(ctxs(a, b, a), 3, C.byref(cam), C.byref(film), C.byref(smp), good, None, None) == inv          # duplicate context
    assert R(ctxs(a, b, c), 3, C.byref(cam), C.byref(film), C.byref(smp), pix(aligned[0], None, aligned[2]), None, None) == inv
    assert R(ctxs(a, b, c), 3, C.byref(cam), C.byref(film), C.byref(smp), pix(aligned[0], aligned[1] + 4, aligned[2]), None, None) == inv
    empty = abi.make_film(2, 2, pvol.gaussian_filter_table())
    empty.x_resolution = 0
    assert R(ctxs(a, b, c), 3, C.byref(cam), C.byref(empty), C.byref(smp), good, None, None) == inv
    # the Python wrappers raise with the status
    with pytest.raises(pvol.PvolError) as e:
        pvol.preprocess_group([], 16)
    assert e.value.status == inv
