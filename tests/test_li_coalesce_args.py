"""CPU-side checks of the batched per-sample entry points (pvol_li_many, pvol_set_li_coalescing,
pvol_get_li_coalescing_stats): bad arguments are refused with PVOL_E_INVALID before anything touches the
context or a device, so these run without a GPU."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, abi


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    return importlib.import_module("cs348b-pbrt_amd.pvol").lib()


@pytest.fixture
def bogus():
    """A context pointer no entry point may dereference on the paths below (a poisoned buffer, not a pvol_ctx)."""
    buf = C.create_string_buffer(b"\xa5" * 4096)
    return C.cast(buf, C.c_void_p), buf


def _arrays(n):
    rays = np.zeros(max(n, 1), abi.RAY_DTYPE)
    mt = np.zeros((max(n, 1), 624), np.uint32)
    mti = np.full(max(n, 1), 624, np.int32)
    Lv = np.zeros((max(n, 1), 30), np.float32)
    T = np.zeros((max(n, 1), 30), np.float32)
    st = np.zeros(max(n, 1), np.int32)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    return rays, mt, mti, Lv, T, st, [rays.ctypes.data, ptr(mt, C.c_uint32), ptr(mti, C.c_int32), ptr(Lv, C.c_float), ptr(T, C.c_float),
                                      ptr(st, C.c_int32)]


def test_null_context_is_refused(L):
    rays, mt, mti, Lv, T, st, a = _arrays(2)
    assert L.pvol_li_many(None, a[0], 2, *a[1:]) == abi.PVOL_E_INVALID
    assert L.pvol_set_li_coalescing(None, 64, 0) == abi.PVOL_E_INVALID
    out = (C.c_uint64 * 6)()
    assert L.pvol_get_li_coalescing_stats(None, out, 0) == abi.PVOL_E_INVALID


def test_li_many_refuses_null_arrays_and_bad_states_before_touching_the_context(L, bogus):
    ctx, _ = bogus
    rays, mt, mti, Lv, T, st, a = _arrays(3)
    for k in range(5):   # each required array in turn (status is optional)
        args = list(a)
        args[k] = None
        assert L.pvol_li_many(ctx, args[0], 3, *args[1:]) == abi.PVOL_E_INVALID, k
    for bad in (-1, 625, 700):
        mti[:] = 624
        mti[1] = bad
        assert L.pvol_li_many(ctx, a[0], 3, *a[1:]) == abi.PVOL_E_INVALID, bad
    assert not mt.any() and not Lv.any() and not T.any() and not st.any()   # nothing was written


def test_li_many_of_no_calls_does_nothing(L, bogus):
    ctx, _ = bogus
    assert L.pvol_li_many(ctx, None, 0, None, None, None, None, None) == abi.PVOL_OK


def test_coalescing_settings_out_of_range_are_refused(L, bogus):
    ctx, _ = bogus
    for max_batch, wait in [(4097, 0), (1 << 31, 0), (64, 1001), (0, 5000)]:
        assert L.pvol_set_li_coalescing(ctx, max_batch, wait) == abi.PVOL_E_INVALID, (max_batch, wait)
    assert L.pvol_get_li_coalescing_stats(ctx, None, 0) == abi.PVOL_E_INVALID


def test_header_declares_the_batched_entry_points():
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    for name in ("pvol_li_many", "pvol_set_li_coalescing", "pvol_get_li_coalescing_stats"):
        assert name + "(" in text
