"""The plan of a render call (pvol_render_plan in csrc/pvol_render_host.hip, exported for the tests as pvol_render_plan_flat next to
pvol_plan_batch and pvol_check_scene): the status pvol_render_tasks_window_device gives its arguments, every task's sub-window and sample
count, the cut of the task list into batches and what each batch reserves and uploads, decided by pure host code.  The model below is
written from core/sampler.cpp:55-74 (in float32, as bench.frame_tiles restates it) and from the loop the entry point had before the plan
existed, not produced by running the plan.  No GPU."""
import ctypes as C
import copy
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import RENDER_CASES, RENDER_SPECULAR_CASES, RENDER_SURF_CASES, ROOT, abi, load_render_case

OK, INVALID, NO_SCENE, UNSUPPORTED, LIMIT = abi.PVOL_OK, abi.PVOL_E_INVALID, abi.PVOL_E_NO_SCENE, abi.PVOL_E_UNSUPPORTED, abi.PVOL_E_LIMIT
RAY, STREAM, TAU_REC = 48, 32, 8   # sizeof(pvol_ray), sizeof(pvol_stream), sizeof(TauRec)
_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    L.pvol_render_plan_flat.argtypes = [C.POINTER(abi.Camera), C.POINTER(abi.Film), C.POINTER(abi.FilmWindow), C.POINTER(abi.Sampler), _u32p,
                                        C.c_uint32, C.POINTER(C.c_int32), C.c_int64, _u64p, C.c_size_t]
    L.pvol_render_plan_flat.restype = C.c_size_t
    return L


def _signed(v):
    return int(v) - (1 << 64) if int(v) >> 63 else int(v)


def plan(lib, cam, film, smp, tasks, knob=0, window=None, pixels=True, scene=True, surf=False, spec=False, null_tasks=False):
    """The plan as a dict; only {"rc": ...} when the call is refused."""
    ids = np.ascontiguousarray(tasks, np.uint32)
    flags = (C.c_int32 * 4)(pixels, scene, surf, spec)
    ref = lambda o: None if o is None else C.byref(o)   # noqa: E731
    args = [ref(cam), ref(film), ref(window), ref(smp),
            None if null_tasks else ids.ctypes.data_as(_u32p), len(ids), flags, knob]
    n = lib.pvol_render_plan_flat(*args, None, 0)
    out = np.zeros(n, np.uint64)
    assert lib.pvol_render_plan_flat(*args, out.ctypes.data_as(_u64p), n) == n >= 1
    p = {"rc": _signed(out[0])}
    if p["rc"] != OK:
        assert n == 1
        return p
    w = [int(v) for v in out]
    p["batchRays"], nt, nb = w[1:4]
    p["spp"], p["n1dCount"], p["n2dCount"], p["scatterIndex"] = w[4:8]
    p["n1d"], p["n2d"] = w[8:24], w[24:40]
    p["shutter"] = np.array(w[40:42], np.uint32).view(np.float32)
    p["r2c"], p["c2w"] = np.array(w[42:58], np.uint32).view(np.float32), np.array(w[58:74], np.uint32).view(np.float32)
    t = np.array(w[74:74 + 11 * nt], np.uint64).reshape(nt, 11)
    p["win"] = [[_signed(v) for v in r[:4]] for r in t]
    p["count"] = [int(r[4]) for r in t]
    p["streams"] = [tuple(int(v) for v in r[5:]) for r in t]   # seed, first_ray, n_rays, reserved, start_draw, end_draw
    b = np.array(w[74 + 11 * nt:], np.uint64).reshape(nb, 14)
    p["batches"] = [dict(b0=int(r[0]), b1=int(r[1]), nRays=int(r[2]), maxRays=int(r[3]), doneRays=int(r[4]), surfOn=int(r[5]), specOn=int(r[6]),
                         want=[int(v) for v in r[7:]]) for r in b]
    return p


# ---- the model
def sub_windows(smp, tasks):
    """Sampler::ComputeSubWindow (core/sampler.cpp:55-74) of every task of the list, in fp32: x0, x1, y0, y1."""
    f32 = np.float32
    dx, dy = smp.x_end - smp.x_start, smp.y_end - smp.y_start
    nx, ny = int(smp.n_tasks), 1
    while (nx & 1) == 0 and 2 * dx * ny < dy * nx:
        nx >>= 1
        ny <<= 1
    num = np.asarray(tasks, np.int64)
    xo, yo = num % nx, num // nx

    def lerp_floor(k, n, lo, hi):   # Floor2Int(Lerp(float(k) / float(n), lo, hi))
        t = k.astype(f32) / f32(n)
        return np.floor((f32(1) - t) * f32(lo) + t * f32(hi)).astype(np.int64)
    return np.stack([lerp_floor(xo, nx, smp.x_start, smp.x_end), lerp_floor(xo + 1, nx, smp.x_start, smp.x_end),
                     lerp_floor(yo, ny, smp.y_start, smp.y_end), lerp_floor(yo + 1, ny, smp.y_start, smp.y_end)], 1)


def model(smp, tasks, knob=0, surf=False, spec=False):
    """The parent's loop: sub-windows and counts, the budget, the greedy cut, the stream tables, the seven pvol_reserve sizes."""
    win = sub_windows(smp, tasks)
    count = [int(c) for c in (win[:, 1] - win[:, 0]) * (win[:, 3] - win[:, 2]) * smp.pixel_samples]
    budget = min(knob if knob > 0 else 256 << 20, 0xfffff000)
    m = {"rc": LIMIT if any(c > budget for c in count) else OK}
    if m["rc"] != OK:
        return m
    m.update(batchRays=budget, win=[[int(v) for v in r] for r in win], count=count, streams=[None] * len(count), batches=[])
    b0, done = 0, 0
    while b0 < len(count):
        b1, n, mx = b0, 0, 0
        while b1 < len(count) and n + count[b1] <= budget:
            m["streams"][b1] = (int(tasks[b1]), n, count[b1], 0, 0, 0)
            n += count[b1]
            mx = max(mx, count[b1])
            b1 += 1
        s_on = int(bool(surf and n))
        p_on = int(bool(s_on and spec))
        want = [max(RAY * n, 64), max(8 * n, 64), max(16 * n, 64), STREAM * (b1 - b0), 16 * (b1 - b0), TAU_REC * n if s_on else 0, 4 * n if p_on else 0]
        m["batches"].append(dict(b0=b0, b1=b1, nRays=n, maxRays=mx, doneRays=done, surfOn=s_on, specOn=p_on, want=want))
        done += n
        b0 = b1
    return m


def assert_plan_is_model(p, m):
    assert p["rc"] == m["rc"]
    for k in ("batchRays", "win", "count", "streams", "batches"):
        if k in m:
            assert p[k] == m[k], k


# ---- golden cases
ALL_CASES = [(n, False, False) for n in RENDER_CASES] + [(n, True, False) for n in RENDER_SURF_CASES] + [(n, True, True) for n in RENDER_SPECULAR_CASES]


@pytest.mark.parametrize("name,surf,spec", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_every_golden_render_is_one_batch_of_the_model(lib, name, surf, spec):
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    s, prm, cam, film, smp, c = load_render_case(name)
    tasks = np.asarray(c["tasks"], np.uint32)
    p = plan(lib, cam, film, smp, tasks, surf=surf, spec=spec)
    assert p["rc"] == OK and len(p["batches"]) == 1
    assert sum(p["count"]) == pvol.render_sample_count(smp, tasks) == len(c["samples.time"])
    assert_plan_is_model(p, model(smp, tasks, surf=surf, spec=spec))
    b = p["batches"][0]
    assert (b["surfOn"], b["specOn"]) == (int(surf), int(spec)) and (b["want"][5] > 0, b["want"][6] > 0) == (surf, spec)
    # what the kernels get of camera and sampler
    assert (p["spp"], p["n1dCount"], p["n2dCount"], p["scatterIndex"]) == (smp.pixel_samples, smp.n1d_count, smp.n2d_count, smp.scatter_index)
    assert p["n1d"] == list(smp.n1d) and p["n2d"] == list(smp.n2d)
    assert p["shutter"].tolist() == [cam.shutter_open, cam.shutter_close]
    assert p["r2c"].tolist() == list(cam.raster_to_camera) and p["c2w"].tolist() == list(cam.camera_to_world)


# ---- cuts
def _frame(dx, dy, spp, n_tasks):
    """A camera, a film and a sampler whose sample extent is dx x dy (the plan reads nothing else of the frame)."""
    s, prm, cam, film, smp, c = load_render_case("vh")
    smp = copy.copy(smp)
    smp.x_start, smp.x_end, smp.y_start, smp.y_end = -2, dx - 2, -2, dy - 2
    smp.pixel_samples, smp.n_tasks = spp, n_tasks
    return cam, film, smp


EXTENTS = [(4, 2), (13, 7), (96, 54)]


def _task_counts(dx, dy):
    above = 1
    while above <= dx * dy:
        above <<= 1
    return [1, 4, 64, above]   # the last: more tasks than pixels, so some tasks are empty


CUTS = [(dx, dy, n) for dx, dy in EXTENTS for n in _task_counts(dx, dy)]


@pytest.mark.parametrize("dx,dy,n_tasks", CUTS, ids=["%dx%d-%d" % c for c in CUTS])
def test_cuts_are_greedy_and_in_order(lib, dx, dy, n_tasks):
    for spp in (1, 16):
        cam, film, smp = _frame(dx, dy, spp, n_tasks)
        ids = np.arange(n_tasks, dtype=np.uint32)
        for tasks in (ids, ids[::-1], ids[::3]):
            free = model(smp, tasks)
            count, largest, total = free["count"], max(free["count"]), sum(free["count"])
            if len(tasks) == n_tasks:
                assert total == dx * dy * spp and (0 in count or n_tasks <= dx * dy)
            for knob in (largest, largest + 1, total, total - 1, 0):
                p, m = plan(lib, cam, film, smp, tasks, knob, surf=True, spec=True), model(smp, tasks, knob, True, True)
                assert_plan_is_model(p, m)
                if m["rc"] == LIMIT:   # a single non-empty task: no budget below it holds it
                    assert knob == total - 1 and 0 < knob < largest
                    continue
                assert p["rc"] == OK
                budget, bs = p["batchRays"], p["batches"]
                assert budget == (knob if knob > 0 else 256 << 20)
                # the batches partition the list in order; doneRays and first_ray are the running sums
                assert bs[0]["b0"] == 0 and bs[-1]["b1"] == len(tasks) and all(a["b1"] == b["b0"] for a, b in zip(bs, bs[1:]))
                done = 0
                for k, b in enumerate(bs):
                    assert b["b1"] > b["b0"] and b["doneRays"] == done
                    mine = count[b["b0"]:b["b1"]]
                    assert b["nRays"] == sum(mine) <= budget and b["maxRays"] == max(mine)
                    first = 0
                    for i in range(b["b0"], b["b1"]):
                        assert p["streams"][i] == (int(tasks[i]), first, count[i], 0, 0, 0)
                        first += count[i]
                    if k + 1 < len(bs):   # maximal: the next task would not fit
                        assert b["nRays"] + count[b["b1"]] > budget
                    done += b["nRays"]
                assert done == total
                if knob in (total, 0):
                    assert len(bs) == 1
            if largest > 1:
                assert plan(lib, cam, film, smp, tasks, largest - 1)["rc"] == LIMIT
        p = plan(lib, cam, film, smp, [], surf=True, spec=True)
        assert p["rc"] == OK and p["batches"] == [] and p["count"] == []


def test_a_batch_of_empty_tasks_switches_the_surface_term_off(lib):
    cam, film, smp = _frame(4, 2, 16, 16)
    counts = model(smp, np.arange(16))["count"]
    empty = [t for t in range(16) if counts[t] == 0]
    assert 0 < len(empty) < 16
    for surf, spec in ((False, False), (True, False), (True, True)):
        p = plan(lib, cam, film, smp, empty, surf=surf, spec=spec)
        assert p["rc"] == OK and len(p["batches"]) == 1
        b = p["batches"][0]
        assert (b["nRays"], b["maxRays"], b["surfOn"], b["specOn"]) == (0, 0, 0, 0)
        assert b["want"] == [64, 64, 64, STREAM * len(empty), 16 * len(empty), 0, 0]


def test_flags_add_the_tau_and_link_buffers(lib):
    cam, film, smp = _frame(13, 7, 16, 4)
    tasks = np.arange(4, dtype=np.uint32)
    counts = model(smp, tasks)["count"]
    for surf, spec in ((False, False), (False, True), (True, False), (True, True)):
        p = plan(lib, cam, film, smp, tasks, max(counts), surf=surf, spec=spec)
        assert p["rc"] == OK and len(p["batches"]) > 1
        for b in p["batches"]:
            n = b["nRays"]
            assert n > 0 and (b["surfOn"], b["specOn"]) == (int(surf), int(surf and spec))   # no specular recursion without the surface integrator
            assert b["want"] == [RAY * n, 64 if 8 * n < 64 else 8 * n, 16 * n, STREAM * (b["b1"] - b["b0"]), 16 * (b["b1"] - b["b0"]),
                                 TAU_REC * n if surf else 0, 4 * n if surf and spec else 0]


# ---- status paths: (id, expected status, edits), in the order of the checks.  An edit names what it changes: cam / film / smp fields,
# "window", or a keyword of plan()
def _status(lib, *edits):
    cam, film, smp = _frame(13, 7, 4, 4)
    cam, film = copy.copy(cam), copy.copy(film)
    kw = dict(tasks=[0, 1, 2, 3], knob=0)
    objs = {"cam": cam, "film": film, "smp": smp}
    for e in edits:
        for k, v in e.items():
            if "." in k:
                o, f = k.split(".")
                if f.endswith("]"):
                    getattr(objs[o], f[:f.index("[")])[int(f[f.index("[") + 1:-1])] = v
                else:
                    setattr(objs[o], f, v)
            elif k in objs:
                objs[k] = v
            else:
                kw[k] = v
    tasks = kw.pop("tasks")
    return plan(lib, objs["cam"], objs["film"], objs["smp"], tasks, **kw)["rc"]


NULL_CAMERA, NO_PIXELS, NO_SCENE_YET = {"cam": None}, {"pixels": False}, {"scene": False}
SPP_3, THIN_LENS, ARRAYS_17 = {"smp.pixel_samples": 3}, {"cam.lens_radius": 0.1}, {"smp.n1d_count": 17}
BAD_SCATTER, NO_TASKS, BAD_ID = {"smp.scatter_index": 2}, {"smp.n_tasks": 0}, {"tasks": [0, 4]}
SMALL_BUDGET = {"knob": 1}
ONE_FAULT = [
    ("null_camera", INVALID, NULL_CAMERA),
    ("null_sampler", INVALID, {"smp": None}),
    ("null_film", INVALID, {"film": None}),
    ("film_filter_wider_than_3", INVALID, {"film.filter_xwidth": 3.5}),
    ("window_past_the_frame", INVALID, {"window": abi.FilmWindow(30, 0, 8, 8)}),
    ("null_task_list", INVALID, {"null_tasks": True}),
    ("null_pixels", INVALID, NO_PIXELS),
    ("no_scene", NO_SCENE, NO_SCENE_YET),
    ("spp_0", INVALID, {"smp.pixel_samples": 0}),
    ("spp_3", INVALID, SPP_3),
    ("spp_2048", INVALID, {"smp.pixel_samples": 2048}),
    ("thin_lens", UNSUPPORTED, THIN_LENS),
    ("17_1d_arrays", LIMIT, ARRAYS_17),
    ("17_2d_arrays", LIMIT, {"smp.n2d_count": 17}),
    ("scatter_index_past_the_arrays", INVALID, BAD_SCATTER),
    ("scatter_array_of_two", INVALID, {"smp.n1d[1]": 2}),
    ("no_tasks_in_the_frame", INVALID, NO_TASKS),
    ("inverted_extent", INVALID, {"smp.x_end": -3}),
    ("task_id_out_of_range", INVALID, BAD_ID),
    ("task_larger_than_the_budget", LIMIT, SMALL_BUDGET),
]
# the earlier check wins
TWO_FAULTS = [
    ("null_pixels_before_no_scene", INVALID, NO_PIXELS, NO_SCENE_YET),
    ("null_camera_before_array_counts", INVALID, NULL_CAMERA, ARRAYS_17),
    ("no_scene_before_spp", NO_SCENE, NO_SCENE_YET, SPP_3),
    ("no_scene_before_thin_lens", NO_SCENE, NO_SCENE_YET, THIN_LENS),
    ("spp_before_thin_lens", INVALID, SPP_3, THIN_LENS),
    ("thin_lens_before_array_counts", UNSUPPORTED, THIN_LENS, ARRAYS_17),
    ("array_counts_before_scatter_index", LIMIT, ARRAYS_17, BAD_SCATTER),
    ("scatter_index_before_the_budget", INVALID, BAD_SCATTER, SMALL_BUDGET),
    ("array_counts_before_no_tasks", LIMIT, ARRAYS_17, NO_TASKS),
    ("task_id_before_the_budget", INVALID, BAD_ID, SMALL_BUDGET),
    ("thin_lens_before_the_budget", UNSUPPORTED, THIN_LENS, SMALL_BUDGET),
]


def test_the_mutated_call_is_accepted_unmutated(lib):
    assert _status(lib) == OK
    assert _status(lib, {"window": abi.FilmWindow(2, 1, 8, 8)}) == OK
    assert _status(lib, {"tasks": [], "null_tasks": True}) == OK   # no list needed for no tasks


@pytest.mark.parametrize("want,edit", [c[1:] for c in ONE_FAULT], ids=[c[0] for c in ONE_FAULT])
def test_one_mutation_per_status_path(lib, want, edit):
    assert _status(lib, edit) == want


@pytest.mark.parametrize("want,first,second", [c[1:] for c in TWO_FAULTS], ids=[c[0] for c in TWO_FAULTS])
def test_two_faults_answer_with_the_earlier_check(lib, want, first, second):
    assert _status(lib, first, second) == want
    assert _status(lib, second) != want   # the later fault alone answers differently


def test_the_hook_is_no_part_of_the_abi(lib):
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert "pvol_render_plan" not in open(os.path.join(ROOT, "include", "pvol.h")).read()   # a test entry like pvol_plan_batch, not ABI
    assert not [e for e in pvol.EXPORTS if "render_plan" in e]
    assert lib.pvol_render_plan_flat(None, None, None, None, None, 0, None, 0, None, 0) == 0   # no flags: no plan
