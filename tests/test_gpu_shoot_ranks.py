"""pvol_preprocess_ranks: the photon shoot sharded over ranks.  Every rank must end with the map a single-rank
pvol_preprocess_blocks builds -- the same bytes, the same work counters -- and the ranks must agree on every error.

The ranks are fresh child processes (tests/shoot_ranks_worker.py) on the one GPU, joined by a gloo rendezvous over a file and the
host all-gather branch; the RCCL branch runs with a one-rank communicator.  At most three workers have the GPU open at a time and
the test process itself never opens it.  Every worker has a time limit; a worker that overruns it or dies by a signal fails the
test, its peers are killed, and no later test in this module starts anything on the GPU."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, abi

WORKER = os.path.join(ROOT, "tests", "shoot_ranks_worker.py")
WORKER_TIMEOUT = 240   # seconds per group of workers: a small shoot plus interpreter, torch and gloo start-up
_gpu_stopped = []      # set once a worker timed out or died by a signal


def _run_workers(specs):
    """Starts one worker per spec at once; returns their .npz results.  Kills all of them if one fails."""
    if _gpu_stopped:
        pytest.fail("an earlier worker timed out or died by a signal (%s): nothing more is started on the GPU" % _gpu_stopped[0])
    procs = [subprocess.Popen([sys.executable, WORKER, json.dumps(s)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              env=dict(os.environ, **s.get("env", {}))) for s in specs]
    deadline = time.monotonic() + WORKER_TIMEOUT
    failure = None
    try:
        while failure is None and any(p.poll() is None for p in procs):
            if time.monotonic() > deadline:
                failure = "timed out after %d s" % WORKER_TIMEOUT
                _gpu_stopped.append(failure)
            for i, p in enumerate(procs):
                rc = p.poll()
                if rc is not None and rc != 0 and failure is None:
                    failure = "worker %d exited with %d" % (i, rc)
                    if rc < 0:
                        _gpu_stopped.append(failure)
            time.sleep(0.1)
        for i, p in enumerate(procs):
            if failure is None and p.returncode != 0:
                failure = "worker %d exited with %d" % (i, p.returncode)
                if p.returncode < 0:
                    _gpu_stopped.append(failure)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        logs = [p.communicate()[0].decode(errors="replace")[-3000:] for p in procs]
    if failure is not None:
        pytest.fail("%s\n%s" % (failure, "\n----\n".join(logs)))
    return [dict(np.load(s["out"])) for s in specs]


def _spec(tmp, tag, scene, n_photons, n_tasks, block=4096, over=None, li=None):
    return {"scene": scene, "n_photons": n_photons, "n_tasks": n_tasks, "block": block, "over": over or {}, "li": li,
            "out": str(tmp / ("%s.npz" % tag))}


def _single(tmp, **kw):
    s = dict(_spec(tmp, "single", **kw), mode="single")
    return _run_workers([s])[0]


def _ranks(tmp, n_ranks, env_of_rank=None, **kw):
    """One gloo-connected worker per rank; env_of_rank = {rank: {name: value}} adds to that rank's environment only."""
    _ranks.groups += 1   # a fresh rendezvous file per group of ranks
    store = "file://" + str(tmp / ("gloo_store_%d" % _ranks.groups))
    specs = [dict(_spec(tmp, "rank%d" % r, **kw), mode="gloo", rank=r, world=n_ranks, store=store) for r in range(n_ranks)]
    for r, env in (env_of_rank or {}).items():
        specs[r]["env"] = env
    return _run_workers(specs)


_ranks.groups = 0


def _assert_same_bytes(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n_photons,n_tasks,block,n_ranks_list", [
    ("volumescene_h", 1500, 16, 4096, (1, 2, 3)),       # 16 tasks: divisible by 1 and 2, not by 3
    ("pinkfloyd", 4000, 4, 4096, (2, 3)),               # spectral splits through the prism; 4 tasks over 3 ranks
    ("volumescene_grid16", 1500, 16, 4096, (3,)),       # VolumeGrid: the grid march's LDS plan
    ("volumescene_h", 1500, 2, 4096, (3,)),             # fewer tasks than ranks: rank 2 shoots nothing and still gets the map
    ("pinkfloyd", 4000, 64, 128, (3,)),                 # 128-path blocks
])
def test_sharded_map_is_the_single_rank_map_byte_for_byte(tmp_path, scene, n_photons, n_tasks, block, n_ranks_list):
    ref = _single(tmp_path, scene=scene, n_photons=n_photons, n_tasks=n_tasks, block=block)
    assert ref["status"][0] == 0 and len(ref["p"]) >= n_photons
    for n_ranks in n_ranks_list:
        for r, got in enumerate(_ranks(tmp_path, n_ranks, scene=scene, n_photons=n_photons, n_tasks=n_tasks, block=block)):
            _assert_same_bytes(got, ref, "%s N=%d rank %d" % (scene, n_ranks, r))


@pytest.mark.gpu
def test_sharded_surface_stores_are_the_single_rank_stores(tmp_path):
    kw = dict(scene="pinkfloyd", n_photons=4000, n_tasks=4, over={"keep_surface_photons": 1})
    ref = _single(tmp_path, **kw)
    assert ref["status"][0] == 0
    assert sum(len(ref["s%d_p" % k]) for k in range(3)) > 0
    for r, got in enumerate(_ranks(tmp_path, 3, **kw)):
        _assert_same_bytes(got, ref, "rank %d" % r)


@pytest.mark.gpu
def test_li_from_a_two_rank_map_is_the_single_rank_li(tmp_path):
    kw = dict(scene="volumescene_h", n_photons=1500, n_tasks=16, li="vh")
    ref = _single(tmp_path, **kw)
    assert ref["status"][0] == 0 and len(ref["li"]) > 0 and np.abs(ref["li"]).sum() > 0
    for r, got in enumerate(_ranks(tmp_path, 2, **kw)):
        _assert_same_bytes(got, ref, "rank %d" % r)


@pytest.mark.gpu
def test_ranks_agree_on_the_stall_abort(tmp_path):
    """The stall case of test_a_store_that_stops_growing_ends_the_pass: every rank gives up with the single-rank nshot."""
    kw = dict(scene="volumescene_h", n_photons=150, n_tasks=2, over={"n_indirect_photons": 0, "n_caustic_photons": 4000})
    ref = _single(tmp_path, **kw)
    assert ref["status"][0] == abi.PVOL_E_SHOOT_FAILED
    for r, got in enumerate(_ranks(tmp_path, 2, **kw)):
        assert got["status"][0] == abi.PVOL_E_SHOOT_FAILED, r
        assert len(got["p"]) == 0
        _assert_same_bytes(got, ref, "rank %d" % r)


@pytest.mark.gpu
def test_ranks_agree_on_one_ranks_local_error(tmp_path):
    """Rank 1 alone is told its block pools may hold 2 photons: its first round fails with PVOL_E_LIMIT, and rank 0 returns the
    same code instead of waiting for it in the next exchange."""
    kw = dict(scene="volumescene_h", n_photons=1500, n_tasks=16)
    res = _ranks(tmp_path, 2, env_of_rank={1: {"PVOL_SHOOT_RANK_CAP_MAX": "2"}}, **kw)
    assert [int(g["status"][0]) for g in res] == [abi.PVOL_E_LIMIT, abi.PVOL_E_LIMIT]
    assert all(len(g["p"]) == 0 for g in res)


@pytest.mark.gpu
def test_rccl_branch_gives_the_single_rank_map(tmp_path):
    kw = dict(scene="volumescene_h", n_photons=1500, n_tasks=16)
    ref = _single(tmp_path, **kw)
    got = _run_workers([dict(_spec(tmp_path, "nccl", **kw), mode="nccl")])[0]
    _assert_same_bytes(got, ref, "rccl")


# ---- CPU: the symbol and the argument checks that run before any device work

@pytest.fixture(scope="module")
def pvol():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    return importlib.import_module("cs348b-pbrt_amd.pvol")


def test_preprocess_ranks_is_exported_and_declared(pvol):
    assert hasattr(pvol.lib(), "pvol_preprocess_ranks") and "pvol_preprocess_ranks" in pvol.EXPORTS
    text = open(os.path.join(ROOT, "include", "pvol.h")).read()
    assert "int pvol_preprocess_ranks(pvol_ctx *ctx, uint32_t n_tasks, uint32_t block_paths, uint32_t rank, uint32_t n_ranks," in text
    assert "typedef struct pvol_shoot_comm" in text


def test_preprocess_ranks_rejects_bad_arguments_before_touching_anything(pvol):
    L = pvol.lib()
    fake_ctx = C.create_string_buffer(64)   # never dereferenced: every call below fails its argument checks first
    ctx = C.cast(fake_ctx, C.c_void_p)
    cb = pvol.ALLGATHER_FN(lambda user, send, recv, n: 0)
    gather = pvol.ShootComm(None, cb, None)
    both = pvol.ShootComm(C.c_void_p(1), cb, None)
    neither = pvol.ShootComm()
    nccl_only = pvol.ShootComm(C.c_void_p(1))
    inv = abi.PVOL_E_INVALID
    assert L.pvol_preprocess_ranks(None, 16, 4096, 0, 2, C.byref(gather)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 2, 2, C.byref(gather)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 5, 2, C.byref(nccl_only)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 0, 0, C.byref(gather)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 0, 2, C.byref(both)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 0, 2, C.byref(neither)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4096, 0, 2, None) == inv
    assert L.pvol_preprocess_ranks(ctx, 0, 4096, 0, 2, C.byref(gather)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 0, 0, 2, C.byref(gather)) == inv
    assert L.pvol_preprocess_ranks(ctx, 16, 4097, 0, 2, C.byref(gather)) == inv
