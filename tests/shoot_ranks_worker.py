"""One process of tests/test_gpu_shoot_ranks.py (not collected by pytest): a single-rank shoot, one rank of a gloo-connected sharded
shoot, or a one-rank sharded shoot over an RCCL communicator.  Each runs in a fresh process started by the test, so no process
forks after the GPU is initialised.  Writes what it computed to an .npz.

    python tests/shoot_ranks_worker.py '<json spec>'
spec: mode ("single" | "gloo" | "nccl"), scene, n_photons, n_tasks, block, over (extra pvol_params), out (.npz path),
li (golden Li case to run on the map, or null), and for "gloo" rank, world, store (file:// rendezvous).
"""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rccl_comm():
    """A one-rank ncclComm_t from the librccl.so.1 loaded RTLD_GLOBAL here, the copy libpvol.so then binds to."""
    class UniqueId(C.Structure):   # ncclUniqueId, passed by value to ncclCommInitRank
        _fields_ = [("internal", C.c_char * 128)]
    try:
        rccl = C.CDLL("librccl.so.1", mode=C.RTLD_GLOBAL)
    except OSError:
        rccl = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "librccl.so.1"), mode=C.RTLD_GLOBAL)
    uid = UniqueId()
    rccl.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    return rccl, comm


def main():
    spec = json.loads(sys.argv[1])
    mode = spec["mode"]
    if mode == "gloo":
        import torch  # noqa: F401  (torch's HIP runtime before libpvol.so's, as tests/conftest.py does)
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=spec["store"], rank=spec["rank"], world_size=spec["world"])
    if mode == "nccl":
        rccl, comm = _rccl_comm()
    import numpy as np
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    abi, blob = pkg.abi, pkg.blob
    gold = os.path.join(ROOT, "tests", "golden")
    s = blob.load(os.path.join(gold, "scene_%s.bin" % spec["scene"]))
    over = dict(spec.get("over") or {})
    case = None
    if spec.get("li"):
        case = blob.load(os.path.join(gold, "li_%s.bin" % spec["li"]))
        over.update(step_size=float(case["params.f"][0]), max_dist=float(case["params.f"][1]), n_used=int(case["params.nused"][0]))
    p = abi.params_from_blob(s, n_volume_photons=spec["n_photons"], **over)
    holder = abi.SceneHolder(s)
    pv = pvol.PhotonVolume(p)
    pv.set_scene(holder)
    status = 0
    try:
        if mode == "single":
            pv.preprocess(spec["n_tasks"], spec["block"])
        elif mode == "gloo":
            pv.preprocess_ranks(spec["n_tasks"], spec["rank"], spec["world"], allgather=pvol.gloo_allgather(), block_paths=spec["block"])
        else:
            pv.preprocess_ranks(spec["n_tasks"], 0, 1, nccl_comm=comm.value, block_paths=spec["block"])
    except pvol.PvolError as e:
        status = e.status
    res = {"status": np.array([status], np.int64), "stats": np.array([pv.shoot_stats()[k] for k in pvol.SHOOT_STAT_NAMES], np.uint64)}
    res["p"], res["wi"], res["alpha"] = pv.download_photons()
    if p.keep_surface_photons:
        for kind in range(3):
            sp, wo, a, npaths = pv.surface_photons(kind)
            res["s%d_p" % kind], res["s%d_wo" % kind], res["s%d_alpha" % kind] = sp, wo, a
            res["s%d_paths" % kind] = np.array([npaths], np.int64)
        for i, a in enumerate(pv.radiance_photons()):
            res["rad%d" % i] = a
    if case is not None and status == 0:
        rays = abi.make_rays(case["rays.o"].reshape(-1, 3), case["rays.d"].reshape(-1, 3), case["rays.mint"], case["rays.maxt"],
                             case["rays.u"], case["rays.time"], case["rays.skip"])
        streams = abi.make_streams(case["streams.seed"], case["streams.n"], case["streams.start"])
        res["li"], res["li_draws"] = pv.li(rays, streams)
    pv.close()
    if mode == "gloo":
        dist.destroy_process_group()
    if mode == "nccl":
        rccl.ncclCommDestroy(comm)
    np.savez(spec["out"], **res)


if __name__ == "__main__":
    main()
