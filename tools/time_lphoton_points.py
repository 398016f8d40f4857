#!/usr/bin/env python
"""Times pvol_lphoton_batch_device on the C2 map: volumescene, 1 M volume photons wanted, the scene's own nused and
maxdist.  A regular lattice of points over the medium, given in x-fastest order and shuffled, each with the cell sort on and off
(PVOL_LPHOTON_NO_SORT is read when a context is made, so there are two contexts over the same downloaded map).  Three runs each,
HIP events around the call; one JSON line per configuration is appended to --out.

    python tools/time_lphoton_points.py [--points 1000000] [--photons 1000000] [--runs 3] [--only lattice-sorted,...] [--out profiles/lphoton_points.jsonl]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = ["lattice-sorted", "lattice-unsorted", "shuffled-sorted", "shuffled-unsorted"]


def lattice(scene, n_points):
    """About n_points points on a regular lattice over the medium's extent (cell centres), x fastest, world space."""
    ext = np.asarray(scene["vol.extent"], np.float64)
    v2w = np.asarray(scene["vol.v2w"], np.float64).reshape(4, 4)
    size = ext[3:] - ext[:3]
    h = (size.prod() / n_points) ** (1.0 / 3.0)
    dims = np.maximum(1, np.round(size / h).astype(int))
    ax = [ext[i] + (np.arange(dims[i]) + 0.5) * size[i] / dims[i] for i in range(3)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    p = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
    return (p @ v2w[:3, :3].T + v2w[:3, 3]).astype(np.float32), [int(d) for d in dims]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--photons", type=int, default=1000000)
    ap.add_argument("--shoot-tasks", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list out of " + ", ".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lphoton_points.jsonl"))
    args = ap.parse_args()
    only = [c for c in args.only.split(",") if c] or CONFIGS
    for c in only:
        if c not in CONFIGS:
            ap.error("unknown configuration %r" % c)

    import torch
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    abi, blob = pkg.abi, pkg.blob
    scene = blob.load(os.path.join(ROOT, "tests", "golden", "scene_volumescene_h.bin"))
    params = abi.params_from_blob(scene, n_volume_photons=args.photons)
    holder = abi.SceneHolder(scene)

    def context(no_sort):
        old = os.environ.get("PVOL_LPHOTON_NO_SORT")
        os.environ["PVOL_LPHOTON_NO_SORT"] = "1" if no_sort else "0"
        try:
            pv = pvol.PhotonVolume(params)
        finally:
            os.environ.pop("PVOL_LPHOTON_NO_SORT", None) if old is None else os.environ.__setitem__("PVOL_LPHOTON_NO_SORT", old)
        pv.set_scene(holder)
        return pv

    ctx = {False: context(False)}
    ctx[False].preprocess(args.shoot_tasks)
    shoot_s = ctx[False].preprocess_times()[0]
    n_photons = ctx[False].photon_count()
    if any(c.endswith("-unsorted") for c in only):
        ctx[True] = context(True)
        ctx[True].upload_photons(*ctx[False].download_photons())
    pts, dims = lattice(scene, args.points)
    n = len(pts)
    perm = np.random.default_rng(348).permutation(n)
    d_pts = {"lattice": torch.from_numpy(pts).cuda(), "shuffled": torch.from_numpy(pts[perm]).cuda()}
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    d_nf = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    first = None
    with open(args.out, "a") as f:
        for name in only:
            order, srt = name.split("-")
            pv = ctx[srt == "unsorted"]
            dp = d_pts[order]

            def call():
                pv.lphoton_batch_device(dp.data_ptr(), 0, n, abi.OUT_XYZ, d_out.data_ptr(), d_nf.data_ptr(), 0, stream)
            call()   # warm-up: grows the scratch
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            pv.check_errors()
            nf = d_nf.cpu().numpy()
            xyz = d_out.cpu().numpy()
            if order == "shuffled":   # back to lattice order: every configuration must give the same bytes
                inv = np.argsort(perm)
                nf, xyz = nf[inv], xyz[inv]
            if first is None:
                first = (nf.copy(), xyz.copy())
            same = bool((nf == first[0]).all() and (xyz.view(np.uint32) == first[1].view(np.uint32)).all())
            rec = {"config": name, "points": n, "lattice": dims, "photons": n_photons, "n_used": int(params.n_used), "max_dist": float(params.max_dist),
                   "ms": [round(m, 3) for m in ms], "ms_mean": round(float(np.mean(ms)), 3),
                   "lookups_per_s": round(n / (float(np.mean(ms)) * 1e-3), 1), "lookups_per_s_best": round(n / (min(ms) * 1e-3), 1),
                   "share_full_k": round(float((nf == params.n_used).mean()), 4), "share_below_10": round(float((nf < 10).mean()), 4),
                   "same_bytes_as_first_config": same, "shoot_s": round(shoot_s, 3)}
            line = json.dumps(rec)
            print(line)
            f.write(line + "\n")
            f.flush()
    for pv in ctx.values():
        pv.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
