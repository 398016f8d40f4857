#!/usr/bin/env python3
"""Times pvol_compute_radiance and a pvol_radiance_lookup_device batch after a device shoot of
tests/golden/scenes/volumescene_equiv.pbrt with `finalgather` on and indirect photons wanted.

    python tools/time_radiance.py [volume_photons] [indirect_photons] [n_tasks] [queries] [out.jsonl]

Appends one JSON line to profiles/radiance_photons.jsonl (or the file named).
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (load torch's HIP runtime first, as tests/conftest.py does)


def main():
    import numpy as np
    n_volume = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    n_indirect = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    n_tasks = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    n_query = int(sys.argv[4]) if len(sys.argv) > 4 else 4000000
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "radiance_photons.jsonl")
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    abi = pkg.abi
    scene = ps.load(os.path.join(ROOT, "tests", "golden", "scenes", "volumescene_equiv.pbrt"))
    p = abi.params_from_blob(scene, n_volume_photons=n_volume, n_indirect_photons=n_indirect, n_caustic_photons=0, final_gather=1,
                             keep_surface_photons=1)
    pv = pvol.PhotonVolume(p)
    pv.set_scene(abi.SceneHolder(scene))
    pv.preprocess(n_tasks)
    shoot_s, build_s = pv.preprocess_times()
    stores = [len(pv.surface_photons(kind)[0]) for kind in range(3)]
    n_lookup, max_dist = 50, 0.1   # CreatePhotonMapSurfaceIntegrator's defaults (photonmap.cpp:340,345)
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pv.compute_radiance(n_lookup, max_dist)
        times.append(time.perf_counter() - t0)
    rp_p, rp_n, lo = pv.radiance_lo()
    n_rp = len(rp_p)
    # points on the walls: the radiance photons' own positions, jittered by a few centimetres, with their normals
    rng = np.random.default_rng(1)
    pick = rng.integers(0, max(n_rp, 1), n_query)
    q_p = torch.from_numpy((rp_p[pick] + rng.normal(scale=0.03, size=(n_query, 3))).astype(np.float32)).cuda()
    q_n = torch.from_numpy(rp_n[pick]).cuda()
    d_lo = torch.empty((n_query, 30), dtype=torch.float32, device="cuda")
    d_found = torch.empty(n_query, dtype=torch.int32, device="cuda")
    look = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pv.radiance_lookup_device(q_p.data_ptr(), q_n.data_ptr(), n_query, d_lo.data_ptr(), d_found.data_ptr(), 0)
        torch.cuda.synchronize()
        look.append(time.perf_counter() - t0)
    line = {"scene": "volumescene_equiv.pbrt", "n_tasks": n_tasks, "volume_photons": pv.photon_count(), "caustic_direct_indirect": stores,
            "radiance_photons": n_rp, "shoot_s": shoot_s, "grid_build_s": build_s, "n_lookup": n_lookup, "max_dist": max_dist,
            "compute_radiance_s": times, "nonzero_lo_rows": int((lo.sum(axis=1) > 0).sum()), "queries": n_query, "lookup_s": look,
            "found": int(d_found.sum().item()), "Mqueries_per_s": n_query / min(look) / 1e6}
    print(json.dumps(line))
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")
    pv.close()


if __name__ == "__main__":
    main()
