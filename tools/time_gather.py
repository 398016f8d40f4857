#!/usr/bin/env python3
"""Times the final gather's sampling half on tests/golden/indirect/room_indirect.pbrt with 100 000 indirect photons
wanted: the host tree build, the map's build as a whole (tree + upload), pvol_gather_photons_device and
pvol_gather_directions_device at 16 samples, for queries on the walls at maxdist 0.15 and 0.5, three runs each.

    python tools/time_gather.py [--out profiles/gather_photons.jsonl] [--queries 4000000] [--runs 3]

Appends one JSON line per maxdist to the file named.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (load torch's HIP runtime first, as tests/conftest.py does)

SCENE = os.path.join(ROOT, "tests", "golden", "indirect", "room_indirect.pbrt")


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_photons.jsonl"))
    ap.add_argument("--queries", type=int, default=4000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--indirect-photons", type=int, default=100000)
    ap.add_argument("--shoot-tasks", type=int, default=2048)
    a = ap.parse_args()
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    abi = pkg.abi
    scene = ps.load(SCENE)
    params = abi.params_from_blob(scene, n_indirect_photons=a.indirect_photons, keep_surface_photons=1)
    pv = pvol.PhotonVolume(params)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.preprocess(a.shoot_tasks)
        ip, iw, _, _ = pv.surface_photons(2)
        n = len(ip)
        tree_s, build_s = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            _, depth = pvol.gather_tree(ip)          # the host tree alone (the test hook)
            tree_s.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pv.build_gather_map()                    # download of the positions, tree, upload
            build_s.append(time.perf_counter() - t0)
        # points on the walls: the photons' own positions, jittered by a few centimetres; frames around random normals
        nq, ns = a.queries, a.samples
        rng = np.random.default_rng(1)
        pick = rng.integers(0, n, nq)
        d_p = torch.from_numpy((ip[pick] + rng.normal(scale=0.03, size=(nq, 3))).astype(np.float32)).cuda()
        g = torch.Generator(device="cuda").manual_seed(2)
        nn = torch.nn.functional.normalize(torch.randn((nq, 3), device="cuda", generator=g), dim=1)
        t = torch.randn((nq, 3), device="cuda", generator=g)
        dpdu = t - (t * nn).sum(1, keepdim=True) * nn
        d_frames = torch.cat([nn, dpdu, nn], dim=1).contiguous()
        d_wo = torch.nn.functional.normalize(torch.randn((nq, 3), device="cuda", generator=g), dim=1).contiguous()
        d_ub = torch.rand((nq, ns, 3), device="cuda", generator=g)
        d_up = torch.rand((nq, ns, 3), device="cuda", generator=g)
        d_index = torch.empty((nq, 50), dtype=torch.int32, device="cuda")
        d_d2 = torch.empty((nq, 50), dtype=torch.float32, device="cuda")
        d_found = torch.empty(nq, dtype=torch.int32, device="cuda")
        d_rounds = torch.empty(nq, dtype=torch.int32, device="cuda")
        d_ob = torch.empty((nq, ns, 8), dtype=torch.float32, device="cuda")
        d_op = torch.empty((nq, ns, 8), dtype=torch.float32, device="cuda")
        cos_g = pvol.gather_cos_angle(10.0)
        for max_dist in (0.15, 0.5):
            look, dirs = [], []
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pv.gather_photons_device(d_p.data_ptr(), nq, max_dist, d_index.data_ptr(), d_d2.data_ptr(), d_found.data_ptr(), d_rounds.data_ptr(), 0)
                torch.cuda.synchronize()
                look.append(time.perf_counter() - t0)
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pv.gather_directions_device(d_p.data_ptr(), d_frames.data_ptr(), d_wo.data_ptr(), nq, max_dist, ns, cos_g, d_ub.data_ptr(),
                                            d_up.data_ptr(), d_ob.data_ptr(), d_op.data_ptr(), 0)
                torch.cuda.synchronize()
                dirs.append(time.perf_counter() - t0)
            line = {"scene": "room_indirect.pbrt", "indirect_photons": n, "tree_depth": depth, "host_tree_s": tree_s, "build_gather_map_s": build_s,
                    "queries": nq, "max_dist": max_dist, "gather_photons_s": look, "Mqueries_per_s": nq / min(look) / 1e6,
                    "found_50": int((d_found == 50).sum().item()), "mean_rounds": float(d_rounds.float().mean().item()),
                    "max_rounds": int(d_rounds.max().item()), "n_samples": ns, "gather_directions_s": dirs,
                    "valid_bsdf": int(d_ob.view(torch.int32)[:, :, 7].sum().item()), "valid_photon": int(d_op.view(torch.int32)[:, :, 7].sum().item())}
            print(json.dumps(line))
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    finally:
        pv.close()


if __name__ == "__main__":
    main()
