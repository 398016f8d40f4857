#!/usr/bin/env python3
"""Times the final gather's tracing half on tests/golden/indirect/room_indirect.pbrt with 100 000 indirect photons
wanted: pvol_final_gather_device at 16 samples for 1 M queries on the walls (the hits of rays from the camera), at maxdist 0.15
and 0.5, three runs each, and beside it pvol_gather_directions_device on the same queries in the same process, so that the cost of
tracing and summing shows as the difference.

    python tools/time_final_gather.py [--out profiles/final_gather.jsonl] [--queries 1000000] [--runs 3]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "final_gather.jsonl"))
    ap.add_argument("--queries", type=int, default=1000000)
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
    params = abi.params_from_blob(scene, n_indirect_photons=a.indirect_photons, keep_surface_photons=1, final_gather=1)
    pv = pvol.PhotonVolume(params)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.preprocess(a.shoot_tasks)
        t0 = time.perf_counter()
        pv.compute_radiance(50, 0.5)
        radiance_s = time.perf_counter() - t0
        n = pv.build_gather_map()
        n_rad = pv.radiance_lo_count()
        # queries on the walls: the hits of rays from the camera, with the hit's own frame, wo back along the ray
        nq, ns = a.queries, a.samples
        rng = np.random.default_rng(1)
        Q, frames, wo, eps = [], [], [], []
        c2w = np.asarray(scene["camera.c2w"], np.float64).reshape(4, 4)
        while sum(len(x) for x in Q) < nq:
            m = nq // 2 + 1024
            d = c2w[:3, 2] + 0.8 * rng.uniform(-1, 1, (m, 3))
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
            rays = abi.make_rays(np.tile(c2w[:3, 3].astype(np.float32), (m, 1)), d, np.zeros(m, np.float32), np.full(m, np.inf, np.float32),
                                 np.zeros(m, np.float32))
            f, i = pv.probe_hits(rays, 0)
            h = i[:, 0] == 1
            Q.append(f[h, 2:5]); frames.append(np.concatenate([f[h, 5:8], f[h, 8:11], f[h, 5:8]], 1)); wo.append(-d[h]); eps.append(f[h, 1])
        Q, frames, wo, eps = (np.ascontiguousarray(np.concatenate(x)[:nq], np.float32) for x in (Q, frames, wo, eps))
        kd = np.tile(np.asarray(scene["mats.kd"], np.float32).reshape(-1, 30)[0], (nq, 1))
        d_p, d_frames, d_wo, d_kd, d_eps = (torch.from_numpy(x).cuda() for x in (Q, frames, wo, kd, eps))
        g = torch.Generator(device="cuda").manual_seed(2)
        d_ub = torch.rand((nq, ns, 3), device="cuda", generator=g)
        d_up = torch.rand((nq, ns, 3), device="cuda", generator=g)
        d_ob = torch.empty((nq, ns, 8), dtype=torch.float32, device="cuda")
        d_op = torch.empty((nq, ns, 8), dtype=torch.float32, device="cuda")
        d_L = torch.empty((nq, 30), dtype=torch.float32, device="cuda")
        d_draws = torch.empty(nq, dtype=torch.int32, device="cuda")
        cos_g = pvol.gather_cos_angle(10.0)
        for max_dist in (0.15, 0.5):
            dirs, full = [], []
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pv.gather_directions_device(d_p.data_ptr(), d_frames.data_ptr(), d_wo.data_ptr(), nq, max_dist, ns, cos_g, d_ub.data_ptr(),
                                            d_up.data_ptr(), d_ob.data_ptr(), d_op.data_ptr(), 0)
                torch.cuda.synchronize()
                dirs.append(time.perf_counter() - t0)
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pv.final_gather_device(d_p.data_ptr(), d_frames.data_ptr(), d_wo.data_ptr(), d_kd.data_ptr(), d_eps.data_ptr(), nq, max_dist, ns, cos_g,
                                       d_ub.data_ptr(), d_up.data_ptr(), d_L.data_ptr(), d_draws.data_ptr(), 0, 0, 0)
                torch.cuda.synchronize()
                full.append(time.perf_counter() - t0)
            valid = int(d_ob.view(torch.int32)[:, :, 7].sum().item()) + int(d_op.view(torch.int32)[:, :, 7].sum().item())
            line = {"scene": "room_indirect.pbrt", "indirect_photons": n, "radiance_photons": n_rad, "compute_radiance_s": radiance_s, "queries": nq,
                    "n_samples": ns, "max_dist": max_dist, "gather_directions_s": dirs, "final_gather_s": full,
                    "trace_and_sum_s": min(full) - min(dirs), "valid_rays": valid, "rays_that_hit": int(d_draws.sum().item()),
                    "Mrays_per_s": valid / min(full) / 1e6, "slices": -(-nq // pvol.lib().pvol_final_gather_slice(ns, 0)),
                    "lit_queries": int((d_L.abs().amax(dim=1) > 0).sum().item())}
            print(json.dumps(line))
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    finally:
        pv.close()


if __name__ == "__main__":
    main()
