#!/usr/bin/env python3
"""Times the surface phase of a frame with an indirect photon map: tests/golden/indirect/room_indirect.pbrt at
320 x 180, 64 spp, 100 000 indirect photons shot once on the device, then three surface integrators over the same stores:

    direct        caustic-only integrator with an empty caustic map: the direct term alone
    indirect_015  both stores (pvol_set_surface_integrator_maps), maxdist 0.15
    indirect_050  the same, maxdist 0.5

    python tools/time_surface_indirect.py [--out profiles/surface_indirect.jsonl] [--runs 3]

One JSON line per run: the render driver's device milliseconds per phase (pvol_get_phase_ms, HIP events on the launch stream) and
the frame's wall seconds.  There is nothing to hold the numbers against but `direct` of the same frame."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENE = os.path.join(ROOT, "tests", "golden", "indirect", "room_indirect.pbrt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_indirect.jsonl"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--xres", type=int, default=320)
    ap.add_argument("--yres", type=int, default=180)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--indirect-photons", type=int, default=100000)
    ap.add_argument("--shoot-tasks", type=int, default=2048)
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    abi = pkg.abi
    scene = ps.load(SCENE)
    params = abi.params_from_blob(scene, n_indirect_photons=a.indirect_photons, keep_surface_photons=1)
    n_used, depth = int(scene["surf.params.i"][0]), int(scene["surf.params.i"][1])
    n_tiles = int(bench.frame_tiles(a.xres, a.yres)[4])
    cam = abi.perspective_camera(float(scene["camera.fov"][0]), a.xres, a.yres, scene["camera.c2w"])
    film = abi.make_film(a.xres, a.yres, pvol.gaussian_filter_table())
    smp = abi.make_sampler(a.xres, a.yres, a.spp, n_tiles)
    ids = np.arange(n_tiles, dtype=np.uint32)
    pv = pvol.PhotonVolume(params)
    lines = []
    try:
        pv.set_scene(abi.SceneHolder(scene))
        t0 = time.perf_counter()
        pv.preprocess(a.shoot_tasks)
        shoot_s = time.perf_counter() - t0
        st = pv.shoot_stats()
        px = torch.zeros((a.yres, a.xres, 4), dtype=torch.float32, device="cuda:0")
        pv.enable_phase_timing(True)
        integrators = [("direct", lambda: pv.set_surface_integrator(n_used, 0.15, depth, False)),
                       ("indirect_015", lambda: pv.set_surface_integrator_maps(n_used, 0.15, depth, False, from_preprocess=True)),
                       ("indirect_050", lambda: pv.set_surface_integrator_maps(n_used, 0.5, depth, False, from_preprocess=True))]
        for name, setup in integrators:
            setup()
            for run in range(a.runs + 1):   # run 0 warms up
                px.zero_()
                torch.cuda.synchronize()
                pv.phase_ms(reset=True)
                t0 = time.perf_counter()
                pv.render_tasks(cam, film, smp, ids, px.data_ptr())
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                pv.check_errors()
                if run == 0:
                    continue
                rec = {"integrator": name, "run": run, "phase_ms": pv.phase_ms(), "render_s": wall, "xres": a.xres, "yres": a.yres, "spp": a.spp,
                       "indirect_photons": int(st["stored_indirect"]), "volume_photons": int(st["stored_volume"]), "shoot_s": shoot_s,
                       "film_mean": float(px[..., :3].mean().item())}
                lines.append(rec)
                print(json.dumps(rec))
    finally:
        pv.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
