#!/usr/bin/env python3
"""Times the single-process multi-GPU path: pvol_preprocess_group (the sharded shoot over an in-process all-gather) and
pvol_render_frame_group (the task deal, one host thread per context, the film reduce and resolve on context 0's stream).

    python tools/time_frame_group.py --devices 0,1,...,7 [--scene volumescene_h] [--xres 1280 --yres 720 --spp 256]
                                     [--photons 1000000] [--shoot-tasks 16384] [--block 4096] [--frames 1] [--out FILE]

The defaults are C2 (bench.py's flagship frame).  Both calls run twice, on ONE context of the first device (N = 1) and on one
context per --devices entry (N = len(devices)).  Reported per N: the shoot's wall time, each context's pvol_get_exchange_seconds
and pvol_get_preprocess_seconds; the frame's wall time (the call plus a synchronise of context 0's stream, after one warm-up
frame, the best of --frames); each context's pvol_get_phase_ms over one more frame; the efficiency T(1) / (N * T(N)) of the
shoot and of the frame; and the largest difference of the N-context film from the one-context film.

Repeated devices are allowed.  With all contexts on one device (e.g. --devices 0,0 on a one-GPU box) the N contexts share one
GPU: the numbers measure the protocol's overhead, NOT a speed-up, and the tool says so in its output.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime before libpvol.so's, as tests/conftest.py does)


def run(args, devices, pkg, pvol, scene):
    abi = pkg.abi
    bench = importlib.import_module("bench")
    pvs = []
    try:
        for d in devices:
            p = abi.params_from_blob(scene, n_volume_photons=args.photons, device=d)
            pvs.append(pvol.PhotonVolume(p))
        holder = abi.SceneHolder(scene)
        for pv in pvs:
            pv.set_scene(holder)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pvol.preprocess_group(pvs, args.shoot_tasks, args.block)
        shoot_s = time.perf_counter() - t0
        out = {"n_contexts": len(devices), "devices": devices, "shoot_wall_s": shoot_s,
               "exchange_s": [pv.exchange_seconds() for pv in pvs],
               "preprocess_s": [list(pv.preprocess_times()) for pv in pvs], "photons": pvs[0].photon_count()}

        n_tiles = int(bench.frame_tiles(args.xres, args.yres)[4])
        cam = abi.perspective_camera(float(scene["camera.fov"][0]), args.xres, args.yres, scene["camera.c2w"])
        film = abi.make_film(args.xres, args.yres, pvol.gaussian_filter_table())
        smp = abi.make_sampler(args.xres, args.yres, args.spp, n_tiles)
        px = [torch.zeros((args.yres, args.xres, 4), dtype=torch.float32, device="cuda:%d" % d) for d in devices]
        rgb = torch.zeros((args.yres, args.xres, 3), dtype=torch.float32, device="cuda:%d" % devices[0])
        streams = [torch.cuda.Stream(device="cuda:%d" % d) for d in devices]
        for d in sorted(set(devices)):
            torch.cuda.synchronize(d)

        def frame():
            t = time.perf_counter()
            pvol.render_frame_group(pvs, cam, film, smp, [x.data_ptr() for x in px], rgb.data_ptr(), [s.cuda_stream for s in streams])
            streams[0].synchronize()   # covers every context's device
            return time.perf_counter() - t
        frame()   # warm-up: work buffers, the staging buffer, first launches
        times = [frame() for _ in range(max(1, args.frames))]
        for pv in pvs:
            pv.check_errors()
            pv.enable_phase_timing(True)
            pv.phase_ms(reset=True)
        frame()
        out["phase_ms"] = [pv.phase_ms(reset=True) for pv in pvs]
        for pv in pvs:
            pv.enable_phase_timing(False)
            pv.check_errors()
        out["frame_wall_s"] = min(times)
        out["frame_wall_s_all"] = times
        out["n_tasks"] = n_tiles
        return out, px[0].cpu().numpy()
    finally:
        for pv in pvs:
            pv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0,0", help="HIP device ordinals, one context each (repeats allowed)")
    ap.add_argument("--scene", default="volumescene_h")
    ap.add_argument("--xres", type=int, default=1280)
    ap.add_argument("--yres", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--photons", type=int, default=1000000)
    ap.add_argument("--shoot-tasks", type=int, default=16384)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=1, help="timed frames per N after one warm-up; the best is reported")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    devices = [int(x) for x in args.devices.split(",") if x != ""]
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    scene = pkg.blob.load(os.path.join(ROOT, "tests", "golden", "scene_%s.bin" % args.scene))

    one, film1 = run(args, devices[:1], pkg, pvol, scene)
    many, filmN = run(args, devices, pkg, pvol, scene)
    n = len(devices)
    shared = len(set(devices)) < n
    res = {
        "tool": "time_frame_group", "scene": args.scene, "xres": args.xres, "yres": args.yres, "spp": args.spp,
        "photons_asked": args.photons, "shoot_tasks": args.shoot_tasks, "block_paths": args.block,
        "visible_devices": pvol.lib().pvol_device_count(), "n1": one, "nN": many,
        "shoot_efficiency": one["shoot_wall_s"] / (n * many["shoot_wall_s"]),
        "frame_efficiency": one["frame_wall_s"] / (n * many["frame_wall_s"]),
        "film_max_abs_diff_vs_n1": float(np.abs(filmN - film1).max()),
        "film_max_abs_n1": float(np.abs(film1).max()),
        "what": ("%d contexts share %s: protocol overhead, NOT a speed-up" % (n, "one device" if len(set(devices)) == 1 else "devices"))
        if shared else "%d contexts on %d distinct devices" % (n, n),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
