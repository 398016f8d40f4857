#!/usr/bin/env python3
"""Frame time of the surface integrator on the wave-per-ray path: projectScene/volumescene_png.pbrt
(rainbow medium, li_par_kernel) and projectScene/darkside.pbrt (nused 300, spot light through a glass prism, li_par_kernel),
each rendered with and without the surface term through tools/render_pbrt.py.  One JSON line per render; `render_s` is the
wall time of render_tasks (shoot excluded), the best of --repeat renders.

    python tools/time_surface_media.py [--repeat 2] [--scenes volumescene_png,darkside] [--darkside-size 160x100]
                                       [--darkside-spp 4] [--darkside-photons N] [--darkside-caustic N]
                                       [--darkside-shoot-tasks N]

Progress (photon map, per-render times) goes to stderr."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "projectScene")


def _render_pbrt():
    spec = importlib.util.spec_from_file_location("render_pbrt", os.path.join(ROOT, "tools", "render_pbrt.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    return rp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--volumescene-size", default="1280x720")
    ap.add_argument("--darkside-size", default="160x100")
    ap.add_argument("--darkside-spp", type=int, default=4)
    ap.add_argument("--darkside-caustic", type=int, default=5000, help="caustic photons (the file asks for 250 000)")
    ap.add_argument("--darkside-photons", type=int, default=20000, help="volume photons (the file asks for 2 500 000)")
    ap.add_argument("--darkside-shoot-tasks", type=int, default=64, help="virtual shoot tasks: one round is this x 4096 paths, and darkside's\n"
                    "spot light stores ~3 volume photons per path, so 2048 tasks overshoot any request by ~24 M photons")
    ap.add_argument("--scenes", default="volumescene_png,darkside")
    a = ap.parse_args()
    rp = _render_pbrt()
    t00 = time.perf_counter()

    def log(*x):
        print("[%7.1f s]" % (time.perf_counter() - t00), *x, file=sys.stderr, flush=True)
    rp.render_scene_file(os.path.join(SCENES, "volumescene_png.pbrt"), xres=32, yres=32, log=lambda *x: None)   # code objects loaded once
    vx, vy = (int(v) for v in a.volumescene_size.split("x"))
    dx, dy = (int(v) for v in a.darkside_size.split("x"))
    jobs = [("volumescene_png", dict(xres=vx, yres=vy)),
            ("darkside", dict(xres=dx, yres=dy, spp=a.darkside_spp, caustic_photons=a.darkside_caustic, photons=a.darkside_photons,
                              shoot_tasks=a.darkside_shoot_tasks))]
    for name, kw in jobs:
        if name not in a.scenes.split(","):
            continue
        for surface in (True, False):
            best, info = None, None
            for _ in range(max(1, a.repeat)):
                log(name, "surface" if surface else "no surface", kw)
                img, info = rp.render_scene_file(os.path.join(SCENES, name + ".pbrt"), surface=surface, log=log, **kw)
                log("render_tasks %.3f s" % info["render_s"])
                best = info["render_s"] if best is None else min(best, info["render_s"])
            n = info["xres"] * info["yres"] * info["spp"]
            print(json.dumps({"scene": name, "xres": info["xres"], "yres": info["yres"], "spp": info["spp"], "surface": info["surface_integrator"],
                              "kernel": info["kernel"], "photons": info["photons"], "caustic_photons": info["caustic_photons"],
                              "render_s": round(best, 4), "msamples_per_s": round(n / best / 1e6, 3), "mean_rgb": [round(float(v), 5) for v in img.mean(axis=(0, 1))]}),
                  flush=True)


if __name__ == "__main__":
    main()
