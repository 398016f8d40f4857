#!/usr/bin/env python3
"""Renders a .pbrt scene file through the device pipeline: scene-file front end (cs348b-pbrt_amd/pbrt_scene.py) -> photon shooter
-> SamplerRendererTasks on the device (LD sampler, camera, surface PhotonIntegrator where it applies, PhotonVolumeIntegrator,
image film) -> RGB.

    python tools/render_pbrt.py SCENE.pbrt OUT.pfm [--xres N --yres N --spp N --photons N --shoot-tasks N --no-surface --devices 0,1,...
                                                    --cropwindow X0 X1 Y0 Y1 --volume-integrator single|photonvolume]

The file's own Film / Sampler / integrator parameters are used unless overridden.  A crop window (the file's `"float cropwindow"`
or --cropwindow, fractions of the frame as in the reference's ImageFilm) renders only that part: the image and the PFM have the
window's size, info["window"] says where it lies; the sampler then covers the window's own sample extent, so the tiles and their
random streams are those of the reference's crop render, not a cut-out of the full frame's.  The surface integrator (direct lighting +
caustic estimate on matte surfaces) is switched on when the scene asks for "photonmap" and the device path
covers it (matte and glass surfaces -- the specular recursion included --, a homogeneous or rainbow medium at any nused and
phase function, or no medium; an indirect map only with `finalgather false`, where it adds its own LPhoton estimate); otherwise (a
VolumeGrid or exponential medium, the final gather over an indirect map) Ls = 0 and the image holds the
volume term alone -- the tool says which.  The volume integrator is the file's (`VolumeIntegrator "single"`: single scattering, no
photon map) unless --volume-integrator names one; the shoot is skipped when neither integrator wants a map (single, and no surface
integrator in use).  info["render_s"]: wall seconds of the frame's render_tasks (shoot excluded)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def apply_surface_integrator(pvs, scene, stored_indirect):
    """The scene file's SurfaceIntegrator "photonmap" on every context of `pvs`: nused, maxdist, maxspeculardepth and finalgather as
    the file states them (or the reference's defaults), the maps taken from the last preprocess.  `finalgather false` with indirect
    photons: LPhoton over both stores (set_surface_integrator_maps).  Everything else takes the caustic-only entry point, which
    refuses an indirect map by name -- `finalgather true` with one is the final gather."""
    final_gather = bool(scene["surf.params.i"][2])
    both_maps = not final_gather and stored_indirect > 0
    for q in pvs:
        setter = q.set_surface_integrator_maps if both_maps else q.set_surface_integrator
        setter(int(scene["surf.params.i"][0]), float(scene["surf.params.f"][0]), int(scene["surf.params.i"][1]), final_gather,
               from_preprocess=True)


def render_scene_file(path, xres=None, yres=None, spp=None, photons=None, shoot_tasks=2048, surface=True, log=print, caustic_photons=None,
                      devices=None, cropwindow=None, phases=False, indirect_photons=None, volume_integrator=None):
    """cropwindow: (x0, x1, y0, y1) overrides the file's; None keeps it (the whole frame when the file names none).
    volume_integrator: "single" or "photonvolume" overrides the file's.
    phases: info["phase_ms"] gets the first context's device milliseconds per phase of the frame (tile pre-pass, march + gather,
    surface, film) from HIP events, which serialise the phases a little: not for the frame's own timing.
    devices: None renders on one context (params.device 0); a list of HIP device ordinals (repeats allowed: [0, 0] runs the
    two-context protocol on one GPU) makes one context per entry, shoots with preprocess_group and renders with render_frame_group,
    whose render_s then includes the film reduce and the resolve."""
    import torch
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    abi = pkg.abi
    scene = ps.load(path)
    xres, yres, spp = xres or int(scene["film"][0]), yres or int(scene["film"][1]), spp or int(scene["film"][2])
    spp = 1 << max(0, int(spp - 1).bit_length())   # LDSampler rounds up to a power of two (samplers/lowdiscrepancy.cpp:41-47)
    over = {"keep_surface_photons": 1}
    if photons:
        over["n_volume_photons"] = int(photons)
    if caustic_photons is not None:
        over["n_caustic_photons"] = int(caustic_photons)
    if indirect_photons is not None:
        over["n_indirect_photons"] = int(indirect_photons)
    params = abi.params_from_blob(scene, **over)
    group = devices is not None
    if group:
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("devices: at least one device ordinal")
    pvs = []
    try:
        if group:
            for d in devices:
                pd = abi.Params.from_buffer_copy(params)
                pd.device = d
                pvs.append(pvol.PhotonVolume(pd))
        else:
            pvs.append(pvol.PhotonVolume(params))
        pv = pvs[0]
        holder = abi.SceneHolder(scene)
        for q in pvs:
            q.set_scene(holder)
        vol_int = volume_integrator or scene.get("vol.integrator", "photonvolume")
        for q in pvs:
            q.set_volume_integrator(vol_int)
        want_surface = surface and scene["surf.name"] == "photonmap"
        # "single" reads no volume map; the caustic and indirect maps are the surface integrator's
        if int(scene["lights.kind"].size) and (vol_int != "single" or want_surface):
            if group:
                pvol.preprocess_group(pvs, shoot_tasks)
            else:
                pv.preprocess(shoot_tasks)
        st = pv.shoot_stats()
        log("photon map: %d volume, %d caustic, %d indirect photons from %d paths" % (st["stored_volume"], st["stored_caustic"], st["stored_indirect"],
                                                                                        st["paths"]))
        used_surface = False
        if surface and scene["surf.name"] != "photonmap":
            log('SurfaceIntegrator "%s" has no device path: the image holds the volume term only' % scene["surf.name"])
        if want_surface:
            try:
                apply_surface_integrator(pvs, scene, st["stored_indirect"])
                used_surface = True
            except pvol.PvolError as e:
                log("surface integrator not applied (%s): the image holds the volume term only" % e)
        import bench   # the reference's task count: max(32 x cores, pixels / 256) rounded up to a power of two (samplerrenderer.cpp:206-208)
        n_tiles = int(bench.frame_tiles(xres, yres)[4])
        cam = abi.perspective_camera(float(scene["camera.fov"][0]), xres, yres, scene["camera.c2w"])
        film = abi.make_film(xres, yres, pvol.gaussian_filter_table())
        smp = abi.make_sampler(xres, yres, spp, n_tiles)
        # ImageFilm's window of the crop at the resolution rendered, and the sample extent that goes with it (film/image.cpp:48-51,
        # :157-166); the whole frame keeps the entry points without a window
        crop = ps.crop_window(cropwindow) if cropwindow is not None else scene["film.cropwindow"]
        win = pvol.film_window_from_crop(film, crop)
        if (win.x_pixel_start, win.y_pixel_start, win.x_pixel_count, win.y_pixel_count) == (0, 0, xres, yres):
            win = None
        else:
            abi.set_sample_extent(smp, pvol.film_sample_extent(film, win))
        wx, wy = (win.x_pixel_count, win.y_pixel_count) if win is not None else (xres, yres)
        ids = np.arange(n_tiles, dtype=np.uint32)
        devs = [torch.device("cuda:%d" % d) for d in devices] if group else [torch.device("cuda:0")]
        pxs = [torch.zeros((wy, wx, 4), dtype=torch.float32, device=d) for d in devs]
        px = pxs[0]
        rgb = torch.zeros((wy, wx, 3), dtype=torch.float32, device=devs[0])
        for d in sorted(set(devs), key=str):
            torch.cuda.synchronize(d)

        def frame():   # the group call zeroes its films, reduces them on the first context's device and resolves there
            if group:
                pvol.render_frame_group(pvs, cam, film, smp, [x.data_ptr() for x in pxs], rgb.data_ptr(), window=win)
                torch.cuda.synchronize(devs[0])   # covers every context's device
            else:
                pv.render_tasks(cam, film, smp, ids, px.data_ptr(), window=win)
                torch.cuda.synchronize()
        if phases:
            pv.enable_phase_timing(True)
            pv.phase_ms(reset=True)
        t0 = time.perf_counter()
        try:
            frame()
        except pvol.PvolError as e:
            if not used_surface:
                raise
            log("surface integrator not applied (%s): the image holds the volume term only" % e)
            for q in pvs:
                q.set_surface_integrator(off=True)
            used_surface = False
            px.zero_()
            t0 = time.perf_counter()
            frame()
        render_s = time.perf_counter() - t0
        if not group:
            pv.film_resolve(film, px.data_ptr(), rgb.data_ptr(), window=win)
            torch.cuda.synchronize()
        for q in pvs:
            q.check_errors()
        info = {"xres": xres, "yres": yres, "spp": spp, "surface_integrator": used_surface, "volume_integrator": vol_int, "kernel": pv.march_kernel_name(),
                "photons": int(st["stored_volume"]), "caustic_photons": int(st["stored_caustic"]), "indirect_photons": int(st["stored_indirect"]), "render_s": render_s}
        if group:
            info["devices"] = devices
        if phases:
            info["phase_ms"] = pv.phase_ms()
        if win is not None:   # xPixelStart, yPixelStart, xPixelCount, yPixelCount
            info["window"] = [win.x_pixel_start, win.y_pixel_start, wx, wy]
        return rgb.cpu().numpy(), info
    finally:
        for q in pvs:
            q.close()


def write_pfm(path, rgb):
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(rgb[::-1], dtype="<f4").tobytes())   # PFM stores the bottom row first


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--xres", type=int)
    ap.add_argument("--yres", type=int)
    ap.add_argument("--spp", type=int)
    ap.add_argument("--photons", type=int)
    ap.add_argument("--shoot-tasks", type=int, default=2048)
    ap.add_argument("--no-surface", action="store_true")
    ap.add_argument("--devices", help="comma-separated HIP device ordinals, one context each (repeats allowed, e.g. 0,0); "
                                      "default: one context on device 0")
    ap.add_argument("--cropwindow", type=float, nargs=4, metavar=("X0", "X1", "Y0", "Y1"),
                    help="render this part of the frame only (fractions of the frame, as Film \"float cropwindow\"); overrides the file's")
    ap.add_argument("--volume-integrator", choices=("single", "photonvolume"), help="overrides the file's VolumeIntegrator")
    ap.add_argument("--phases", action="store_true", help="also report device milliseconds per phase of the frame")
    a = ap.parse_args()
    devices = [int(d) for d in a.devices.split(",")] if a.devices else None
    img, info = render_scene_file(a.scene, a.xres, a.yres, a.spp, a.photons, a.shoot_tasks, not a.no_surface, devices=devices, cropwindow=a.cropwindow, phases=a.phases,
                                  volume_integrator=a.volume_integrator)
    write_pfm(a.out, img)
    print(info, "mean rgb", img.mean(axis=(0, 1)))
