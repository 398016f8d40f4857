#!/usr/bin/env python
"""Times pvol_radiance_gather_batch_device on tests/golden/indirect/room_indirect.pbrt.

The scene is shot with `finalgather` and kept stores, the radiance photons are computed and the gather map is built; the surface
integrator is switched on without an indirect map.  The camera rays come from a numpy pinhole camera and sampler (one ray through the
centre of every pixel sample cell, jittered by a numpy generator), which draw nothing from the streams: rng_skip = 0, one stream per
image row.  Then, three runs each, HIP events around the call:
    gather         pvol_radiance_gather_batch_device (XYZ) on those rays
    radiance       pvol_radiance_batch_device (XYZ) on the same rays: everything but the gather
    final_gather   pvol_final_gather_device on the Lambertian hits of those rays (pvol_probe_hits), with the same sample rows
gather - radiance is what the gather costs inside the walk; final_gather is what its core costs on live queries alone.  Also recorded:
the new kernels' VGPR, SGPR, spill and scratch figures from the code object's metadata.  One JSON line is appended to --out; --pfm
writes the frame (box-filtered XYZ, one value per pixel) as a PFM.

    python tools/time_radiance_gather.py [--xres 320 --yres 240 --spp 4] [--samples 16] [--runs 3] [--out profiles/radiance_gather.jsonl] [--pfm frame.pfm]
"""
import argparse
import importlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENE = os.path.join(ROOT, "tests", "golden", "indirect", "room_indirect.pbrt")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernel_resources(lib_path, prefix="rays_gather_"):
    """The metadata notes of every gfx950 code object bundled in `lib_path`, for the kernels whose name starts with `prefix`."""
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        return {}
    blob = open(lib_path, "rb").read()
    found = {}
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        o = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idl = struct.unpack_from("<QQQ", blob, o)
            ident = blob[o + 24:o + 24 + idl]
            o += 24 + idl
            if b"gfx950" not in ident or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(blob[at + off:at + off + size])
                f.flush()
                notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+\S*?(%s\w+?_kernel)" % prefix, block)   # the name is mangled
                if not name:
                    continue
                def num(key):
                    m = re.search(r"\.%s:\s+(\d+)" % key, block)
                    return int(m.group(1)) if m else None
                found[name.group(1)] = {"vgpr": num("vgpr_count"), "sgpr": num("sgpr_count"), "vgpr_spill": num("vgpr_spill_count"),
                                        "sgpr_spill": num("sgpr_spill_count"), "scratch_bytes": num("private_segment_fixed_size"),
                                        "lds_bytes": num("group_segment_fixed_size")}
        at = blob.find(MAGIC, at + len(MAGIC))
    return found


def camera_rays(abi, scene, xres, yres, spp, rng):
    """A pinhole camera at the scene's camera-to-world with its fov, and a jittered sampler: numpy's, nothing from the streams."""
    c2w = np.asarray(scene["camera.c2w"], np.float64).reshape(4, 4)
    fov = float(np.asarray(scene.get("camera.fov", [70.0])).reshape(-1)[0])
    half = np.tan(np.radians(fov) / 2)
    aspect = xres / yres
    sx, sy = (half * aspect, half) if aspect >= 1 else (half, half / aspect)
    py, px, _ = np.meshgrid(np.arange(yres), np.arange(xres), np.arange(spp), indexing="ij")
    jx, jy = rng.random(px.shape), rng.random(px.shape)
    x = ((px + jx) / xres * 2 - 1) * sx
    y = (1 - (py + jy) / yres * 2) * sy
    d = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3) @ c2w[:3, :3].T
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    n = len(d)
    rays = abi.make_rays(np.tile(c2w[:3, 3].astype(np.float32), (n, 1)), d, np.zeros(n, np.float32), np.full(n, np.inf, np.float32),
                         rng.random(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32))
    streams = abi.make_streams(np.arange(yres), np.full(yres, xres * spp), 0)
    return rays, streams


def timed(torch, fn, runs):
    fn()   # warm-up: grows the scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(round(e0.elapsed_time(e1), 3))
    return ms


def write_pfm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--xres", type=int, default=320)
    ap.add_argument("--yres", type=int, default=240)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--max-dist", type=float, default=0.5)
    ap.add_argument("--indirect-photons", type=int, default=100000)
    ap.add_argument("--volume-photons", type=int, default=100000)
    ap.add_argument("--shoot-tasks", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_gather.jsonl"))
    ap.add_argument("--pfm", default="")
    a = ap.parse_args()

    import torch   # load torch's HIP runtime first, as tests/conftest.py does
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
    abi = pkg.abi
    scene = ps.load(SCENE)
    params = abi.params_from_blob(scene, n_indirect_photons=a.indirect_photons, n_volume_photons=a.volume_photons, keep_surface_photons=1, final_gather=1)
    pv = pvol.PhotonVolume(params)
    try:
        pv.set_scene(abi.SceneHolder(scene))
        pv.preprocess(a.shoot_tasks)
        pv.compute_radiance(50, 0.5)
        n_gather = pv.build_gather_map()
        n_rad = pv.radiance_lo_count()
        pv.set_surface_integrator(50, 0.15, 5)
        rng = np.random.default_rng(1)
        rays, streams = camera_rays(abi, scene, a.xres, a.yres, a.spp, rng)
        n, ns = len(rays), a.samples
        cos_g = pvol.gather_cos_angle(10.0)
        # the Lambertian hits, for pvol_final_gather_device on its own
        f, i = pv.probe_hits(rays, 0)
        h = i[:, 0] == 1
        kd_all = np.asarray(scene["mats.kd"], np.float32).reshape(-1, 30)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, -1).copy()).cuda()
        g = torch.Generator(device="cuda").manual_seed(2)
        d_ub = torch.rand((n, ns, 3), device="cuda", generator=g)
        d_up = torch.rand((n, ns, 3), device="cuda", generator=g)
        hi = torch.from_numpy(np.flatnonzero(h)).cuda()
        q = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in
             (f[h, 2:5], np.concatenate([f[h, 5:8], f[h, 8:11], f[h, 5:8]], 1), -rays["d"][h], kd_all[i[h, 2]], f[h, 1])]
        q_ub, q_up = d_ub[hi].contiguous(), d_up[hi].contiguous()
        nq = int(h.sum())
        q_L = torch.empty((nq, 30), dtype=torch.float32, device="cuda")
        q_draws = torch.empty(nq, dtype=torch.int32, device="cuda")
        d_L = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        d_gd = torch.empty(n, dtype=torch.int32, device="cuda")
        d_L0 = torch.empty((n, 4), dtype=torch.float32, device="cuda")

        def fresh_streams():
            return torch.from_numpy(streams.view(np.uint8).reshape(len(streams), -1).copy()).cuda()
        d_st = fresh_streams()

        def run_gather():
            pv.radiance_gather_batch_device(d_rays.data_ptr(), n, d_st.data_ptr(), len(streams), a.max_dist, ns, cos_g, d_ub.data_ptr(), d_up.data_ptr(),
                                            abi.OUT_XYZ, d_L.data_ptr(), 0, gather_draws=d_gd.data_ptr())

        def run_radiance():
            pv.radiance_batch_device(d_rays.data_ptr(), n, d_st.data_ptr(), len(streams), abi.OUT_XYZ, d_L0.data_ptr(), 0)

        def run_final_gather():
            pv.final_gather_device(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), q[4].data_ptr(), nq, a.max_dist, ns, cos_g,
                                   q_ub.data_ptr(), q_up.data_ptr(), q_L.data_ptr(), q_draws.data_ptr(), 0, 0, 0)
        t_gather = timed(torch, run_gather, a.runs)
        t_radiance = timed(torch, run_radiance, a.runs)
        t_fg = timed(torch, run_final_gather, a.runs)
        pv.check_errors()
        per = abi.RADIANCE_RAY_SCRATCH + abi.radiance_gather_scratch(ns) + abi.RADIANCE_CALLER_SCRATCH
        line = {"scene": "room_indirect.pbrt", "xres": a.xres, "yres": a.yres, "spp": a.spp, "rays": n, "lambertian_hits": nq, "n_samples": ns,
                "max_dist": a.max_dist, "indirect_photons": n_gather, "radiance_photons": n_rad,
                "gather_ms": t_gather, "radiance_ms": t_radiance, "final_gather_ms": t_fg,
                "gather_minus_radiance_ms": round(min(t_gather) - min(t_radiance), 3),
                "walk_overhead_ms": round(min(t_gather) - min(t_radiance) - min(t_fg), 3),
                "slices": -(-n // pvol.lib().pvol_radiance_gather_slice(ns, 0)), "scratch_bytes_per_ray": per,
                "gather_draws": int(d_gd.sum().item()), "lit_rays": int(((d_L[:, :3] - d_L0[:, :3]).abs().amax(dim=1) > 0).sum().item()),
                "kernels": kernel_resources(pvol.LIB_PATH)}
        print(json.dumps(line))
        with open(a.out, "a") as fo:
            fo.write(json.dumps(line) + "\n")
        if a.pfm:
            img = d_L[:, :3].cpu().numpy().reshape(a.yres, a.xres, a.spp, 3).mean(axis=2)
            write_pfm(a.pfm, img)
    finally:
        pv.close()


if __name__ == "__main__":
    main()
