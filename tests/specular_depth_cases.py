"""The reference's captures of the specular recursion at a given "maxspeculardepth" (oracle/gen_golden.py `specular`), the
scenes around them, and the oracle set up for either -- shared by tests/test_specular_depth.py (oracle against the reference's
records) and tests/test_gpu_specular_depth.py (device against both).  Not a test module."""
import os

import numpy as np

from conftest import GOLD, abi, blob, load_photons, load_scene

# capture -> (scene, maxspeculardepth).  All four are the frame of sph_surf: 32 x 32, 4 spp, 16 tasks, tasks 5, 6, 9, 10 (the ball),
# stepsize 0.1, nused 50, photons_sph and caustic_sph.  sphereroom_kr is sphereroom with Kr = 0.25 on the glass: a glass hit
# spawns a reflected and a transmitted ray, so a camera sample owns a tree of segments where sphereroom gives it a chain.
DEPTH_CAPTURES = {
    "sph_surf_d1": ("sphereroom", 1),
    "sph_surf_d2": ("sphereroom", 2),
    "sphkr_surf_d3": ("sphereroom_kr", 3),
    "sphkr_surf_d5": ("sphereroom_kr", 5),
}
PHOTONS = "sph"


def load_caustic(tag=PHOTONS):
    cb = blob.load(os.path.join(GOLD, "caustic_%s.bin" % tag))
    return (cb["p"].reshape(-1, 3), cb["wo"].reshape(-1, 3), cb["alpha"].reshape(-1, 30)), int(cb["n_paths"][0])


def load_depth_capture(name):
    """(scene blob, params, camera, film, sampler, capture) of a capture of DEPTH_CAPTURES: conftest.load_render_case for them."""
    c = blob.load(os.path.join(GOLD, "render_%s.bin" % name))
    s = load_scene(DEPTH_CAPTURES[name][0])
    p = abi.params_from_blob(s, step_size=float(c["params.f"][0]), max_dist=float(c["params.f"][1]), n_used=int(c["params.nused"][0]))
    si = c["sampler.i"]
    sl = c["camera.shutter_lens"]
    cam = abi.make_camera(c["camera.raster_to_camera"], c["camera.camera_to_world"], float(sl[0]), float(sl[1]), float(sl[2]), float(sl[3]))
    fw = c["film.filter_width"]
    film = abi.make_film(int(si[0]), int(si[1]), c["film.filter_table"], float(fw[0]), float(fw[1]))
    smp = abi.make_sampler(int(si[0]), int(si[1]), int(si[2]), int(si[3]), float(fw[0]), float(fw[1]),
                           n1d=tuple(int(v) for v in c["sampler.n1d"]), n2d=tuple(int(v) for v in c["sampler.n2d"]),
                           tau_index=int(si[4]), scatter_index=int(si[5]))
    return s, p, cam, film, smp, c


def capture_depth(c):
    return int(c["surf.maxspeculardepth"][0])


def one_light(s, kr=None, kt=None):
    """The scene blob with its first light only (sphereroom: the spot; the point light is dropped), so that a render takes the COUNT
    pre-pass and the ray-parallel path; kr / kt: a grey value for every glass of the scene."""
    s = dict(s)
    n = len(s["lights.kind"])
    for k in ("lights.kind", "lights.pos", "lights.dir", "lights.l2w", "lights.w2l", "lights.intensity", "lights.cos"):
        s[k] = s[k][:len(s[k]) // n].copy()
    glass = s["mats.kind"] == abi.MATERIAL_GLASS
    assert glass.any()
    for key, v in (("mats.kr", kr), ("mats.kt", kt)):
        if v is not None:
            a = s[key].reshape(-1, 30).copy()
            a[glass] = v
            s[key] = a.ravel()
    return s


def oracle_render(orc, s, p, cam, film, smp, tasks, n_used, max_dist, depth, final_gather=False):
    """The oracle's records of the frame with the surface integrator at `depth` (photons_sph, caustic_sph)."""
    caustic, n_paths = load_caustic()
    o = orc.Oracle(abi.SceneHolder(s), p)
    try:
        o.set_photons(*load_photons(PHOTONS))
        o.set_surface_integrator(n_used, max_dist, final_gather, caustic, n_paths, max_specular_depth=depth)
        r = orc.render_tasks(o, cam, film, smp, tasks)
    finally:
        o.close()
    assert not r["unsupported_hits"]
    for k in ("surf_xyz", "xyzT", "spec_segments", "spec_depth", "spec_both"):
        r[k].setflags(write=False)
    return r


def coverage(r):
    """(samples with a segment, samples per deepest level, samples with a hit that spawned both lobes) from the oracle's counts."""
    seg, lvl, both = r["spec_segments"], r["spec_depth"], r["spec_both"]
    return int((seg > 0).sum()), {int(k): int((lvl == k).sum()) for k in np.unique(lvl)}, int((both > 0).sum())
