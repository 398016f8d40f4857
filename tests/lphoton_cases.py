"""The inputs the tests of pvol_lphoton_batch share (test_lphoton_points.py without a GPU, test_gpu_lphoton_points.py on one): golden
scenes and photon maps, (nused, maxdist) pairs at which the selection really runs, and seeded query points.

With the fixtures' own nused 50 / maxdist 0.5 no query finds 50 photons in the 6 000-photon maps, so the pairs below are used."""
import functools

import numpy as np

from conftest import abi, load_photons, load_scene

import lphoton_ref as ref

F = np.float32
SCENES = [("volumescene_h", "vh"), ("volumescene_hg", "vhg"), ("pinkfloyd", "pf")]
GRID_SCENE = ("volumescene_grid16", "grid16")
PAIRS = [(10, 0.5), (20, 1.0), (50, 1.0), (576, 2.0)]
N_QUERIES = 1000
N_SPECIAL = 12


def params(scene, nused, maxdist):
    return abi.params_from_blob(scene, max_dist=float(maxdist), n_used=int(nused))


def queries(scene, photons, seed, n=N_QUERIES, nused=None, maxdist=None):
    """n points: photon positions (seeded choice) jittered by +-0.05, the last N_SPECIAL of them replaced by points that find few or
    no photons -- just outside the medium's extent at its corners and faces, outside the photons' box, and 10 units away -- and a
    unit direction for each."""
    rng = np.random.default_rng(seed)
    pp = np.asarray(photons[0], F).reshape(-1, 3)
    q = (pp[rng.integers(0, len(pp), n)] + rng.uniform(-0.05, 0.05, (n, 3))).astype(F)
    if nused is not None:
        # The selection must run: where the map is too thin for that many of these points to find nused photons inside maxdist
        # (grid16's 4 001 photons at nused 576: 3 %), the first 40 % of the points are drawn around the 1 % of the photons with the
        # most neighbours inside maxdist instead.  A property of the map alone; the code under test is not asked.
        max2 = F(maxdist) * F(maxdist)
        if ((ref.dist2(pp, q) < max2).sum(axis=1) >= nused).mean() < 0.3:
            crowd = (ref.dist2(pp, pp) < max2).sum(axis=1)
            top = np.argsort(-crowd, kind="stable")[:max(1, len(pp) // 100)]
            m = (2 * n) // 5
            q[:m] = (pp[top[rng.integers(0, len(top), m)]] + rng.uniform(-0.05, 0.05, (m, 3))).astype(F)
    ext = np.asarray(scene["vol.extent"], np.float64)
    v2w = np.asarray(scene["vol.v2w"], np.float64).reshape(4, 4)
    lo, hi = ext[:3], ext[3:]
    mid = 0.5 * (lo + hi)
    vol_pts = [hi + 0.01, lo - 0.01, np.array([hi[0] + 0.3, mid[1], mid[2]]), np.array([mid[0], lo[1] - 0.3, mid[2]]),
               np.array([mid[0], mid[1], hi[2] + 2.0]), hi - 0.01, lo + 0.01, mid]
    special = [v2w[:3, :3] @ v + v2w[:3, 3] for v in vol_pts]
    plo, phi = pp.min(axis=0).astype(np.float64), pp.max(axis=0).astype(np.float64)
    special += [phi + 0.2, plo - 0.2, phi + 10.0, plo - 10.0]
    assert len(special) == N_SPECIAL
    q[n - N_SPECIAL:] = np.asarray(special, F)
    w = rng.normal(size=(n, 3))
    w = (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(F)
    return q, w


@functools.lru_cache(maxsize=None)
def case(scene_name, tag, nused, maxdist):
    """(scene blob, photons, q, w, yardstick dict) -- computed once, shared, never written to."""
    scene = load_scene(scene_name)
    photons = load_photons(tag)
    q, w = queries(scene, photons, seed=1000 + nused, nused=nused, maxdist=maxdist)
    want = ref.lphoton(photons, q, w, nused, maxdist, ref.Medium(scene))
    for v in want.values():
        v.setflags(write=False)
    return scene, photons, q, w, want
