"""Scene::Intersect / Scene::IntersectP ray by ray: the oracle's closest and any hit against the reference's
records of chosen rays -- tests/golden/hits_*.bin, authored per class in oracle/gen_golden.py (`hits`) and answered by the reference's
own Sphere::Intersect / Triangle::Intersect through its BVHAccel on the scenes spherezoo, trizoo and trizoo_h.  The bar is bit
for bit on every field, as in test_scene_units_match_reference.
Two classes are decided by the records themselves and are no pin of the reference's hierarchy: 99, rays on which two leaves return
the very same t (the tree keeps whichever it visits last), and 98, rays on which the hierarchy answers otherwise than a loop over
its own leaves (its box test drops hits on or outside a box face: an origin on an axis-aligned triangle with mint = 0, a sphere `hit`
one ulp outside its box).  For both the fixture also holds the reference's leaves scanned in scene order with its own
GeometricPrimitive::Intersect -- the project's rule (the scan; the later primitive wins, a sphere beats a triangle) spoken by the
reference's shape code -- and the oracle is held to that, bit for bit as well."""
import os

import numpy as np
import pytest

from conftest import GOLD, abi, blob, load_scene

TIE_CLASS, TREE_CLASS = 99, 98
FIELDS = [("IntersectP", 0, 1), ("Intersect", 1, 2), ("t", 2, 3), ("p", 3, 6), ("nn", 6, 9), ("dpdu", 9, 12), ("rayEpsilon", 12, 13)]
# which rays hits_<scene>.bin answers: trizoo_h holds the records of trizoo's rays
HIT_RAYS = {"spherezoo": "spherezoo", "trizoo": "trizoo", "trizoo_h": "trizoo"}


def load_hits(scene_name):
    """(rays, f[n, 14], i[n, 2]) of one hit fixture.  f, i: the records every ray is held to -- the reference's Scene::IntersectP /
    Scene::Intersect, but for the rays of classes 98 and 99 its scan over the scene's leaves (see the module docstring).  rays["tree"]:
    the hierarchy's own (f, i) for every ray, rays["ties"]: how many leaves share the closest t."""
    r = blob.load(os.path.join(GOLD, "hits_%s.bin" % HIT_RAYS[scene_name]))
    c = blob.load(os.path.join(GOLD, "hits_%s.bin" % scene_name))
    tree = (c["ref.f"].reshape(-1, 14), c["ref.i"].reshape(-1, 2))
    f, i = tree[0].copy(), tree[1].copy()
    f[c["scan.idx"]] = c["scan.f"].reshape(-1, 14)
    i[c["scan.idx"]] = c["scan.i"].reshape(-1, 2)
    rays = {"o": r["rays.o"].reshape(-1, 3), "d": r["rays.d"].reshape(-1, 3), "mint": r["rays.mint"], "maxt": r["rays.maxt"],
            "cls": c["rays.cls"], "param": r["rays.param"], "authored": r["rays.authored"], "tree": tree, "ties": c["ref.ties"]}
    return rays, f, i


def oracle_hits(orc, scene_name, rays):
    s = load_scene(scene_name)
    o = orc.Oracle(abi.SceneHolder(s), abi.params_from_blob(s))
    return o.hits(rays["o"], rays["d"], rays["mint"], rays["maxt"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def first_ray(rays, k):
    return "ray %d (class %d): o=%r d=%r mint=%r maxt=%r" % (k, rays["cls"][k], rays["o"][k].tolist(), rays["d"][k].tolist(),
                                                             float(rays["mint"][k]), float(rays["maxt"][k]))


def test_fixture_classes_are_populated_and_flips_are_present():
    """What the fixtures promise: every authored class holds hits and misses, the classes 98 and 99 are exactly the rays whose records
    say so, and the scenes carry the flips."""
    for name, classes in (("spherezoo", list(range(1, 15))), ("trizoo", [12, 13, 14, 20, 21, 22, 23, 25, 26]), ("trizoo_h", [20, 25])):
        rays, f, i = load_hits(name)
        tf, ti = rays["tree"]
        tie = (f[:, 1] > 0) & (rays["ties"] >= 2)
        assert ((rays["cls"] == TIE_CLASS) == tie).all()
        differs = ~tie & ((bits(tf) != bits(f)).any(1) | (ti != i).any(1))
        assert ((rays["cls"] == TREE_CLASS) == differs).all()
        for c in classes:
            m = rays["cls"] == c
            hits = int((f[m, 1] > 0).sum())
            assert hits >= 20 and (c == 10 or m.sum() - hits >= 20), (name, c, hits, int(m.sum()))
    assert load_scene("spherezoo")["spheres.flip"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0]   # reversed; mirrored; both cancel
    t = load_scene("trizoo")
    assert t["tris.flip"].sum() == 4 and len(t["tris.flip"]) == 55 and len(load_scene("trizoo_h")["tris.flip"]) == 71
    # flipped primitives are hit, so `if (flip) nn = -nn` is pinned by the reference
    rays, f, i = load_hits("spherezoo")
    assert ((f[:, 1] > 0) & np.isin(i[:, 0], [-4, -5]) & (rays["cls"] < TREE_CLASS)).sum() >= 100
    rays, f, i = load_hits("trizoo")
    assert ((f[:, 1] > 0) & (i[:, 0] >= 50) & (i[:, 0] <= 53) & (rays["cls"] < TREE_CLASS)).sum() >= 20


def negative_zero(a):
    return (a == 0) & np.signbit(a)


def test_fixture_rays_carry_the_negative_zeros():
    """-0.0 is in the rays as committed, not only as authored: class 8 of spherezoo has y = -0 in origin and in direction on an
    identity sphere (0, 1) and on the half sphere (2, phimax = pi), hit and missed; class 22 of trizoo has axis-aligned directions
    (two zero components: inv = +-inf beside the NaN of 0 * inf) with a -0.0, hit and missed, and one-zero directions with one."""
    rays, f, _ = load_hits("spherezoo")
    hit = f[:, 1] > 0
    for spheres in ((0, 1), (2,)):
        m = (rays["authored"] == 8) & np.isin(rays["param"], spheres)
        for a in (rays["o"], rays["d"]):
            z = m & negative_zero(a[:, 1])
            assert z.sum() >= 8 and (z & hit).any(), (spheres, int(z.sum()))
        assert (m & negative_zero(rays["o"][:, 1]) & negative_zero(rays["d"][:, 1])).sum() >= 4
    rays, f, _ = load_hits("trizoo")
    hit, d = f[:, 1] > 0, rays["d"]
    two = (rays["authored"] == 22) & ((d == 0).sum(1) == 2) & negative_zero(d).any(1)
    assert two.sum() >= 50 and (two & hit & (rays["cls"] == 22)).sum() >= 5 and (two & ~hit).sum() >= 5
    assert ((rays["authored"] == 22) & ((d == 0).sum(1) == 1) & negative_zero(d).any(1)).sum() >= 50


@pytest.mark.parametrize("scene_name", ["spherezoo", "trizoo", "trizoo_h"])
def test_oracle_hits_equal_the_reference_bit_for_bit(orc, scene_name):
    """Every field of every ray.  Classes below 98 are held to the reference's Scene::Intersect / IntersectP; 98 and 99 to the
    reference's own leaves scanned in scene order (the project's rule: the later primitive wins a tie, a sphere beats a triangle)."""
    rays, rf, ri = load_hits(scene_name)
    f, i = oracle_hits(orc, scene_name, rays)
    for name, a, b in FIELDS:
        bad = np.flatnonzero((bits(f[:, a:b]) != bits(rf[:, a:b])).any(1))
        assert len(bad) == 0, "%s differs on %d rays; first: %s oracle %r reference %r" % (
            name, len(bad), first_ray(rays, bad[0]), f[bad[0]].tolist(), rf[bad[0]].tolist())
    hit = rf[:, 1] > 0
    assert (i[hit] == ri[hit]).all()   # which primitive, which material
    tie = rays["cls"] == TIE_CLASS
    print("%s: %d tie rays, the reference's tree kept the rule's primitive on %d; %d rays on which its tree and its leaves differ" %
          (scene_name, tie.sum(), (rays["tree"][1][tie, 0] == ri[tie, 0]).sum(), (rays["cls"] == TREE_CLASS).sum()))


def test_trizoo_records_do_not_depend_on_the_reference_tree():
    """The same rays against the same 55 triangles with and without the far-away filler: another BVHAccel, the same answers."""
    r0, f0, i0 = load_hits("trizoo")
    r1, f1, i1 = load_hits("trizoo_h")
    assert (bits(f0) == bits(f1)).all() and (i0 == i1).all()
    assert (bits(r0["tree"][0]) == bits(r1["tree"][0])).all() and (r0["tree"][1] == r1["tree"][1]).all() and (r0["cls"] == r1["cls"]).all()


# ------------------------------------------------------------------------------------- the hierarchy's slab test, modelled on the CPU
def outside_own_box(s, ref):
    """Rays whose closest hit, by the scan, lies outside the box of the very triangle it is on, grown by the hierarchy's pad (1e-5 of
    the triangles' diagonal).  Triangle::Intersect's fp32 arithmetic does that for a sliver seen from far away: trizoo's sliver, 4
    long and 1e-4 high, is `hit` up to 4 units beside itself from 33 scene diagonals on.  No box test can follow the scan
    there -- the reference's own BVHAccel does not either (class 98) -- so these rays are the stated limit of hierarchy == scan."""
    f, i = ref
    T = s["tris.p"].reshape(-1, 3, 3)
    pad = np.float32(1e-5 * np.linalg.norm((T.reshape(-1, 3).max(0) - T.reshape(-1, 3).min(0)).astype(np.float64)))
    tri = np.where((f[:, 1] > 0) & (i[:, 0] >= 0), i[:, 0], 0)
    out = ((f[:, 3:6] < T[tri].min(1) - pad) | (f[:, 3:6] > T[tri].max(1) + pad)).any(1)
    return out & (f[:, 1] > 0) & (i[:, 0] >= 0)


def far_rays(diagonals, n=6000):
    """n rays from `diagonals` scene diagonals of trizoo out, aimed at and around its 1e-3 triangle (index 54)."""
    w = load_scene("trizoo")["world"].astype(np.float64)
    rng = np.random.default_rng(int(diagonals))
    tgt = np.array([2.5, 2.5, 1.0]) + np.stack([rng.uniform(-2e-4, 1.2e-3, n), rng.uniform(-2e-4, 1.2e-3, n), np.zeros(n)], 1)
    out = rng.normal(size=(n, 3))
    out[:, 2] = np.abs(out[:, 2]) + 0.05
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    o = (tgt + out * diagonals * np.linalg.norm(w[3:] - w[:3])).astype(np.float32)
    d = tgt - o
    return {"o": o, "d": (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), "mint": np.zeros(n, np.float32),
            "maxt": np.full(n, np.inf, np.float32), "cls": np.full(n, 25, np.int32)}


SLAB_WIDEN = np.float32(2.0 ** -21)   # PVOL_BVH_SLAB_WIDEN of csrc/pvol_bvh_dev.h


def slab_passes(lo, hi, o, d, mint, maxt, widen):
    """bvh_slab of csrc/pvol_bvh_dev.h in numpy float32, operation for operation (fmin / fmax drop the NaN of 0 * inf as fminf /
    fmaxf do); widen = 0 is the test as it stood before the interval was widened."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.float32(1) / d
        a, b = (lo - o) * inv, (hi - o) * inv
        near, far = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2])
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        if widen:
            tn = tn * (np.float32(1) - np.copysign(widen, tn))
            tf = tf * (np.float32(1) + np.copysign(widen, tf))
        else:
            tn, tf = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], mint)), np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], maxt))
        return np.fmax(tn, mint) <= np.fmin(tf, maxt)


@pytest.mark.parametrize("diagonals", [300.0, 600.0, 3000.0])
def test_slab_model_reaches_every_triangle_the_scan_hits(orc, diagonals):
    """Why bvh_slab widens its interval.  The model: the traversal reaches a triangle iff the triangle's own padded box
    passes the slab test with the ray clipped to [mint, t of the scan's hit] -- the strictest clip the traversal can apply, since its
    running `best` never falls below the scan's t; the ancestors' boxes contain the leaf's and fmin / fmax are monotone, so they
    pass when the leaf's does.  The pad is a fixed length, the rounding of (lo - o) * inv grows with |o|: at 600 and 3 000 diagonals
    the unwidened test leaves out boxes whose triangle the scan hits; the widened one leaves out none at any of the three."""
    s = load_scene("trizoo_h")
    rays = far_rays(diagonals)
    f, i = orc.Oracle(abi.SceneHolder(s), abi.params_from_blob(s)).hits(rays["o"], rays["d"], rays["mint"], rays["maxt"])
    hit = (f[:, 1] > 0) & (i[:, 0] >= 0) & ~outside_own_box(s, (f, i))
    assert hit.sum() >= 1000
    T = s["tris.p"].reshape(-1, 3, 3).astype(np.float32)
    pad = np.float32(1e-5 * np.linalg.norm((T.reshape(-1, 3).max(0) - T.reshape(-1, 3).min(0)).astype(np.float64)))
    tri = i[hit, 0]
    lo, hi = T[tri].min(1) - pad, T[tri].max(1) + pad
    args = (lo, hi, rays["o"][hit], rays["d"][hit], rays["mint"][hit], f[hit, 2])
    old, new = slab_passes(*args, widen=0), slab_passes(*args, widen=SLAB_WIDEN)
    print("%g diagonals: %d hits of the scan; boxes left out: %d unwidened, %d widened" % (diagonals, hit.sum(), (~old).sum(), (~new).sum()))
    assert new.all()
    assert diagonals < 600 or (~old).sum() >= 10
