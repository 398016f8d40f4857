"""Yardstick of the final gather's sampling half, numpy and plain Python: the reference's kd-tree
(core/kdtree.h:99-147), its Lookup (:157-183), PhotonProcess with libstdc++'s three heap routines transcribed
(core/photonshooter.h:186-203), the doubling loop of integrators/photonmap.cpp:193-199 and the two sampling loops (:208-219,
:250-265) with their weights (:233-243, :280-291).  Every decision is taken on float32 values in the reference's order.  The heap
transcription is held against the real library by tests/heap_probe.cpp (test_gather_photons.py)."""
import numpy as np

f32 = np.float32
K = 50
NO_CHILD = (1 << 29) - 1
NODE_DTYPE = np.dtype([("p", "<f4", 3), ("split_pos", "<f4"), ("split_axis", "<u4"), ("has_left_child", "<u4"), ("right_child", "<u4"),
                       ("index", "<u4")])
SAMPLE_DTYPE = np.dtype([("wi", "<f4", 3), ("weight", "<f4"), ("bsdf_pdf", "<f4"), ("photon_pdf", "<f4"), ("photon_index", "<u4"), ("valid", "<u4")])
M_PI = f32(3.14159265358979323846)
INV_PI = f32(0.31830988618379067154)


# ---- the three heap routines of libstdc++ over a Python list; an element is (d2, id), and tuple comparison is ClosePhoton::operator<
def push_heap_at(h, hole, top, value):   # __push_heap
    parent = (hole - 1) // 2
    while hole > top and h[parent] < value:
        h[hole] = h[parent]
        hole = parent
        parent = (hole - 1) // 2
    h[hole] = value


def adjust_heap(h, hole, length, value):   # __adjust_heap
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if h[child] < h[child - 1]:
            child -= 1
        h[hole] = h[child]
        hole = child
    if length % 2 == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        h[hole] = h[child - 1]
        hole = child - 1
    push_heap_at(h, hole, top, value)


def make_heap(h):
    n = len(h)
    if n < 2:
        return
    parent = (n - 2) // 2
    while True:
        adjust_heap(h, parent, n, h[parent])
        if parent == 0:
            return
        parent -= 1


def pop_heap(h):
    n = len(h)
    if n > 1:
        value = h[n - 1]
        h[n - 1] = h[0]
        adjust_heap(h, 0, n - 1, value)


def push_heap(h):
    n = len(h)
    push_heap_at(h, n - 1, 0, h[n - 1])


def photon_process(seq, k, md2):
    """PhotonProcess::operator() fed the sequence seq of (d2, id), every element subject to kdtree.h:181's `d2 < maxDistSquared`.
    Returns (photons[] as it ends, maxDistSquared)."""
    h = []
    for e in seq:
        if not e[0] < md2:
            continue
        if len(h) < k:
            h.append(e)
            if len(h) == k:
                make_heap(h)
                md2 = h[0][0]
        else:
            pop_heap(h)
            h[k - 1] = e
            push_heap(h)
            md2 = h[0][0]
    return h, md2


# ---- the tree
def build_tree(P):
    """KdTree<Photon>::KdTree over P[n, 3] float32: (nodes in the reference's numbering, depth).  Each range is sorted by
    (coordinate, index), CompareNode's strict total order, and split at its median (start + end) / 2."""
    P = np.ascontiguousarray(P, f32)
    n = len(P)
    nodes = np.zeros(n, NODE_DTYPE)
    next_free = [1]
    depth = [0]

    def build(node, idx, level):
        depth[0] = max(depth[0], level)
        if len(idx) == 1:
            nodes[node] = (P[idx[0]], 0.0, 3, 0, NO_CHILD, idx[0])
            return
        pts = P[idx]
        d = pts.max(axis=0) - pts.min(axis=0)   # float32
        axis = 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)   # BBox::MaximumExtent
        order = idx[np.lexsort((idx, pts[:, axis]))]
        mid = len(idx) // 2
        m = order[mid]
        left, right = order[:mid], order[mid + 1:]
        nodes[node] = (P[m], P[m, axis], axis, 1 if len(left) else 0, NO_CHILD, m)
        if len(left):
            child = next_free[0]
            next_free[0] += 1
            assert child == node + 1
            build(child, left, level + 1)
        if len(right):
            child = next_free[0]
            next_free[0] += 1
            nodes["right_child"][node] = child
            build(child, right, level + 1)

    build(0, np.arange(n, dtype=np.int64), 1)
    return nodes, depth[0]


class Tree:
    """The node arrays as Python lists (a float32 is exact as a Python float, so comparisons decide as fp32 does)."""

    def __init__(self, P):
        self.nodes, self.depth = build_tree(P)
        nd = self.nodes
        self.n = len(nd)
        self.P = np.ascontiguousarray(nd["p"], f32)
        self.split = nd["split_pos"].tolist()
        self.axis = nd["split_axis"].tolist()
        self.left = nd["has_left_child"].tolist()
        self.right = nd["right_child"].tolist()
        self.index = nd["index"].astype(np.int64)
        self.split_f32 = nd["split_pos"].astype(f32)
        self.axis_clamped = np.minimum(nd["split_axis"], 2).astype(np.int64)

    def lookup(self, q, max_dist, k=K):
        """photonmap.cpp:193-199 at the point q: (store indices in heap order, d2, found, rounds); the loop also ends after a
        round whose md2 was +inf (the device's bound)."""
        q = np.asarray(q, f32)
        with np.errstate(all="ignore"):
            dv = self.P - q
            d2 = ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]).tolist()
            pd = q[self.axis_clamped] - self.split_f32
            plane2 = (pd * pd).tolist()
        qa = [float(q[0]), float(q[1]), float(q[2]), 0.0]
        split, axis, left, right, n = self.split, self.axis, self.left, self.right, self.n
        state = {}

        def process(node):
            dd = d2[node]
            if not dd < state["md2"]:
                return
            h = state["h"]
            if len(h) < k:
                h.append((dd, node))
                if len(h) == k:
                    make_heap(h)
                    state["md2"] = h[0][0]
            else:
                pop_heap(h)
                h[k - 1] = (dd, node)
                push_heap(h)
                state["md2"] = h[0][0]

        def visit(node):   # privateLookup
            a = axis[node]
            if a != 3:
                if qa[a] <= split[node]:
                    if left[node]:
                        visit(node + 1)
                    if plane2[node] < state["md2"] and right[node] < n:
                        visit(right[node])
                else:
                    if right[node] < n:
                        visit(right[node])
                    if plane2[node] < state["md2"] and left[node]:
                        visit(node + 1)
            process(node)

        with np.errstate(all="ignore"):
            search = f32(max_dist) * f32(max_dist)
        rounds = 0
        while True:
            round_md2 = float(search)
            state["md2"], state["h"] = round_md2, []
            visit(0)
            with np.errstate(all="ignore"):
                search = search * f32(2.0)
            rounds += 1
            if len(state["h"]) == k or not round_md2 < float("inf"):
                break
        h = state["h"]
        idx = np.zeros(k, np.uint32)
        dd = np.zeros(k, f32)
        for e, (v, node) in enumerate(h):
            idx[e] = self.index[node]
            dd[e] = v
        return idx, dd, len(h), rounds

    def lookup_many(self, Q, max_dist):
        out = [self.lookup(q, max_dist) for q in np.asarray(Q, f32).reshape(-1, 3)]
        return (np.array([o[0] for o in out], np.uint32).reshape(-1, K), np.array([o[1] for o in out], f32).reshape(-1, K),
                np.array([o[2] for o in out], np.uint32), np.array([o[3] for o in out], np.uint32))


# ---- the two sampling loops
def cos_gather_angle(ga):
    """core/photonshooter.cpp:413: cos(Radians(ga)), Radians in fp32, cos in double, stored as a float."""
    rad = f32(f32(M_PI / f32(180.0)) * f32(ga))
    return float(f32(np.cos(np.float64(rad))))


def _cosf(x):
    """cosf as the reference's C library computes it: correctly rounded, here through the double-precision function."""
    return np.cos(np.asarray(x, f32).astype(np.float64)).astype(f32)


def _sinf(x):
    return np.sin(np.asarray(x, f32).astype(np.float64)).astype(f32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _concentric_disk(u1, u2):   # montecarlo.cpp:306-348
    one, two = f32(1), f32(2)
    sx, sy = two * u1 - one, two * u2 - one
    r = np.zeros_like(sx)
    theta = np.zeros_like(sx)
    with np.errstate(all="ignore"):
        a = sx >= -sy
        c1 = a & (sx > sy)
        c2 = a & ~(sx > sy)
        c3 = ~a & (sx <= sy)
        c4 = ~a & ~(sx <= sy)
        r = np.where(c1, sx, np.where(c2, sy, np.where(c3, -sx, -sy))).astype(f32)
        t1 = np.where(sy > 0, sy / r, f32(8.0) + sy / r)
        theta = np.where(c1, t1, np.where(c2, two - sx / r, np.where(c3, f32(4.0) - sy / r, f32(6.0) + sx / r))).astype(f32)
        theta = theta * f32(M_PI / f32(4.0))
        dx, dy = r * _cosf(theta), r * _sinf(theta)
    zero = (sx == 0) & (sy == 0)
    return np.where(zero, f32(0), dx).astype(f32), np.where(zero, f32(0), dy).astype(f32)


def _power_heuristic(n, fp, gp):
    f, g = f32(n) * fp, f32(n) * gp
    with np.errstate(all="ignore"):
        return (f * f) / (f * f + g * g)


def directions(wi_store, index, frames, wo, cos_gather, u_bsdf, u_photon):
    """Both loops for queries whose lookup found 50 photons.  wi_store[n,3]: Photon::wi in the store's order; index[count,50];
    frames[count,9] = nn, dpdu, ng; wo[count,3]; u_*[count,ns,3].  Returns (bsdf records, photon records, margin_bsdf, margin_photon):
    SAMPLE_DTYPE arrays [count, ns], and per sample the smallest distance of a decision (the side test, a `.999f * cos`
    comparison, `pdf == 0` / SameHemisphere) from its threshold, in float64."""
    wi_store, frames, wo = (np.ascontiguousarray(x, f32) for x in (wi_store, frames, wo))
    u_bsdf, u_photon = np.ascontiguousarray(u_bsdf, f32), np.ascontiguousarray(u_photon, f32)
    count, ns = u_bsdf.shape[:2]
    cg = f32(cos_gather)
    thresh = f32(0.999) * cg
    cone_pdf = f32(1.0) / (f32(2.0) * M_PI * (f32(1.0) - cg))
    nn, dpdu, ng = frames[:, None, 0:3], frames[:, 3:6], frames[:, None, 6:9]
    ln = np.sqrt(_dot(dpdu, dpdu))
    inv = f32(1.0) / ln
    sn = (dpdu * inv[:, None]).astype(f32)[:, None, :]
    tn = _cross(nn, sn)
    woW = wo[:, None, :]
    wo_z = _dot(woW, nn)
    wo_ng = _dot(woW, ng)
    dirs = wi_store[index.astype(np.int64)]   # [count, 50, 3]

    def finish(wi, bsdf_pdf, valid0, chosen, photon_loop, margin):
        side = _dot(wi, ng) * wo_ng
        valid = valid0 & (side > 0)
        margin = np.minimum(margin, np.abs(side.astype(np.float64)))
        dots = (dirs[:, None, :, 0] * wi[:, :, None, 0] + dirs[:, None, :, 1] * wi[:, :, None, 1]) + dirs[:, None, :, 2] * wi[:, :, None, 2]
        inside = dots > thresh
        margin = np.minimum(margin, np.abs(dots.astype(np.float64) - np.float64(thresh)).min(axis=2))
        photon_pdf = np.zeros((count, ns), f32)
        for j in range(K):   # the reference adds conePdf photon by photon
            photon_pdf = np.where(inside[:, :, j], photon_pdf + cone_pdf, photon_pdf).astype(f32)
        photon_pdf = photon_pdf / f32(K)
        abs_dot = np.abs(_dot(wi, nn))
        with np.errstate(all="ignore"):
            if photon_loop:
                weight = abs_dot * _power_heuristic(ns, photon_pdf, bsdf_pdf) / photon_pdf
            else:
                weight = abs_dot * _power_heuristic(ns, bsdf_pdf, photon_pdf) / bsdf_pdf
        rec = np.zeros((count, ns), SAMPLE_DTYPE)
        rec["wi"] = np.where(valid[..., None], wi, f32(0))
        rec["weight"] = np.where(valid, weight, f32(0))
        rec["bsdf_pdf"] = np.where(valid, bsdf_pdf, f32(0))
        rec["photon_pdf"] = np.where(valid, photon_pdf, f32(0))
        rec["photon_index"] = chosen
        rec["valid"] = valid
        return rec, margin

    # the BSDF loop
    dx, dy = _concentric_disk(u_bsdf[:, :, 1], u_bsdf[:, :, 2])
    lz = np.sqrt(np.maximum(f32(0), f32(1) - dx * dx - dy * dy)).astype(f32)
    lz = np.where(wo_z < 0, -lz, lz)
    same = wo_z * lz
    pdf = np.where(same > 0, np.abs(lz) * INV_PI, f32(0)).astype(f32)
    wi = (sn * dx[..., None] + tn * dy[..., None]) + nn * lz[..., None]
    rec_b, margin_b = finish(wi.astype(f32), pdf, pdf != 0, np.full((count, ns), 0xffffffff, np.uint32), False, np.abs(same.astype(np.float64)))

    # the photon loop
    num = np.minimum(K - 1, np.floor(u_photon[:, :, 0] * f32(K)).astype(np.int64))
    chosen = np.take_along_axis(index.astype(np.int64), num, axis=1)
    z = wi_store[chosen]
    with np.errstate(all="ignore"):
        use_x = np.abs(z[..., 0]) > np.abs(z[..., 1])
        inv_x = f32(1) / np.sqrt(z[..., 0] * z[..., 0] + z[..., 2] * z[..., 2])
        inv_y = f32(1) / np.sqrt(z[..., 1] * z[..., 1] + z[..., 2] * z[..., 2])
    zero = np.zeros_like(inv_x)
    vx = np.where(use_x[..., None], np.stack([-z[..., 2] * inv_x, zero, z[..., 0] * inv_x], axis=-1),
                  np.stack([zero, z[..., 2] * inv_y, -z[..., 1] * inv_y], axis=-1)).astype(f32)
    vy = _cross(z, vx)
    u1, u2 = u_photon[:, :, 1], u_photon[:, :, 2]
    cost = (f32(1) - u1) * cg + u1 * f32(1)
    sint = np.sqrt(f32(1) - cost * cost)
    phi = u2 * f32(2) * M_PI
    wi = (vx * (_cosf(phi) * sint)[..., None] + vy * (_sinf(phi) * sint)[..., None]) + z * cost[..., None]
    wi = wi.astype(f32)
    wi_z = _dot(wi, nn)
    same = wo_z * wi_z
    bsdf_pdf = np.where(same > 0, np.abs(wi_z) * INV_PI, f32(0)).astype(f32)
    rec_p, margin_p = finish(wi, bsdf_pdf, np.ones((count, ns), bool), chosen.astype(np.uint32), True, np.abs(same.astype(np.float64)))
    for a in (dx, lz, pdf, wi, cost, sint, phi, wi_z):
        assert a.dtype == f32
    return rec_b, rec_p, margin_b, margin_p
