"""numpy restatement of ComputeRadianceTask::Run (core/photonshooter.cpp:359-395), EPhoton (:17-35), PhotonProcess
(core/photonshooter.h:186-203) and RadiancePhotonProcess (:63-78), shared by test_radiance_photons.py and
test_gpu_radiance_photons.py.  Decisions are made in float32 in the reference's order -- d2 = dx*dx + dy*dy + dz*dz, the strict
`d2 < md2` of core/kdtree.h:180, the sign of the dot product -- and sums run in float64."""
import heapq

import numpy as np

F32 = np.float32
PI32 = F32(3.14159265358979323846)       # core/pbrt.h:191
INV_PI32 = F32(0.31830988618379067154)   # core/pbrt.h:192


def d2_f32(P, q):
    """DistanceSquared(photon.p, q) for every row of P, in float32."""
    P = np.asarray(P, F32).reshape(-1, 3)
    q = np.asarray(q, F32)
    dx, dy, dz = P[:, 0] - q[0], P[:, 1] - q[1], P[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def dot_f32(n, W):
    """Dot(n, w) for every row of W, in float32."""
    W = np.asarray(W, F32).reshape(-1, 3)
    n = np.asarray(n, F32)
    return (n[0] * W[:, 0] + n[1] * W[:, 1]) + n[2] * W[:, 2]


def knn(d2, k, max_dist):
    """The photons PhotonProcess ends with and the final md2: (indices, md2, tie).  tie: an exact float32 tie at the k-th place."""
    md2max = F32(max_dist) * F32(max_dist)
    inside = np.flatnonzero(d2 < md2max)
    if len(inside) < k:
        return inside, md2max, False
    order = inside[np.argsort(d2[inside], kind="stable")]
    tie = len(order) > k and d2[order[k]] == d2[order[k - 1]]
    return order[:k], d2[order[k - 1]], bool(tie)


def photon_process(d2, visit_order, k, max_dist):
    """PhotonProcess transcribed literally over the photons in `visit_order`: an unordered array until the k-th photon arrives,
    then std::make_heap and, for every later photon inside md2, pop_heap / overwrite the last / push_heap.  Returns (set of
    indices, md2)."""
    md2 = F32(max_dist) * F32(max_dist)
    photons, heap = [], None   # heap: a max-heap of (distanceSquared, photon) as ClosePhoton::operator< orders them
    for i in visit_order:
        dist2 = d2[i]
        if not dist2 < md2:
            continue
        if heap is None:
            photons.append((dist2, int(i)))
            if len(photons) == k:
                heap = [(-a, -b) for a, b in photons]
                heapq.heapify(heap)
                md2 = F32(-heap[0][0])
        else:
            heapq.heappop(heap)
            heapq.heappush(heap, (-dist2, -int(i)))
            md2 = F32(-heap[0][0])
    kept = photons if heap is None else [(-a, -b) for a, b in heap]
    return {b for _, b in kept}, md2


def ephoton(P, W, A, n_paths, q, n, k, max_dist):
    """EPhoton for the point q and both sides of n: (E(n)[30], E(-n)[30], tie), float64."""
    if P is None or len(P) == 0:
        return np.zeros(30), np.zeros(30), False
    idx, md2, tie = knn(d2_f32(P, q), k, max_dist)
    if len(idx) == 0:
        return np.zeros(30), np.zeros(30), False
    dots = dot_f32(n, np.asarray(W, F32).reshape(-1, 3)[idx])
    rows = np.asarray(A, np.float64).reshape(-1, 30)[idx]
    denom = float((F32(int(n_paths)) * md2) * PI32)
    return rows[dots > 0].sum(axis=0) / denom, rows[dots < 0].sum(axis=0) / denom, tie


def compute_lo(maps, rp_p, rp_n, rho_r, rho_t, k, max_dist):
    """maps: [caustic, direct, indirect], each None or (p, wi, alpha, n_paths).  Returns (Lo[n, 30] float64, ties[n, 3] bool in
    the same map order): Lo = INV_PI rho_r (Ed + Ei + Ec)(n) + INV_PI rho_t (Ed + Ei + Ec)(-n), a side skipped when its rho is
    black."""
    n = len(rp_p)
    lo = np.zeros((n, 30))
    ties = np.zeros((n, 3), bool)
    for i in range(n):
        black_r, black_t = not np.any(rho_r[i] != 0), not np.any(rho_t[i] != 0)
        if black_r and black_t:
            continue
        ep, em = np.zeros(30), np.zeros(30)
        for m in (1, 2, 0):   # direct + indirect + caustic
            if maps[m] is None:
                continue
            P, W, A, n_paths = maps[m]
            a, b, ties[i, m] = ephoton(P, W, A, n_paths, rp_p[i], rp_n[i], k, max_dist)
            ep, em = ep + a, em + b
        if not black_r:
            lo[i] += float(INV_PI32) * rho_r[i].astype(np.float64) * ep
        if not black_t:
            lo[i] += float(INV_PI32) * rho_t[i].astype(np.float64) * em
    return lo, ties


def nearest_facing(rp_p, rp_n, q, n):
    """RadiancePhotonProcess from an infinite radius: (index of the nearest photon with Dot(rp.n, n) > 0 or -1, tie)."""
    facing = np.flatnonzero(dot_f32(n, rp_n) > 0)   # the products commute, the sum order is the reference's
    if len(facing) == 0:
        return -1, False
    with np.errstate(over="ignore"):
        d2 = d2_f32(np.asarray(rp_p, F32).reshape(-1, 3)[facing], q)
    if not (d2 < np.inf).any():   # every d2 overflowed: `dist2 < maxDistSquared` (kdtree.h:181) never holds
        return -1, False
    j = int(np.argmin(d2))
    return int(facing[j]), bool((d2 == d2[j]).sum() > 1)


def lo_error(got, ref):
    """The project's bar: relative L2 over the 30 bins per radiance photon, floored at 1e-6 of the largest reference value."""
    ref = np.asarray(ref, np.float64)
    floor = 1e-6 * float(np.abs(ref).max()) if ref.size else 0.0
    num = np.linalg.norm(np.asarray(got, np.float64) - ref, axis=1)
    return num / np.maximum(np.linalg.norm(ref, axis=1), max(floor, 1e-300))
