"""The yardstick of pvol_lphoton_batch: PhotonVolumeIntegrator::LPhoton (integrators/photonvolume.cpp:65-108) at
explicit points in plain numpy, no library.

The selection is exact: the fp32 DistanceSquared(photon.p, p) is formed in the reference's operation order, (dx dx + dy dy) + dz dz
with every intermediate rounded to float32; the photons with d2 < float32(maxdist)^2 are stable-sorted by d2 and the first nused
kept.  That gives n_found and radius2 (the reference's maxmd) as exact float32 values, and the flag "tie at the boundary"
(d2[k-1] == d2[k]): there the reference keeps whichever tied photon its traversal met first, and L may differ.

L is float64: sum of alpha x HG(wi, -w) x "photon inside the extent" (homogeneous kinds; a density region's p() does not test
Inside), divided by float32(4/3 pi dV) x sigma_s(p), dV = float32(r2 sqrt(r2)); zero where sigma_s(p) is black and where n_found < 10."""
import numpy as np

F = np.float32
VOL_NONE, VOL_HOMOGENEOUS, VOL_GRID, VOL_RAINBOW, VOL_EXPONENTIAL = 0, 1, 2, 3, 4
PI_F = F(3.14159265358979323846)   # core/pbrt.h:191: M_PI is a float literal


def _xform_point(m, p):
    """Transform::operator()(Point) (core/transform.h:187-201) in float32, left to right."""
    m = np.asarray(m, F).reshape(4, 4)
    p = np.asarray(p, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(4)]
    one = r[3] == F(1)
    inv = np.where(one, F(1), F(1) / np.where(one, F(1), r[3])).astype(F)
    return np.stack([np.where(one, r[i], r[i] * inv) for i in range(3)], axis=1).astype(F)


class Medium:
    """What LPhoton asks of the scene's volume region (a scene blob's vol.* entries): g, sigma_s at a point, p()'s Inside test."""

    def __init__(self, s):
        self.kind = int(s["vol.kind"][0])
        self.g = float(s["vol.g"][0])
        self.sigma_s = np.asarray(s["vol.sigma_s"], F).reshape(-1)[:30]
        ext = np.asarray(s["vol.extent"], F)
        self.lo, self.hi = ext[:3], ext[3:]
        self.w2v = np.asarray(s["vol.w2v"], F)
        if self.kind == VOL_GRID:
            self.dims = [int(v) for v in s["vol.dims"]]
            self.grid = np.asarray(s["vol.density"], F).reshape(self.dims[2], self.dims[1], self.dims[0])
        if self.kind == VOL_EXPONENTIAL:
            self.a, self.b = (F(v) for v in np.asarray(s["vol.exp"], F).reshape(2))
            up = np.asarray(s["vol.updir"], F).reshape(3)
            inv = F(1) / F(np.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2]))   # Normalize(): one reciprocal, three products
            self.up = (up * inv).astype(F)

    def region(self):
        return self.kind in (VOL_GRID, VOL_EXPONENTIAL)

    def inside(self, p):
        q = _xform_point(self.w2v, p)
        return ((q >= self.lo) & (q <= self.hi)).all(axis=1)   # BBox::Inside, geometry.h:404-408

    def photon_weight(self, p):
        """HomogeneousVolumeDensity::p tests Inside (homogeneous.h:76-79); DensityRegion::p (volume.h:93-95) does not."""
        return np.ones(len(p), bool) if self.region() else self.inside(p)

    def density(self, p):
        """The factor of sigma_s at world points p, float32."""
        q = _xform_point(self.w2v, p)
        ins = ((q >= self.lo) & (q <= self.hi)).all(axis=1)
        if self.kind == VOL_NONE:
            return np.zeros(len(q), F)
        if self.kind == VOL_EXPONENTIAL:   # volumes/exponential.h:58-62
            d = q - self.lo
            h = ((d[:, 0] * self.up[0] + d[:, 1] * self.up[1]) + d[:, 2] * self.up[2]).astype(F)
            return np.where(ins, self.a * np.exp((-self.b * h).astype(F)).astype(F), F(0)).astype(F)
        if self.kind != VOL_GRID:
            return ins.astype(F)
        # VolumeGridDensity::Density, volumes/volumegrid.cpp:39-57
        n = [F(v) for v in self.dims]
        v = [(((q[:, i] - self.lo[i]) / (self.hi[i] - self.lo[i])).astype(F) * n[i] - F(.5)).astype(F) for i in range(3)]
        vi = [np.floor(c).astype(np.int64) for c in v]
        dx, dy, dz = [(v[i] - vi[i].astype(F)).astype(F) for i in range(3)]

        def D(x, y, z):
            x, y, z = (np.clip(c, 0, self.dims[i] - 1) for i, c in enumerate((x, y, z)))
            return self.grid[z, y, x]

        def lerp(t, a, b):
            return ((F(1) - t) * a + t * b).astype(F)
        x, y, z = vi
        d00 = lerp(dx, D(x, y, z), D(x + 1, y, z))
        d10 = lerp(dx, D(x, y + 1, z), D(x + 1, y + 1, z))
        d01 = lerp(dx, D(x, y, z + 1), D(x + 1, y, z + 1))
        d11 = lerp(dx, D(x, y + 1, z + 1), D(x + 1, y + 1, z + 1))
        return np.where(ins, lerp(dz, lerp(dy, d00, d10), lerp(dy, d01, d11)), F(0)).astype(F)

    def sigma_s_at(self, p):
        return (self.density(p)[:, None] * self.sigma_s[None, :]).astype(F)   # float x Spectrum, per bin



def dist2(photon_p, q):
    """DistanceSquared(photon.p, q) (geometry.h, kdtree.h:180) for every query (rows) and photon (columns), float32 throughout."""
    pp = np.asarray(photon_p, F).reshape(-1, 3)
    q = np.asarray(q, F).reshape(-1, 3)
    dx = pp[None, :, 0] - q[:, None, 0]
    dy = pp[None, :, 1] - q[:, None, 1]
    dz = pp[None, :, 2] - q[:, None, 2]
    return ((dx * dx + dy * dy) + dz * dz).astype(F)


def select(photon_p, q, nused, maxdist):
    """(kept, n_found, radius2, tie): kept[i] the photon indices query i keeps, nearest first, ties in photon order."""
    d2 = dist2(photon_p, q)
    max2 = F(maxdist) * F(maxdist)   # photonvolume.h:18
    near = d2 < max2
    n_cand = near.sum(axis=1)
    d2m = np.where(near, d2, F(np.inf))
    take = min(nused + 1, d2.shape[1])
    order = np.argsort(d2m, axis=1, kind="stable")[:, :take]
    val = np.take_along_axis(d2m, order, axis=1)
    n_found = np.minimum(n_cand, nused).astype(np.uint32)
    rows = np.arange(len(d2))
    radius2 = np.where(n_found > 0, val[rows, np.maximum(n_found.astype(np.int64) - 1, 0)], F(0)).astype(F)
    tie = np.zeros(len(d2), bool)
    if take > nused:
        tie = (n_cand > nused) & (val[:, nused - 1] == val[:, nused])
    kept = [order[i, :n_found[i]] for i in range(len(d2))]
    return kept, n_found, radius2, tie


def phase_hg(wi, wo, g):
    """PhaseHG (core/volume.cpp:150-154), float64."""
    if g == 0.0:
        return np.full(len(wi), 1.0 / (4.0 * np.pi))
    cos = np.asarray(wi, np.float64) @ np.asarray(wo, np.float64)
    return 1.0 / (4.0 * np.pi) * (1.0 - g * g) / np.power(1.0 + g * g - 2.0 * g * cos, 1.5)


def lphoton(photons, q, w, nused, maxdist, medium):
    """LPhoton at the points q with directions w (None: g must be 0).  photons = (p, wi, alpha).  Returns a dict: L[n,30] float64,
    n_found uint32, radius2 float32, tie bool, sigma_s[n,30]."""
    pp, wi, alpha = (np.asarray(a, F) for a in photons)
    pp, wi, alpha = pp.reshape(-1, 3), wi.reshape(-1, 3), alpha.reshape(-1, 30)
    q = np.asarray(q, F).reshape(-1, 3)
    n = len(q)
    sig = medium.sigma_s_at(q)
    if len(pp) == 0:
        return dict(L=np.zeros((n, 30)), n_found=np.zeros(n, np.uint32), radius2=np.zeros(n, F), tie=np.zeros(n, bool), sigma_s=sig)
    assert w is not None or medium.g == 0.0
    kept, n_found, radius2, tie = select(pp, q, nused, maxdist)
    weight = medium.photon_weight(pp).astype(np.float64)
    a64 = alpha.astype(np.float64)
    L = np.zeros((n, 30))
    for i in range(n):
        if n_found[i] < 10 or not sig[i].any():   # photonvolume.cpp:83-84; scale.IsBlack()
            continue
        k = kept[i]
        ph = phase_hg(wi[k], -np.asarray(w, F).reshape(-1, 3)[i], medium.g) if medium.g != 0.0 else np.full(len(k), 1.0 / (4.0 * np.pi))
        flux = (a64[k] * (ph * weight[k])[:, None]).sum(axis=0)
        r2 = radius2[i]
        dV = F(r2 * F(np.sqrt(r2)))
        if dV == 0:
            continue
        f = F(4.0 / 3.0 * np.float64(PI_F) * np.float64(dV))   # photonvolume.cpp:103: a double product, stored as float
        with np.errstate(divide="ignore", invalid="ignore"):
            L[i] = flux / (np.float64(f) * sig[i].astype(np.float64))
    return dict(L=L, n_found=n_found, radius2=radius2, tie=tie, sigma_s=sig)


def rel_l2(a, b, floor=1e-30):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), floor)
