"""numpy restatement of SingleScatteringIntegrator::Li (integrators/single.cpp:66-139) over the scene blobs of tests/golden, shared by
test_single_ref.py and test_gpu_single.py.  Decisions -- step counts, slab clips, the inside test, the cone's edge, the roulette -- are
taken in float32 in the reference's order; Tr is a float32 spectrum multiplied step by step as single.cpp:101 does; radiance is summed
in float64.  `photon=True` turns the three statements in which single.cpp differs back into photonvolume.cpp's (Tr assigned per step
:155, Lv = sa Lve step + ss L_i step + Tr Lv :215, the return value :221) with an empty map, which is what ties this file to the
oracle (test_single_ref.py).  Covered: the MT19937 stream (core/rng.cpp), the three LDShuffleScrambled arrays (core/montecarlo.h),
tau() of a homogeneous extent and DensityRegion::tau over VolumeGrid and exponential densities, the three delta lights.  Occlusion is
a callable so that the tests can hand in Oracle.hits."""
import numpy as np

F32 = np.float32
U32 = np.uint32
PI32 = F32(3.14159265358979323846)
HOMOGENEOUS, GRID, RAINBOW, EXPONENTIAL = 1, 2, 3, 4
POINT, SPOT, DISTANT = 0, 1, 2


class MT:
    """core/rng.cpp:43-107."""

    def __init__(self, seed=None, state=None):
        if state is not None:
            self.mt = np.array(state[:624], np.uint32)
            self.mti = int(state[624])
        else:
            mt = np.zeros(624, np.uint64)
            x = int(seed) & 0xffffffff
            mt[0] = x
            for i in range(1, 624):
                x = (1812433253 * (x ^ (x >> 30)) + i) & 0xffffffff
                mt[i] = x
            self.mt = mt.astype(np.uint32)
            self.mti = 624
        self.draws = 0

    def _regenerate(self):
        mt = self.mt

        def twist(a, b):
            y = (a & U32(0x80000000)) | (b & U32(0x7fffffff))
            return (y >> U32(1)) ^ np.where(y & U32(1), U32(0x9908b0df), U32(0))
        mt[0:227] = mt[397:624] ^ twist(mt[0:227], mt[1:228])
        mt[227:454] = mt[0:227] ^ twist(mt[227:454], mt[228:455])
        mt[454:623] = mt[227:396] ^ twist(mt[454:623], mt[455:624])
        mt[623] = mt[396] ^ twist(mt[623:624], mt[0:1])[0]
        self.mti = 0

    def skip(self, n):
        n = int(n)
        self.draws += n
        while n > 0:
            if self.mti >= 624:
                self._regenerate()
            take = min(n, 624 - self.mti)
            self.mti += take
            n -= take

    def uint(self):
        if self.mti >= 624:
            self._regenerate()
        y = int(self.mt[self.mti])
        self.mti += 1
        self.draws += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        y ^= y >> 18
        return y & 0xffffffff

    def float(self):
        return F32((self.uint() & 0xffffff) / float(1 << 24))

    def state(self):
        return np.concatenate([self.mt, np.array([self.mti], np.uint32)])


def van_der_corput(n, scramble):
    n = int("{:032b}".format(n)[::-1], 2) ^ scramble
    return min(F32(((n >> 8) & 0xffffff) / float(1 << 24)), F32(np.nextafter(F32(1), F32(0))))


def ld_shuffle_scrambled_1d(n, rng):
    """LDShuffleScrambled1D(1, n, samples, rng), montecarlo.h:296-304: 1 + n + n draws."""
    scramble = rng.uint()
    s = [van_der_corput(i, scramble) for i in range(n)]
    rng.skip(n)   # Shuffle(samples + i, 1, 1, rng): i + RandomUInt() % 1
    for i in range(n):
        other = i + rng.uint() % (n - i)
        s[i], s[other] = s[other], s[i]
    return s


def _f32v(a):
    return np.asarray(a, F32).reshape(3)


def xform_point(m, p):
    x = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3]
    y = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + m[7]
    z = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + m[11]
    w = ((m[12] * p[0] + m[13] * p[1]) + m[14] * p[2]) + m[15]
    v = np.array([x, y, z], F32)
    return v if w == F32(1) else v * (F32(1) / w)


def xform_vector(m, v):
    return np.array([(m[0] * v[0] + m[1] * v[1]) + m[2] * v[2], (m[4] * v[0] + m[5] * v[1]) + m[6] * v[2],
                     (m[8] * v[0] + m[9] * v[1]) + m[10] * v[2]], F32)


def length(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def vdiv(v, f):
    return v * (F32(1) / f)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class Medium:
    """The volume region and the lights of a scene blob."""

    def __init__(self, s, step_size):
        self.kind = int(s["vol.kind"][0])
        self.lo, self.hi = np.asarray(s["vol.extent"][:3], F32), np.asarray(s["vol.extent"][3:], F32)
        self.w2v = np.asarray(s["vol.w2v"], F32).reshape(16)
        self.sig_a, self.sig_s, self.le = (np.asarray(s[k], F32).reshape(30) for k in ("vol.sigma_a", "vol.sigma_s", "vol.le"))
        self.sig_t = self.sig_a + self.sig_s
        self.g = F32(s["vol.g"][0])
        self.step = F32(step_size)
        self.cie_y = np.asarray(s["cie.y"], F32).reshape(30)
        self.region = self.kind in (GRID, EXPONENTIAL)
        if self.kind == GRID:
            self.nx, self.ny, self.nz = (int(v) for v in s["vol.dims"])
            self.density = np.asarray(s["vol.density"], F32).reshape(self.nz, self.ny, self.nx)
        if self.kind == EXPONENTIAL:
            self.exp_a, self.exp_b = (F32(v) for v in s["vol.exp"])
            up = _f32v(s["vol.updir"])
            self.up = vdiv(up, length(up))
        n = len(s["lights.kind"])
        self.lights = [dict(kind=int(s["lights.kind"][i]), pos=_f32v(s["lights.pos"][3 * i:3 * i + 3]), dir=_f32v(s["lights.dir"][3 * i:3 * i + 3]),
                            w2l=np.asarray(s["lights.w2l"][16 * i:16 * i + 16], F32), I=np.asarray(s["lights.intensity"][30 * i:30 * i + 30], F32),
                            cos_total=F32(s["lights.cos"][2 * i]), cos_start=F32(s["lights.cos"][2 * i + 1])) for i in range(n)]

    def y(self, c):   # SampledSpectrum::y, core/spectrum.h:433-439
        yy = F32(0)
        for i in range(30):
            yy = yy + self.cie_y[i] * c[i]
        return yy * F32(300) / F32(106.856895 * 30)

    def inside(self, pv):
        return bool(np.all(pv >= self.lo) and np.all(pv <= self.hi))

    def intersect(self, o, d, mint, maxt):   # VolumeRegion::IntersectP -> BBox::IntersectP, core/geometry.cpp:68-86
        ov, dv = xform_point(self.w2v, o), xform_vector(self.w2v, d)
        t0, t1 = F32(mint), F32(maxt)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for i in range(3):
                inv = F32(1) / dv[i]
                tn, tf = (self.lo[i] - ov[i]) * inv, (self.hi[i] - ov[i]) * inv
                if tn > tf:
                    tn, tf = tf, tn
                t0 = tn if tn > t0 else t0
                t1 = tf if tf < t1 else t1
                if t0 > t1:
                    return None
        return t0, t1

    def density_at(self, pv):
        """Density(Pobj): volumegrid.cpp:39-57, exponential.h:58-62; 1 / 0 for the homogeneous extent's Inside()."""
        if not self.inside(pv):
            return F32(0)
        if self.kind == EXPONENTIAL:
            return self.exp_a * np.exp(-self.exp_b * dot(pv - self.lo, self.up), dtype=F32)
        if self.kind != GRID:
            return F32(1)
        vox = (pv - self.lo) / (self.hi - self.lo)
        vox = vox * np.array([self.nx, self.ny, self.nz], F32) - F32(.5)
        v = np.floor(vox).astype(np.int64)
        dx, dy, dz = (vox - v.astype(F32)).astype(F32)

        def D(x, y, z):
            return self.density[min(max(z, 0), self.nz - 1), min(max(y, 0), self.ny - 1), min(max(x, 0), self.nx - 1)]

        def lerp(t, a, b):
            return (F32(1) - t) * a + t * b
        x, y, z = (int(c) for c in v)
        d00, d10 = lerp(dx, D(x, y, z), D(x + 1, y, z)), lerp(dx, D(x, y + 1, z), D(x + 1, y + 1, z))
        d01, d11 = lerp(dx, D(x, y, z + 1), D(x + 1, y, z + 1)), lerp(dx, D(x, y + 1, z + 1), D(x + 1, y + 1, z + 1))
        return lerp(dz, lerp(dy, d00, d10), lerp(dy, d01, d11))

    def tau(self, o, d, mint, maxt, step, u):
        """VolumeRegion::tau: homogeneous.h:80-84, DensityRegion::tau core/volume.cpp:296-310.  float32[30]."""
        if not self.region:
            h = self.intersect(o, d, mint, maxt)
            if h is None:
                return np.zeros(30, F32)
            return length((o + d * h[0]) - (o + d * h[1])) * self.sig_t
        ln = length(d)
        if ln == 0:
            return np.zeros(30, F32)
        dn = vdiv(d, ln)
        h = self.intersect(o, dn, F32(mint) * ln, F32(maxt) * ln)
        if h is None:
            return np.zeros(30, F32)
        t0, t1 = h
        tau = np.zeros(30, F32)
        t0 = t0 + F32(u) * step
        while t0 < t1:
            tau = tau + self.density_at(xform_point(self.w2v, o + dn * t0)) * self.sig_t
            t0 = t0 + step
        return tau * step

    def phase(self, w, wp):   # PhaseHG, core/volume.cpp:150-154
        if self.g == 0:
            return F32(1) / (F32(4) * PI32)
        c = dot(w, wp)
        return F32(1) / (F32(4) * PI32) * (F32(1) - self.g * self.g) / np.power(F32(1) + self.g * self.g - F32(2) * self.g * c, F32(1.5))

    def sample_light(self, light, p):
        """Light::Sample_L(p, 0, ...) of distant.cpp:48-55, point.cpp:50-57, spot.cpp:50-69: (L[30] float32, wo, shadow ray o, d, maxt)."""
        if light["kind"] == DISTANT:
            return light["I"], light["dir"], (p, light["dir"], F32(np.inf))
        lp = light["pos"]
        wo = vdiv(lp - p, length(lp - p))
        dist = length(p - lp)
        vis = (p, vdiv(lp - p, dist), dist * (F32(1) - F32(0)))
        d2 = dot(lp - p, lp - p)
        fall = F32(1)
        if light["kind"] == SPOT:
            wl = xform_vector(light["w2l"], -wo)
            cos = vdiv(wl, length(wl))[2]
            if cos < light["cos_total"]:
                fall = F32(0)
            elif cos > light["cos_start"]:
                fall = F32(1)
            else:
                delta = (cos - light["cos_total"]) / (light["cos_start"] - light["cos_total"])
                fall = delta * delta * delta * delta
        return light["I"] * fall / d2, wo, vis


def li(M, ray, rng, occluded, photon=False, info=None):
    """One call of Li(): (Lv[30] float64, T[30] float32).  `occluded(o[n, 3], d[n, 3], maxt[n]) -> bool[n]` is Scene::IntersectP with
    mint 0.  `info` (a dict) receives what the tests select by: steps begun, roulette tests, whether the ray was killed, the
    smallest relative distance of any step's Tr.y() from the 1e-3 threshold, and the light samples that were unoccluded, black (they
    draw nothing) or shadowed."""
    o, d = _f32v(ray["o"]), _f32v(ray["d"])
    T1, Z = np.ones(30, F32), np.zeros(30)
    if info is not None:
        info.update(steps=0, tests=0, killed=False, margin=np.inf, unoccluded=0, black=0, shadowed=0)
    h = M.intersect(o, d, ray["mint"], ray["maxt"]) if M.kind != 0 else None
    if h is None or (h[1] - h[0]) == 0:
        return Z, T1
    t0, t1 = h
    n = int(np.ceil((t1 - t0) / M.step))
    step = (t1 - t0) / F32(n)
    Tr = T1.copy()
    p = o + d * t0
    w = -d
    t0 = t0 + F32(ray["scatter_u"]) * step
    light_num = ld_shuffle_scrambled_1d(n, rng)
    rng.skip(3 + 4 * n)   # lightComp (1 + 2n) and lightPos (2 + 2n): the delta lights read neither
    # the march points and their light samples do not depend on drawn values: one occlusion call per light for the whole ray
    pts = []
    for i in range(n):
        pts.append(o + d * t0)
        t0 = t0 + step
    n_lights = len(M.lights)
    samples = [[M.sample_light(L, q) for q in pts] for L in M.lights]
    occ = [occluded(np.array([s[2][0] for s in row]), np.array([s[2][1] for s in row]), np.array([s[2][2] for s in row])) for row in samples]
    Lv = np.zeros(30)
    for i in range(n):
        p_prev, p = p, pts[i]
        if info is not None:
            info["steps"] += 1
        step_tau = M.tau(p_prev, p - p_prev, 0, 1, F32(.5) * M.step, rng.float())
        e = np.exp(-step_tau, dtype=F32)
        Tr = e if photon else Tr * e
        yv = M.y(Tr)
        if info is not None:
            info["margin"] = min(info["margin"], abs(float(yv) / 1e-3 - 1.0))
        if yv < 1e-3:
            if info is not None:
                info["tests"] += 1
            if rng.float() > F32(.5):
                Tr = np.zeros(30, F32)
                if info is not None:
                    info["killed"] = True
                break
            Tr = Tr / F32(.5)
        pv = xform_point(M.w2v, p)
        dens = M.density_at(pv)
        ss, sa = M.sig_s * dens, M.sig_a * dens
        lve = M.le * dens
        Ld_term = np.zeros(30)
        if ss.any() and n_lights > 0:
            ln = min(int(np.floor(light_num[i] * F32(n_lights))), n_lights - 1)
            L, wo, vis = samples[ln][i]
            if info is not None:
                info["black"] += int(not L.any())
                info["shadowed"] += int(bool(L.any()) and bool(occ[ln][i]))
            if L.any() and not occ[ln][i]:
                if info is not None:
                    info["unoccluded"] += 1
                Ttr = np.exp(-M.tau(vis[0], vis[1], 0, vis[2], F32(4) * M.step, rng.float()), dtype=F32)
                ph = M.phase(w, -wo) if (M.region or M.inside(pv)) else F32(0)   # homogeneous.h:76-79
                Ld_term = float(ph) * (L.astype(np.float64) * Ttr) * float(n_lights)
        if photon:
            Lv = sa.astype(np.float64) * lve * float(step) + ss.astype(np.float64) * Ld_term * float(step) + Tr.astype(np.float64) * Lv
        else:
            Lv = Lv + Tr.astype(np.float64) * lve + Tr.astype(np.float64) * ss * Ld_term
    return (Lv if photon else Lv * float(step)), Tr


def li_batch(s, step_size, rays, streams, occluded, photon=False, states=None, infos=None):
    """pvol_li_batch's contract: (out[n, 60] float64, draws[n] uint32, end_draw[nStreams] uint64, final states[nStreams, 625]).
    states: per stream the live MT19937 state (625 words) instead of seed + start_draw."""
    M = Medium(s, step_size)
    out = np.zeros((len(rays), 60))
    draws = np.zeros(len(rays), np.uint32)
    ends = np.zeros(len(streams), np.uint64)
    finals = np.zeros((len(streams), 625), np.uint32)
    for si, st in enumerate(streams):
        if states is not None:
            rng = MT(state=states[si])
            rng.draws = int(st["start_draw"])
        else:
            rng = MT(seed=int(st["seed"]))
            rng.skip(int(st["start_draw"]))
        for k in range(int(st["n_rays"])):
            ri = int(st["first_ray"]) + k
            rng.skip(int(rays[ri]["rng_skip"]))
            d0 = rng.draws
            info = {} if infos is not None else None
            Lv, T = li(M, rays[ri], rng, occluded, photon, info)
            if infos is not None:
                infos[ri] = info
            out[ri, :30], out[ri, 30:] = Lv, T
            draws[ri] = rng.draws - d0
        ends[si] = rng.draws
        finals[si] = rng.state()
    return out, draws, ends, finals


def xyz_rows(s, out):
    """PVOL_OUT_XYZ of spectral rows: X, Y, Z of Lv (core/spectrum.h:421-431) and T.y()."""
    scale = 300.0 / (106.856895 * 30)
    cie = [np.asarray(s[k], np.float64) for k in ("cie.x", "cie.y", "cie.z")]
    return np.stack([out[:, :30] @ cie[0] * scale, out[:, :30] @ cie[1] * scale, out[:, :30] @ cie[2] * scale, out[:, 30:] @ cie[1] * scale], axis=1)


def oracle_occlusion(oracle):
    """Scene::IntersectP through Oracle.hits (flag 0 of its record)."""
    def occluded(o, d, maxt):
        if len(maxt) == 0:
            return np.zeros(0, bool)
        f, _ = oracle.hits(o, d, np.zeros(len(maxt), F32), maxt)
        return f[:, 0] != 0
    return occluded


def row_error(got, ref):
    """The project's bar as tests/test_gpu_parity.py takes it: relative L2 per ray over Lv, floored at 1e-6 of the batch's largest
    reference value, and over T without a floor.  Returns the larger of the two per ray."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    errs = []
    for a, b, floor in ((got[:, :30], ref[:, :30], 1e-6 * float(np.abs(ref[:, :30]).max()) if ref.size else 0.0), (got[:, 30:], ref[:, 30:], 0.0)):
        errs.append(np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), max(floor, 1e-30)))
    return np.maximum(errs[0], errs[1])
