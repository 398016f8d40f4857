// pvol_radwalk_dev.h -- radianceMap->Lookup(p, RadiancePhotonProcess(n), INFINITY) (core/photonshooter.h:63-78) for one lane: the
// walk over the radiance map's grid that finds the nearest radiance photon whose normal faces n.  It exists once, here, and is
// included by pvol_radiance.hip (pvol_radiance_lookup*) and pvol_final_gather.hip (the gather rays' Lindir), so that both answer
// identically on identical input, ties included: the first photon in the walk's order wins an equal distance.
// Include after pvol_math.h.
#ifndef PVOL_RADWALK_DEV_H
#define PVOL_RADWALK_DEV_H
#include "pvol_gridrows_dev.h"

// The radiance map as the walk reads it: the grid, the photons' normals in the grid's order (pos4[j].w holds photon j's place in
// the input order as bits), and the slack of a shell's distance bound.  n == 0: no photons, nothing is found.
struct RadWalk {
    GridView g;
    const float4 *nrm4;
    uint32_t n;
    float eps;
};
struct pvol_ctx;
// the view of the context's radiance result (pvol_radiance.hip); its `rad.have` must hold
__attribute__((visibility("hidden"))) RadWalk pvol_radiance_walk(const pvol_ctx *c);

// Cube shells of cells outward from the query's (clamped) cell; a shell's cells lie beyond one of the six faces of the cube of
// shells before it, so the nearest of those faces that still has cells behind it bounds the shell's distance from below.
// Returns the photon's place in the grid's order, or -1 when no photon faces (nx, ny, nz).
__device__ __forceinline__ int64_t radiance_nearest(const RadWalk &W, const float q[3], float nx, float ny, float nz) {
    float best = INFINITY;
    int64_t bestIdx = -1;
    if (!W.n) return bestIdx;
    const GridView &g = W.g;
    int c0[3], maxS = 0;
    for (int a = 0; a < 3; ++a) {
        // clamped in float before the conversion: a huge (or, from the device entry point, non-finite) coordinate must not
        // reach an int conversion outside its range; fmaxf / fminf drop a NaN
        const float cf = fminf(fmaxf(floorf((q[a] - g.gridLo[a]) * g.invCell), 0.f), (float)(g.gdim[a] - 1));
        c0[a] = min(max((int)cf, 0), g.gdim[a] - 1);
        maxS = max(maxS, max(c0[a], g.gdim[a] - 1 - c0[a]));
    }
    for (int s = 0; s <= maxS; ++s) {
        if (s > 0) {
            float face = INFINITY;
            for (int a = 0; a < 3; ++a) {
                if (c0[a] + s <= g.gdim[a] - 1) face = fminf(face, (g.gridLo[a] + (float)(c0[a] + s) * g.cellSize) - q[a]);
                if (c0[a] - s >= 0) face = fminf(face, q[a] - (g.gridLo[a] + (float)(c0[a] - s + 1) * g.cellSize));
            }
            const float d = fmaxf(0.f, face - W.eps);
            if (best < INFINITY && d * d >= best) break;   // with nothing found yet (or every d2 so far overflowed) the walk goes on
        }
        const int z0 = max(0, c0[2] - s), z1 = min(g.gdim[2] - 1, c0[2] + s);
        const int y0 = max(0, c0[1] - s), y1 = min(g.gdim[1] - 1, c0[1] + s);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const bool wholeRow = abs(z - c0[2]) == s || abs(y - c0[1]) == s;
                const size_t base = ((size_t)z * g.gdim[1] + y) * g.gdim[0];
                // the row's cells of this shell: all of c0x - s .. c0x + s on a face, else the two ends
                for (int part = 0; part < 2; ++part) {
                    int x0, x1;
                    if (wholeRow) {
                        if (part) break;
                        x0 = max(0, c0[0] - s); x1 = min(g.gdim[0] - 1, c0[0] + s);
                    } else {
                        x0 = x1 = part ? c0[0] + s : c0[0] - s;
                        if (x0 < 0 || x0 > g.gdim[0] - 1) continue;
                    }
                    const uint32_t j0 = g.cellStart[base + x0], j1 = g.cellStart[base + x1 + 1];
                    for (uint32_t j = j0; j < j1; ++j) {
                        const float4 pp = g.pos4[j];
                        const float dx = pp.x - q[0], dy = pp.y - q[1], dz = pp.z - q[2];
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        if (d2 < best) {
                            const float4 rn = W.nrm4[j];
                            if (rn.x * nx + rn.y * ny + rn.z * nz > 0.f) { best = d2; bestIdx = (int64_t)j; }
                        }
                    }
                }
            }
    }
    return bestIdx;
}
#endif
