// pvol_closest_dev.h -- included by pvol_march.hip (and through it pvol_surface_dev.h, pvol_group_dev.h, pvol_tile_dev.h) and by
// pvol_probe.hip.  The per-lane forms of Scene::Intersect / Scene::IntersectP (core/scene.h:50-61): one ray per lane, the whole
// scene.  surf_closest takes the triangles (linear scan or hierarchy), then the spheres, so that a sphere wins an equal t;
// lane_occluded asks the spheres first and then the triangles -- any hit will do.  They live here, unchanged, so that the test probe
// (pvol_probe.hip) calls the very functions the surface kernel, the tile pre-pass, the specular recursion and the march kernels call.
#ifndef PVOL_CLOSEST_DEV_H
#define PVOL_CLOSEST_DEV_H
#include "pvol_shading_dev.h"

// Scene::IntersectP for one lane: spheres, then the hierarchy or the scan
__device__ __forceinline__ bool lane_occluded(const DevScene &S, const RayD &vis) {
    if (S.nSpheres && spheres_occluded(S, vis.o, vis.d, vis.mint, vis.maxt)) return true;
    if (S.bvhNodes) return bvh_occluded(S, vis.o, vis.d, vis.mint, vis.maxt);
    bool hit = false;
    for (int t = 0; t < S.nTris && !hit; ++t) hit = tri_hit(S.tris[t], vis);
    return hit;
}

struct SurfHit {
    int tri, mat;   // tri: where the triangle's vertices lie -- scene index (linear scan) or hierarchy slot; -1 - i: sphere i
    float t;
    float rayEps;   // Intersection::rayEpsilon: 1e-3 t for a triangle (trianglemesh.cpp:205), 5e-4 t for a sphere (sphere.cpp:155)
    V3 p, nn;
    V3 dpdu;        // the BSDF's frame starts from it (core/reflection.cpp:619-627)
};                  // nn, dpdu are the SHADING geometry where the triangle carries vertex normals (pvol_shading_dev.h)
// isect.dg.nn, the geometric normal (BSDF::f's side test): the hit's nn unless the scene has vertex normals
__device__ __forceinline__ V3 surf_ng(const DevScene &S, const SurfHit &h) { return (S.triN && h.tri >= 0) ? geometric_normal(S, h.tri) : h.nn; }
// Scene::Intersect for one lane: closest hit, the later triangle on equal t (as the linear scans of this library and its oracle),
// DifferentialGeometry normal as shapes/trianglemesh.cpp:163-181 + core/diffgeom.cpp:46-54 build it
__device__ bool surf_closest(const DevScene &S, V3 o, V3 d, float mint, SurfHit *h) {
    float mt = INFINITY;
    int best = -1, where = -1;
    V3 p1, p2, p3;
    bool flip;
    if (S.bvhNodes) {
        const int slot = bvh_closest(S, o, d, mint, INFINITY, &mt);
        if (slot < 0 && !S.nSpheres) return false;
        if (slot >= 0) {
        const float4 q1 = S.bvhTris[3 * slot], q2 = S.bvhTris[3 * slot + 1], q3 = S.bvhTris[3 * slot + 2];
        p1 = v3(q1.x, q1.y, q1.z); p2 = v3(q2.x, q2.y, q2.z); p3 = v3(q3.x, q3.y, q3.z);
        best = __float_as_int(q1.w);
        where = slot;
        h->mat = __float_as_int(q2.w);
        flip = __float_as_int(q3.w) != 0;
        }
    } else {
        for (int i = 0; i < S.nTris; ++i) {
            float t;
            if (tri_closest(S.tris[i], o, d, mint, mt, &t)) { mt = t; best = i; }
        }
        if (best < 0 && !S.nSpheres) return false;
        if (best >= 0) {
            const DevTri &tr = S.tris[best];
            p1 = v3(tr.p1[0], tr.p1[1], tr.p1[2]); p2 = v3(tr.p2[0], tr.p2[1], tr.p2[2]); p3 = v3(tr.p3[0], tr.p3[1], tr.p3[2]);
            h->mat = S.shootScene->triMat[best];
            flip = S.shootScene->triFlip[best] != 0;
            where = best;
        }
    }
    if (S.nSpheres) {   // Shape "sphere" (pvol_sphere_dev.h): tested after the triangles
        V3 ph, dpduW;
        const int si = spheres_closest(S, o, d, mint, &mt, &ph);
        if (si >= 0) {
            h->tri = -1 - si;
            h->mat = S.spheres[si].mat;
            h->t = mt;
            h->rayEps = 5e-4f * mt;
            sphere_dg(S.spheres[si], ph, &h->p, &dpduW, &h->nn);
            h->dpdu = dpduW;
            return true;
        }
        if (best < 0) return false;
    }
    const float du1 = 0.f - 1.f, du2 = 1.f - 1.f, dv1 = 0.f - 1.f, dv2 = 0.f - 1.f;
    const V3 dp1 = p1 - p3, dp2 = p2 - p3;
    const float invdet = 1.f / (du1 * dv2 - dv1 * du2);
    const V3 dpdu = (dp1 * dv2 - dp2 * dv1) * invdet;
    const V3 dpdv = (dp1 * (-du2) + dp2 * du1) * invdet;
    h->tri = where;
    h->t = mt;
    h->rayEps = 1e-3f * mt;
    h->p = o + d * mt;
    h->nn = normalize(cross(dpdu, dpdv));
    h->dpdu = dpdu;
    if (flip) h->nn = h->nn * -1.f;
    if (S.triN) {   // Triangle::GetShadingGeometry for a mesh with "normal N" (triN is in the scene's original order)
        const ShadingFrame f = shading_geometry(S.triN + (size_t)best * 9, p1, p2, p3, o, d, h->dpdu, flip);
        if (f.any) { h->dpdu = f.dpdu; h->nn = f.nn; }
    }
    return true;
}
#endif
