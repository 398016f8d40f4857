// pvol_closest_dev.h -- included by pvol_march.hip (and through it pvol_surface_dev.h, pvol_group_dev.h, pvol_tile_dev.h), pvol_shoot.hip,
// the gather-ray units and pvol_probe.hip.  The four forms of Scene::Intersect / IntersectP (core/scene.h:50-61) on one hit record:
//   surf_closest / lane_occluded    one ray per lane: the surface kernel, the tile pre-pass, the specular recursion, the march kernels
//   scene_closest / scene_occluded  one ray per wave, a triangle per lane: the photon shooter and the wave-per-ray march kernels
// A closest hit takes the triangles (scan or hierarchy), then the spheres, so that a sphere wins an equal t; an any-hit asks the
// spheres first -- any hit will do.  The test probe (pvol_probe.hip) calls all four, the very functions the kernels call.
// The closest-hit forms differ in their scan and the shooter's maxt; fetch, sphere step and differential geometry are the same text
// twice (as helpers they move shoot_kernel's spills): change both, probe mode 3 == mode 0 holds them together.
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
// Scene::IntersectP for one wave: one triangle per lane; a large scene walks its hierarchy (wave-uniform ray)
__device__ __forceinline__ bool scene_occluded(const DevScene &S, const RayD &ray, int lane) {
    if (S.nSpheres && spheres_occluded(S, ray.o, ray.d, ray.mint, ray.maxt)) return true;
    if (S.bvhNodes) return bvh_occluded(S, ray.o, ray.d, ray.mint, ray.maxt);
    bool hit = false;
    for (int base = 0; base < S.nTris; base += LANES) {
        int t = base + lane;
        bool h = (t < S.nTris) && tri_hit(S.tris[t], ray);
        hit = hit || wave_any(h);
    }
    return hit;
}

struct Hit {
    int tri, mat;   // tri: where the triangle's vertices lie -- scene index (linear scan) or hierarchy slot; -1 - i: sphere i
    float t;
    float rayEps;   // Intersection::rayEpsilon: 1e-3 t for a triangle (trianglemesh.cpp:205), 5e-4 t for a sphere (sphere.cpp:155)
    V3 p, nn;
    V3 dpdu;        // the BSDF's frame starts from it (core/reflection.cpp:619-627)
};                  // nn, dpdu are the SHADING geometry where the triangle carries vertex normals (pvol_shading_dev.h)
// isect.dg.nn, the geometric normal (BSDF::f's side test, the radiance photon's normal): the hit's nn unless the scene has vertex normals
__device__ __forceinline__ V3 hit_ng(const DevScene &S, const Hit &h) { return (S.triN && h.tri >= 0) ? geometric_normal(S, h.tri) : h.nn; }
// Scene::Intersect for one lane: closest hit, the later triangle on equal t (as the linear scans of this library and its oracle).
// Out of line on purpose.
__device__ bool surf_closest(const DevScene &S, V3 o, V3 d, float mint, Hit *h) {
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

// Scene::Intersect for one wave (the photon shooter; *maxt in and out as Ray::maxt is).  The serial scan tightens maxt with `t > maxt`
// rejections, so of several triangles at the same t the LATER one wins: one triangle per lane, minimum over the wave, highest lane of
// the tie.  Forced inline with everything on the shooter's path.
__device__ __forceinline__ bool scene_closest(const DevScene &S, const DevShootScene &H, V3 o, V3 d, float mint, float *maxt, Hit *hit, int lane) {
    float tk = INFINITY;
    bool any = false;
    int best = -1, where = -1;
    V3 p1, p2, p3;
    bool flip;
    if (S.bvhNodes) {   // large scene: every lane walks the hierarchy with the same ray (pvol_bvh_dev.h)
        const int slot = bvh_closest(S, o, d, mint, *maxt, &tk);
        if (slot < 0 && !S.nSpheres) return false;
        if (slot < 0) tk = INFINITY;
        else {
        const float4 q1 = S.bvhTris[3 * slot], q2 = S.bvhTris[3 * slot + 1], q3 = S.bvhTris[3 * slot + 2];
        p1 = v3(q1.x, q1.y, q1.z); p2 = v3(q2.x, q2.y, q2.z); p3 = v3(q3.x, q3.y, q3.z);
        best = __float_as_int(q1.w);
        where = slot;
        hit->mat = __float_as_int(q2.w);
        flip = __float_as_int(q3.w) != 0;
        }
    } else {
        for (int base = 0; base < S.nTris; base += LANES) {   // at most PVOL_MAX_TRIS == 64: one pass
            float t = 0.f;
            const bool h = (base + lane < S.nTris) && tri_closest(S.tris[base + lane], o, d, mint, *maxt, &t);
            const float tm = -wave_max(h ? -t : -INFINITY);
            if (__ballot(h) && tm <= tk) {
                const uint64_t m = __ballot(h && t == tm);
                tk = tm;
                best = base + 63 - __clzll((unsigned long long)m);
                any = true;
            }
        }
        if (!any && !S.nSpheres) return false;
        if (any) {
            const DevTri &tr = S.tris[best];
            p1 = v3(tr.p1[0], tr.p1[1], tr.p1[2]); p2 = v3(tr.p2[0], tr.p2[1], tr.p2[2]); p3 = v3(tr.p3[0], tr.p3[1], tr.p3[2]);
            hit->mat = H.triMat[best];
            flip = H.triFlip[best] != 0;
            where = best;
        }
    }
    if (S.nSpheres) {   // Shape "sphere" (pvol_sphere_dev.h), tested after the triangles with the ray shortened to their hit
        float ts = best >= 0 ? tk : *maxt;
        V3 ph;
        const int si = spheres_closest(S, o, d, mint, &ts, &ph);
        if (si >= 0) {
            *maxt = ts;
            hit->tri = -1 - si;
            hit->mat = S.spheres[si].mat;
            hit->t = ts;
            hit->rayEps = 5e-4f * ts;   // sphere.cpp:155
            sphere_dg(S.spheres[si], ph, &hit->p, &hit->dpdu, &hit->nn);
            return true;
        }
        if (best < 0) return false;
    }
    *maxt = tk;
    // shapes/trianglemesh.cpp:163-181 with the default uvs (0,0),(1,0),(1,1)
    float du1 = 0.f - 1.f, du2 = 1.f - 1.f, dv1 = 0.f - 1.f, dv2 = 0.f - 1.f;
    V3 dp1 = p1 - p3, dp2 = p2 - p3;
    float determinant = du1 * dv2 - dv1 * du2;
    float invdet = 1.f / determinant;
    hit->dpdu = (dp1 * dv2 - dp2 * dv1) * invdet;
    V3 dpdv = (dp1 * (-du2) + dp2 * du1) * invdet;
    hit->tri = where;
    hit->t = tk;
    hit->p = o + d * tk;
    hit->rayEps = 1e-3f * tk;
    hit->nn = normalize(cross(hit->dpdu, dpdv));   // core/diffgeom.cpp:46-54
    if (flip) hit->nn = hit->nn * -1.f;
    if (S.triN) {   // Triangle::GetShadingGeometry for a mesh with "normal N" (triN is in the scene's original order)
        const ShadingFrame f = shading_geometry(S.triN + (size_t)best * 9, p1, p2, p3, o, d, hit->dpdu, flip);
        if (f.any) { hit->dpdu = f.dpdu; hit->nn = f.nn; }
    }
    return true;
}
#endif
