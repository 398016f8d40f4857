// pvol_shading_dev.h -- included by pvol_closest_dev.h.
//
// Triangle::GetShadingGeometry (shapes/trianglemesh.cpp:293-368) for a mesh with per-vertex normals and neither "S" nor "uv": the
// default uvs (0,0), (1,0), (1,1) of Triangle::GetUVs.  The vertex normals come from DevScene::triN, already in world space (the
// reference interpolates in object space and transforms the sum; the map is linear, so the two differ by rounding: DESIGN.md 16).
//
// What the callers keep of the shading DifferentialGeometry is what the BSDF's frame is built from (core/reflection.cpp:619-627):
// dpdu = ss and nn = Normalize(Cross(ss, ts)), negated for ReverseOrientation ^ TransformSwapsHandedness as the constructor does for
// every DifferentialGeometry (core/diffgeom.cpp:46-54) -- so a reversed mesh flips its SHADING normal too.  That is the reference.
#ifndef PVOL_SHADING_DEV_H
#define PVOL_SHADING_DEV_H
#include "pvol_bsdf_dev.h"

struct ShadingFrame { V3 dpdu, nn; bool any; };

// n9: the triangle's three vertex normals (any == false when all nine are zero: the mesh has none, the frame is not computed).
// p1, p2, p3: the hit triangle; o, d: the ray that hit it (the barycentrics are Triangle::Intersect's own, trianglemesh.cpp:136-153,
// recomputed from the same operands); dpdu: dg.dpdu.  Out of line: the kernels that call it sit at their register budgets.
__device__ __attribute__((noinline)) ShadingFrame shading_geometry(const float *n9, V3 p1, V3 p2, V3 p3, V3 o, V3 d, V3 dpdu, bool flip) {
    ShadingFrame r;
    r.dpdu = dpdu; r.nn = v3(0.f, 0.f, 0.f);
    const V3 n0 = v3(n9[0], n9[1], n9[2]), n1 = v3(n9[3], n9[4], n9[5]), n2 = v3(n9[6], n9[7], n9[8]);
    r.any = n0.x != 0.f || n0.y != 0.f || n0.z != 0.f || n1.x != 0.f || n1.y != 0.f || n1.z != 0.f || n2.x != 0.f || n2.y != 0.f || n2.z != 0.f;
    if (!r.any) return r;
    const V3 e1 = p2 - p1, e2 = p3 - p1;
    const V3 s1 = cross(d, e2);
    const float invDivisor = 1.f / dot(s1, e1);
    const V3 s = o - p1;
    const float b1 = dot(s, s1) * invDivisor;
    const V3 s2 = cross(s, e1);
    const float b2 = dot(d, s2) * invDivisor;
    // dg.u = b0 * 0 + b1 * 1 + b2 * 1, dg.v = b0 * 0 + b1 * 0 + b2 * 1 (trianglemesh.cpp:185-187): the products with 0 and 1 are exact
    const float tu = b1 + b2, tv = b2;
    // SolveLinearSystem2x2 (core/transform.cpp:39-49) with A = {{1, 1}, {0, 1}}, det 1: x0 = (1 * tu - 1 * tv) / 1, x1 = (1 * tv - 0 * tu) / 1
    float bb1 = tu - tv, bb2 = tv, bb0;
    if (bb1 != bb1 || bb2 != bb2) bb0 = bb1 = bb2 = 1.f / 3.f;   // degenerate parametric mapping (:312-315)
    else bb0 = 1.f - bb1 - bb2;
    const V3 ns = normalize(n0 * bb0 + n1 * bb1 + n2 * bb2);
    V3 ss = normalize(dpdu);
    V3 ts = cross(ss, ns);
    if (len_sq(ts) > 0.f) {
        ts = normalize(ts);
        ss = cross(ts, ns);
    } else if (fabsf(ns.x) > fabsf(ns.y)) {   // CoordinateSystem written out: coordinate_system() here costs tile_kernel / tile_mw_kernel 16 B of scratch
        const float invLen = 1.f / sqrtf(ns.x * ns.x + ns.z * ns.z);
        ss = v3(-ns.z * invLen, 0.f, ns.x * invLen);
        ts = cross(ns, ss);
    } else {
        const float invLen = 1.f / sqrtf(ns.y * ns.y + ns.z * ns.z);
        ss = v3(0.f, ns.z * invLen, -ns.y * invLen);
        ts = cross(ns, ss);
    }
    r.dpdu = ss;
    r.nn = normalize(cross(ss, ts));
    if (flip) r.nn = r.nn * -1.f;
    return r;
}

// isect.dg.nn of a hit whose nn is the shading one: recomputed from the triangle where it is consumed (BSDF::f's side test, the radiance
// photon's normal) instead of being carried in the hit.  `tri` is the hit's own: the scene's index in a scene that is scanned linearly,
// the slot of the hierarchy's triangle array in a large one.  The very operations of the closest-hit routines (trianglemesh.cpp:163-181,
// core/diffgeom.cpp:46-54), so a triangle without vertex normals gets its nn back bit for bit.
__device__ __attribute__((noinline)) V3 geometric_normal(const DevScene &S, int tri) {
    V3 p1, p2, p3;
    bool flip;
    if (S.bvhNodes) {
        const float4 q1 = S.bvhTris[3 * tri], q2 = S.bvhTris[3 * tri + 1], q3 = S.bvhTris[3 * tri + 2];
        p1 = v3(q1.x, q1.y, q1.z); p2 = v3(q2.x, q2.y, q2.z); p3 = v3(q3.x, q3.y, q3.z);
        flip = __float_as_int(q3.w) != 0;
    } else {
        const DevTri &tr = S.tris[tri];
        p1 = v3(tr.p1[0], tr.p1[1], tr.p1[2]); p2 = v3(tr.p2[0], tr.p2[1], tr.p2[2]); p3 = v3(tr.p3[0], tr.p3[1], tr.p3[2]);
        flip = S.shootScene->triFlip[tri] != 0;
    }
    const float du1 = 0.f - 1.f, du2 = 1.f - 1.f, dv1 = 0.f - 1.f, dv2 = 0.f - 1.f;
    const V3 dp1 = p1 - p3, dp2 = p2 - p3;
    const float invdet = 1.f / (du1 * dv2 - dv1 * du2);
    const V3 dpdu = (dp1 * dv2 - dp2 * dv1) * invdet;
    const V3 dpdv = (dp1 * (-du2) + dp2 * du1) * invdet;
    const V3 nn = normalize(cross(dpdu, dpdv));
    return flip ? nn * -1.f : nn;
}
#endif
