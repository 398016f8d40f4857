// pvol_bsdf_dev.h -- included after pvol_math.h by the shooter (pvol_shoot.hip) and by everything behind the camera (pvol_spec_dev.h
// through pvol_shading_dev.h, pvol_gather.hip): the reflection primitives both sides share, in the reference's operation order.
#ifndef PVOL_BSDF_DEV_H
#define PVOL_BSDF_DEV_H

// CoordinateSystem, core/geometry.h:508-518
__device__ __forceinline__ void coordinate_system(V3 v, V3 *v1, V3 *v2) {
    if (fabsf(v.x) > fabsf(v.y)) {
        const float invLen = 1.f / sqrtf(v.x * v.x + v.z * v.z);
        *v1 = v3(-v.z * invLen, 0.f, v.x * invLen);
    } else {
        const float invLen = 1.f / sqrtf(v.y * v.y + v.z * v.z);
        *v1 = v3(0.f, v.z * invLen, -v.y * invLen);
    }
    *v2 = cross(v, *v1);
}

// The BSDF's frame (BSDF::BSDF, core/reflection.cpp:619-627; WorldToLocal / LocalToWorld, core/reflection.h:431-440)
struct BsdfFrame { V3 sn, tn, nn; };
__device__ __forceinline__ BsdfFrame bsdf_frame(V3 nn, V3 dpdu) {
    BsdfFrame f;
    f.nn = nn;
    f.sn = normalize(dpdu);
    f.tn = cross(nn, f.sn);
    return f;
}
__device__ __forceinline__ V3 to_local(const BsdfFrame &f, V3 v) { return v3(dot(v, f.sn), dot(v, f.tn), dot(v, f.nn)); }
__device__ __forceinline__ V3 to_world(const BsdfFrame &f, V3 v) {
    return v3(f.sn.x * v.x + f.tn.x * v.y + f.nn.x * v.z, f.sn.y * v.x + f.tn.y * v.y + f.nn.y * v.z, f.sn.z * v.x + f.tn.z * v.y + f.nn.z * v.z);
}

// FresnelDielectric::Evaluate with scalar indices, core/reflection.cpp:60-67 + 115-135
__device__ __forceinline__ float fresnel_dielectric(float cosi, float eta_i, float eta_t) {
    cosi = cosi < -1.f ? -1.f : (cosi > 1.f ? 1.f : cosi);
    const bool entering = cosi > 0.f;
    float ei = eta_i, et = eta_t;
    if (!entering) { const float t = ei; ei = et; et = t; }
    const float sint = ei / et * sqrtf(fmaxf(0.f, 1.f - cosi * cosi));
    if (sint >= 1.f) return 1.f;
    const float cost = sqrtf(fmaxf(0.f, 1.f - sint * sint));
    const float ac = fabsf(cosi);
    const float Rparl = ((et * ac) - (ei * cost)) / ((et * ac) + (ei * cost));
    const float Rperp = ((ei * ac) - (et * cost)) / ((ei * ac) + (et * cost));
    return (Rparl * Rparl + Rperp * Rperp) / 2.f;
}

// cosf / sinf as the reference's C library gives them: correctly rounded.  The device's own are good to an ulp or two: not enough for
// the gather, where near the rim of the disk sqrt(1 - dx^2 - dy^2) turns one ulp of dx into 1e-3 of the pdf.
__device__ __forceinline__ float cos_rounded(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float sin_rounded(float x) { return (float)sin((double)x); }

// ConcentricSampleDisk, core/montecarlo.cpp:306-348.  ROUNDED: the gather's form; the shooter keeps the device's cosf / sinf.
template <bool ROUNDED> __device__ __forceinline__ void concentric_disk(float u0, float u1, float *dx, float *dy) {
    float r, theta;
    const float sx = 2 * u0 - 1, sy = 2 * u1 - 1;
    if (sx == 0.f && sy == 0.f) { *dx = 0.f; *dy = 0.f; return; }
    if (sx >= -sy) {
        if (sx > sy) { r = sx; if (sy > 0.f) theta = sy / r; else theta = 8.0f + sy / r; }
        else { r = sy; theta = 2.0f - sx / r; }
    } else {
        if (sx <= sy) { r = -sx; theta = 4.0f - sy / r; }
        else { r = -sy; theta = 6.0f + sx / r; }
    }
    theta *= K_PI / 4.f;
    *dx = r * (ROUNDED ? cos_rounded(theta) : cosf(theta));
    *dy = r * (ROUNDED ? sin_rounded(theta) : sinf(theta));
}
#endif
