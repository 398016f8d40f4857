// pvol_light_dev.h -- Light::Sample_L(p, eps, ...) of the three delta lights (distant.cpp:48-55, point.cpp:50-57, spot.cpp:50-57)
// and the shadow ray of its VisibilityTester (core/light.h:85-101), ONE text for every kernel that samples a light.
// Built with -ffp-contract=off: the operations and their order are the reference's, so every caller takes the cone's edge and the
// shadow ray's end on the same fp32 values.
#ifndef PVOL_LIGHT_DEV_H
#define PVOL_LIGHT_DEV_H
#include "pvol_dev.h"
#include "pvol_math.h"

// SpotLight::Falloff (spot.cpp:60-69) from cos(theta) of the direction in light space; 0 means L.IsBlack()
__device__ __forceinline__ float spot_falloff(float costheta, float cosTotalWidth, float cosFalloffStart) {
    if (costheta < cosTotalWidth) return 0.f;
    if (costheta > cosFalloffStart) return 1.f;
    const float delta = (costheta - cosTotalWidth) / (cosFalloffStart - cosTotalWidth);
    return delta * delta * delta * delta;
}
// z of Normalize(WorldToLight(w)); the rows of w2l lie PITCH floats apart (DevLight 4, the tile pre-pass's register copy 3)
template <int PITCH> __device__ __forceinline__ float spot_costheta(const float *w2l, V3 w) {
    return normalize(v3(w2l[0] * w.x + w2l[1] * w.y + w2l[2] * w.z,
                        w2l[PITCH] * w.x + w2l[PITCH + 1] * w.y + w2l[PITCH + 2] * w.z,
                        w2l[2 * PITCH] * w.x + w2l[2 * PITCH + 1] * w.y + w2l[2 * PITCH + 2] * w.z)).z;
}

struct LightSample {
    V3 wo;          // towards the light
    RayD vis;       // the shadow ray
    float d2;       // squared distance (1 for a distant light)
    float fall;     // cone falloff (1 unless spot)
    bool distant;
};
// The caller's own: L = I * fall / d2, the black test, the occlusion routine, what it does with a lit sample.
// mint: 0 inside the volume, the hit's epsilon at a surface.
__device__ __forceinline__ LightSample light_sample(const DevLight &light, V3 p, float mint) {
    LightSample r;
    r.d2 = 1.f;
    r.fall = 1.f;
    r.distant = light.kind == PVOL_LIGHT_DISTANT;
    if (r.distant) {
        r.wo = v3(light.dir[0], light.dir[1], light.dir[2]);
        r.vis.o = p; r.vis.d = r.wo; r.vis.mint = mint; r.vis.maxt = INFINITY;
    } else {
        const V3 lp = v3(light.pos[0], light.pos[1], light.pos[2]);
        r.wo = normalize(lp - p);
        const float dist = len(p - lp);   // of p - lp, the direction of lp - p: VisibilityTester::SetSegment
        r.vis.o = p; r.vis.d = vdiv(lp - p, dist); r.vis.mint = mint; r.vis.maxt = dist * (1.f - 0.f);
        r.d2 = len_sq(lp - p);
        if (light.kind == PVOL_LIGHT_SPOT)   // Falloff(-wi)
            r.fall = spot_falloff(spot_costheta<4>(light.w2l, -r.wo), light.cosTotalWidth, light.cosFalloffStart);
    }
    return r;
}
#endif
