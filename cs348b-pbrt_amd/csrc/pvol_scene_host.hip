// pvol_scene_host.hip -- pvol_set_scene in three steps: the scene's device image, a pure function of the
// arguments (pvol_scene_image: every check and all host arithmetic, no HIP call, no context); the upload of what only a device
// can hold (the triangle hierarchy, the density grid) into owners; the commit, the only step that touches the context.  Host code
// only: this unit defines no kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include "pvol_host.h"

static bool finite_f(float x) { return x == x && fabsf(x) != INFINITY; }

// ---- host evaluation of the light-power CDF (ComputeLightSamplingCDF core/integrator.cpp:261-268,
// Distribution1D montecarlo.h:56-76), fp32 in the reference's order (this file is built with
// -ffp-contract=off)
static float host_spec_y(const pvol_scene *s, const float *c30) {
    float yy = 0.f;
    for (int i = 0; i < 30; ++i) yy += s->cie_y.c[i] * c30[i];
    return yy * float(700 - 400) / float(106.856895f * 30);
}
static void world_sphere(const pvol_scene *s, float c[3], float *rad) {   // BBox::BoundingSphere, core/geometry.cpp:60-63
    bool inside = true;
    for (int a = 0; a < 3; ++a) {
        c[a] = .5f * s->world_min[a] + .5f * s->world_max[a];
        inside = inside && c[a] >= s->world_min[a] && c[a] <= s->world_max[a];
    }
    float dx = c[0] - s->world_max[0], dy = c[1] - s->world_max[1], dz = c[2] - s->world_max[2];
    *rad = inside ? sqrtf(dx * dx + dy * dy + dz * dz) : 0.f;
}
static const float kPiF = 3.14159265358979323846f;
static float light_power_y(const pvol_scene *s, const pvol_light &l, float worldRadius) {
    float p[30];
    for (int i = 0; i < 30; ++i) {
        float I = l.intensity.c[i];
        if (l.kind == PVOL_LIGHT_SPOT) p[i] = I * 2.f * kPiF * (1.f - .5f * (l.cos_falloff_start + l.cos_total_width));   // spot.cpp:72-75
        else if (l.kind == PVOL_LIGHT_POINT) p[i] = I * (4.f * kPiF);                                                      // point.cpp:60-62
        else p[i] = I * kPiF * worldRadius * worldRadius;                                                                  // distant.cpp:58-63
    }
    return host_spec_y(s, p);
}

static int fill_shoot_scene(const pvol_params &params, const pvol_scene *s, DevShootScene &H) {
    memset(&H, 0, sizeof(H));
    if (s->n_materials > PVOL_MAX_MATERIALS) return PVOL_E_UNSUPPORTED;
    if (s->n_materials && !s->materials) return PVOL_E_INVALID;
    H.nMats = (int)s->n_materials;
    for (uint32_t i = 0; i < s->n_materials; ++i) {
        const pvol_material &m = s->materials[i];
        if (m.kind != PVOL_MATERIAL_MATTE && m.kind != PVOL_MATERIAL_GLASS) return PVOL_E_UNSUPPORTED;
        DevMaterial &d = H.mats[i];
        d.kind = m.kind; d.ior = m.ior; d.vn = m.vn; d.nBxdf = 0;
        bool kdBlack = true, krBlack = true, ktBlack = true;
        for (int b = 0; b < 30; ++b) {
            d.kd[b] = m.kd.c[b]; d.kr[b] = m.kr.c[b]; d.kt[b] = m.kt.c[b];
            kdBlack = kdBlack && m.kd.c[b] == 0.f; krBlack = krBlack && m.kr.c[b] == 0.f; ktBlack = ktBlack && m.kt.c[b] == 0.f;
        }
        if (m.kind == PVOL_MATERIAL_MATTE) { if (!kdBlack) d.bxdfType[d.nBxdf++] = 1 | 4; }          // Lambertian
        else { if (!krBlack) d.bxdfType[d.nBxdf++] = 1 | 16; if (!ktBlack) d.bxdfType[d.nBxdf++] = 2 | 16; }
    }
    for (uint32_t i = 0; i < s->n_triangles; ++i) {
        int mi = s->triangles[i].material;
        if (mi < 0 || (uint32_t)mi >= std::max(1u, s->n_materials)) return PVOL_E_INVALID;
        if (s->n_triangles <= PVOL_MAX_TRIS) {   // a larger scene keeps both in its hierarchy's leaves (pvol_bvh.hip)
            H.triMat[i] = mi;
            H.triFlip[i] = s->triangles[i].flip_normal;
        }
    }
    world_sphere(s, H.worldCenter, &H.worldRadius);
    int n = (int)s->n_lights;
    for (int i = 0; i < n; ++i) {
        memcpy(H.l2w[i], s->lights[i].light_to_world, sizeof(float) * 12);
        H.lightFunc[i] = light_power_y(s, s->lights[i], H.worldRadius);
    }
    if (n > 0) {
        H.lightCdf[0] = 0.f;
        for (int i = 1; i < n + 1; ++i) H.lightCdf[i] = H.lightCdf[i - 1] + H.lightFunc[i - 1] / n;
        H.lightFuncInt = H.lightCdf[n];
        if (H.lightFuncInt == 0.f) { for (int i = 1; i < n + 1; ++i) H.lightCdf[i] = float(i) / float(n); }
        else { for (int i = 1; i < n + 1; ++i) H.lightCdf[i] /= H.lightFuncInt; }
    }
    H.shooterStep = params.shooter_step_size;
    H.maxPhotonDepth = params.max_photon_depth;
    H.finalGather = params.final_gather;
    H.nCausticWanted = params.n_caustic_photons;
    H.nIndirectWanted = params.n_indirect_photons;
    H.nVolumeWanted = params.n_volume_photons;
    return PVOL_OK;
}

static void pad32(float *dst, const pvol_spectrum &s) {
    for (int i = 0; i < 30; ++i) dst[i] = s.c[i];
    dst[30] = dst[31] = 0.f;
}

// the diagonal of a box that grows point by point, in double
struct Bounds {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void add(int a, float x) { lo[a] = std::min(lo[a], x); hi[a] = std::max(hi[a], x); }
    double diagonal() const {
        return sqrt((double)(hi[0] - lo[0]) * (hi[0] - lo[0]) + (double)(hi[1] - lo[1]) * (hi[1] - lo[1]) + (double)(hi[2] - lo[2]) * (hi[2] - lo[2]));
    }
};

extern "C" {

// Arguments of an exponential medium (pvol_volume.density = {a, b, updir}), checked without a device: every value finite, updir not
// of zero length.  up3 gets Normalize(updir) with the reference's operations (core/geometry.h:94-98, :507: the vector divided by
// its length, which Vector::operator/ does with one reciprocal and three products).
int pvol_check_exponential(const pvol_volume *v, float *up3) {
    if (!v || !v->density) return PVOL_E_INVALID;
    const float *e = v->density;
    for (int i = 0; i < 5; ++i) if (!finite_f(e[i])) return PVOL_E_INVALID;
    const float length = sqrtf(e[2] * e[2] + e[3] * e[3] + e[4] * e[4]);
    if (!(length > 0.f) || length == INFINITY) return PVOL_E_INVALID;
    const float inv = 1.f / length;
    if (up3) for (int i = 0; i < 3; ++i) up3[i] = e[2 + i] * inv;
    return PVOL_OK;
}

// a * expf(-b * height) is monotone in the height and the height is linear in the point: the maximum over the extent is at a corner
float pvol_exponential_max_density(const pvol_volume *v, const float *up3) {
    float md = 0.f;
    for (int k = 0; k < 8; ++k) {
        const float d[3] = {(k & 1) ? v->extent_max[0] - v->extent_min[0] : 0.f, (k & 2) ? v->extent_max[1] - v->extent_min[1] : 0.f,
                            (k & 4) ? v->extent_max[2] - v->extent_min[2] : 0.f};
        const float height = d[0] * up3[0] + d[1] * up3[1] + d[2] * up3[2];
        md = std::max(md, v->density[0] * expf(-v->density[1] * height));
    }
    return md;
}

int pvol_check_scene(const pvol_params *params, const pvol_scene *s) {
    SceneImage img;
    return pvol_scene_image(params, s, &img);
}

// Arguments of pvol_set_triangle_normals against a scene of sceneTris triangles, checked without a device: NULL with count 0 (clear)
// is fine; otherwise one row of nine finite floats per triangle of the scene.
static int check_triangle_normals(uint32_t sceneTris, const float *n, uint32_t nTriangles) {
    if (!n) return nTriangles == 0 ? PVOL_OK : PVOL_E_INVALID;
    if (nTriangles != sceneTris) return PVOL_E_INVALID;
    for (size_t i = 0, m = (size_t)nTriangles * 9; i < m; ++i) if (!finite_f(n[i])) return PVOL_E_INVALID;
    return PVOL_OK;
}
int pvol_check_triangle_normals(const pvol_scene *s, const float *n, uint32_t nTriangles) {
    if (!s) return PVOL_E_INVALID;
    return check_triangle_normals(s->n_triangles, n, nTriangles);
}

}  // extern "C"

// The order of the checks is part of the behaviour (a scene with several faults answers with the first): volume kind, counts,
// NULL arrays, spheres, grid dimensions, exponential arguments, light kinds, the step bound, materials, non-finite vertices.
int pvol_scene_image(const pvol_params *params, const pvol_scene *s, SceneImage *out) {
    if (!params || !s || !out) return PVOL_E_INVALID;
    const pvol_volume &v = s->volume;
    if (v.kind != PVOL_VOLUME_NONE && v.kind != PVOL_VOLUME_HOMOGENEOUS && v.kind != PVOL_VOLUME_GRID && v.kind != PVOL_VOLUME_RAINBOW &&
        v.kind != PVOL_VOLUME_EXPONENTIAL)
        return PVOL_E_UNSUPPORTED;
    if (s->n_lights > PVOL_MAX_LIGHTS || s->n_triangles > PVOL_BVH_MAX_TRIS) return PVOL_E_UNSUPPORTED;
    if ((s->n_lights && !s->lights) || (s->n_triangles && !s->triangles)) return PVOL_E_INVALID;
    if (s->n_spheres > PVOL_MAX_SPHERES) return PVOL_E_UNSUPPORTED;
    if (s->n_spheres && !s->spheres) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const pvol_sphere &sp = s->spheres[i];
        if (!(sp.radius > 0.f) || sp.material < 0 || (uint32_t)sp.material >= std::max(1u, s->n_materials)) return PVOL_E_INVALID;
    }
    if (v.kind == PVOL_VOLUME_GRID && (!v.density || v.nx < 1 || v.ny < 1 || v.nz < 1)) return PVOL_E_INVALID;
    float expUp[3] = {0.f, 0.f, 0.f};
    if (v.kind == PVOL_VOLUME_EXPONENTIAL && pvol_check_exponential(&v, expUp) != PVOL_OK) return PVOL_E_INVALID;
    // (a density that overflows somewhere in the extent is a non-finite value of the medium as well)
    if (v.kind == PVOL_VOLUME_EXPONENTIAL && pvol_exponential_max_density(&v, expUp) == INFINITY) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        const int k = s->lights[i].kind;
        if (k != PVOL_LIGHT_POINT && k != PVOL_LIGHT_SPOT && k != PVOL_LIGHT_DISTANT) return PVOL_E_UNSUPPORTED;
    }
    DevScene &h = out->scene;
    memset(&h, 0, sizeof(h));
    h.volKind = v.kind;
    for (int i = 0; i < 3; ++i) { h.extLo[i] = v.extent_min[i]; h.extHi[i] = v.extent_max[i]; }
    memcpy(h.w2v, v.world_to_volume, sizeof(h.w2v));
    pad32(h.sigA, v.sigma_a); pad32(h.sigS, v.sigma_s); pad32(h.le, v.le);
    h.g = v.g;
    h.nx = v.nx; h.ny = v.ny; h.nz = v.nz;
    out->maxDensity = 1.f;
    if (v.kind == PVOL_VOLUME_GRID) {
        float md = 0.f;
        for (size_t i = 0, n = (size_t)v.nx * v.ny * v.nz; i < n; ++i) md = std::max(md, v.density[i]);
        out->maxDensity = md;
    }
    if (v.kind == PVOL_VOLUME_EXPONENTIAL) {
        h.expA = v.density[0]; h.expB = v.density[1];
        for (int i = 0; i < 3; ++i) h.expUp[i] = expUp[i];
        out->maxDensity = pvol_exponential_max_density(&v, h.expUp);
    }
    h.nLights = (int)s->n_lights;
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        const pvol_light &l = s->lights[i];
        DevLight &d = h.lights[i];
        d.kind = l.kind;
        for (int k = 0; k < 3; ++k) { d.pos[k] = l.pos[k]; d.dir[k] = l.dir[k]; }
        memcpy(d.w2l, l.world_to_light, sizeof(float) * 12);
        d.cosTotalWidth = l.cos_total_width;
        d.cosFalloffStart = l.cos_falloff_start;
        pad32(d.intensity, l.intensity);
    }
    h.nSpheres = (int)s->n_spheres;
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const pvol_sphere &sp = s->spheres[i];
        DevSphere &d = h.spheres[i];
        memcpy(d.o2w, sp.object_to_world, sizeof(d.o2w));
        memcpy(d.w2o, sp.world_to_object, sizeof(d.w2o));
        d.radius = sp.radius; d.zmin = sp.z_min; d.zmax = sp.z_max; d.thetaMin = sp.theta_min; d.thetaMax = sp.theta_max; d.phiMax = sp.phi_max;
        d.mat = sp.material; d.flip = sp.flip_normal;
    }
    // more triangles than the embedded array: the hierarchy holds them (nTris 0, nBvhTris set by the upload)
    const bool big = s->n_triangles > PVOL_MAX_TRIS;
    h.nTris = big ? 0 : (int)s->n_triangles;
    for (uint32_t i = 0; i < s->n_triangles && !big; ++i) {
        const pvol_triangle &t = s->triangles[i];
        for (int k = 0; k < 3; ++k) { h.tris[i].p1[k] = t.p[0][k]; h.tris[i].p2[k] = t.p[1][k]; h.tris[i].p3[k] = t.p[2][k]; }
    }
    pad32(h.cieX, s->cie_x); pad32(h.cieY, s->cie_y); pad32(h.cieZ, s->cie_z);
    h.stepSize = params->step_size;
    h.maxDist = params->max_dist;
    h.maxDistSq = params->max_dist * params->max_dist;  // photonvolume.h:18
    h.nUsed = params->n_used;
    h.candCap = ((params->n_used + 63) / 64) * 64 + 192;
    // march-step bound: diagonal of the volume's world bound / stepSize (rays are clipped to the extent)
    // (every scene with a medium: a one-light homogeneous scene reaches the record plan too -- pvol_li with the caller's live
    // RNG state takes the RESOLVE + REPLAY path -- and with maxSteps 0 every such ray was reported as PVOL_E_LIMIT)
    if (v.kind != PVOL_VOLUME_NONE) {
        Bounds world;
        for (int k = 0; k < 8; ++k) {
            float x = (k & 1) ? v.extent_max[0] : v.extent_min[0], y = (k & 2) ? v.extent_max[1] : v.extent_min[1],
                  z = (k & 4) ? v.extent_max[2] : v.extent_min[2];
            const float *m = v.volume_to_world;
            float w[3] = {m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7], m[8] * x + m[9] * y + m[10] * z + m[11]};
            for (int a = 0; a < 3; ++a) world.add(a, w[a]);
        }
        double steps = world.diagonal() / params->step_size * 1.05 + 4;
        if (steps > 12000) return PVOL_E_LIMIT;
        h.maxSteps = ((int)steps + 63) & ~63;
    }
    int rc = fill_shoot_scene(*params, s, out->shoot);
    if (rc != PVOL_OK) return rc;
    std::vector<int32_t> mat(s->n_triangles);
    for (uint32_t i = 0; i < s->n_triangles; ++i) mat[i] = s->triangles[i].material;
    for (uint32_t i = 0; i < s->n_spheres; ++i) mat.push_back(s->spheres[i].material);   // the surface integrator's matte check covers them
    out->primMat.swap(mat);
    out->bvhPad = 0.f;
    if (big) {
        Bounds tris;
        for (uint32_t i = 0; i < s->n_triangles; ++i)
            for (int vi = 0; vi < 3; ++vi)
                for (int k = 0; k < 3; ++k) {
                    const float x = s->triangles[i].p[vi][k];
                    if (!finite_f(x)) return PVOL_E_INVALID;
                    tris.add(k, x);
                }
        out->bvhPad = (float)(1e-5 * tris.diagonal());
    }
    return PVOL_OK;
}

// The scene's triangles as a linear BVH on the device (pvol_bvh.hip); *ms: the build between two events.
static int upload_bvh(const pvol_scene *s, const SceneImage &img, DevPtr<float4> &tris, DevPtr<float4> &nodes, double *ms) {
    const uint32_t n = s->n_triangles;
    std::vector<float> tv((size_t)n * 9);
    std::vector<int32_t> fl(n);
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(&tv[(size_t)i * 9], s->triangles[i].p, sizeof(float) * 9);
        fl[i] = s->triangles[i].flip_normal;
    }
    DevPtr<float> dTri;
    DevPtr<int32_t> dMat, dFlip;
    bool good = dTri.alloc(tv.size()) && dMat.alloc(n) && dFlip.alloc(n) && tris.alloc((size_t)n * 3) && nodes.alloc((size_t)(n - 1) * 4) &&
                ok(hipMemcpy(dTri.get(), tv.data(), tv.size() * 4, hipMemcpyHostToDevice)) &&
                ok(hipMemcpy(dMat.get(), img.primMat.data(), (size_t)n * 4, hipMemcpyHostToDevice)) &&
                ok(hipMemcpy(dFlip.get(), fl.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    if (good) {
        DevEvent e0, e1;
        e0.create(true); e1.create(true);
        hipEventRecord(e0.get(), 0);
        good = ok(pvol_build_bvh(dTri.get(), dMat.get(), dFlip.get(), n, img.bvhPad, tris.get(), nodes.get(), 0));
        hipEventRecord(e1.get(), 0);
        hipEventSynchronize(e1.get());
        float t = 0.f;
        hipEventElapsedTime(&t, e0.get(), e1.get());
        *ms = t;
    }
    return good ? PVOL_OK : PVOL_E_NO_MEMORY;
}

extern "C" int pvol_set_scene(pvol_ctx *c, const pvol_scene *s) {
    if (!c || !s) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    // image: a rejected scene leaves the previous one, including its density grid, in place
    SceneImage img;
    int rc = pvol_scene_image(&c->params, s, &img);
    if (rc != PVOL_OK) return rc;
    // upload: into owners, which free what they hold on every way out
    DevPtr<float4> nodes, tris;
    DevPtr<float> density;
    double bvhMs = 0.0;
    const bool big = s->n_triangles > PVOL_MAX_TRIS;   // more triangles than the embedded array
    if (big && (rc = upload_bvh(s, img, tris, nodes, &bvhMs)) != PVOL_OK) return rc;
    if (s->volume.kind == PVOL_VOLUME_GRID) {
        const size_t n = (size_t)s->volume.nx * s->volume.ny * s->volume.nz;
        if (!density.alloc(n)) return PVOL_E_NO_MEMORY;
        if (!ok(hipMemcpy(density.get(), s->volume.density, sizeof(float) * n, hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
    }
    // commit: kernels of earlier batches may still read the old scene and grid
    DevScene &h = img.scene;
    h.density = density.get();
    h.bvhNodes = nodes.get(); h.bvhTris = tris.get(); h.nBvhTris = big ? (int)s->n_triangles : 0;
    h.shootScene = c->dsh.get();
    pvol_map_to_scene(c->volMap, h);   // the volume map stays; the surface integrator belongs to the scene it was enabled on (h.surf is zero)
    h.ringMax = c->hs.ringMax; h.rkEstimate = c->hs.rkEstimate;
    // the kept map's moment rows are a function of this scene's spectra: built aside, committed with the scene
    DevPtr<float> mom;
    int momTerms = 0;
    if ((rc = pvol_map_moments(c->volMap, h, mom, &momTerms)) != PVOL_OK) return rc;
    h.mom = mom.get();
    if (!ok(hipDeviceSynchronize()) || !ok(hipMemcpy(c->dsh.get(), &img.shoot, sizeof(img.shoot), hipMemcpyHostToDevice)) ||
        !ok(hipMemcpy(c->ds.get(), &h, sizeof(DevScene), hipMemcpyHostToDevice))) {
        pvol_push_scene(c);   // best effort: put the device copy of the previous scene back
        hipMemcpy(c->dsh.get(), &c->hsh, sizeof(c->hsh), hipMemcpyHostToDevice);
        return PVOL_E_NO_DEVICE;
    }
    c->dDensity = std::move(density);
    c->dBvhNodes = std::move(nodes); c->dBvhTris = std::move(tris);
    c->bvhBuildMs = bvhMs;
    c->volMap.mom = std::move(mom); c->momentTerms = momTerms;
    c->triMatHost.swap(img.primMat);
    c->maxDensity = img.maxDensity;
    pvol_free_caustic_map(c);
    c->dTriN.reset();   // vertex normals belong to the scene they were set on (h.triN is zero)
    c->nSceneTris = s->n_triangles;
    c->hs = h;
    c->hsh = img.shoot;
    c->haveScene = true;
    return PVOL_OK;
}

// Per-vertex shading normals of the scene's triangles (Triangle::GetShadingGeometry, shapes/trianglemesh.cpp:293-368): a side array
// in the scene's triangle order, which both closest-hit routines index by the hit's original triangle number (pvol_shading_dev.h).
extern "C" int pvol_set_triangle_normals(pvol_ctx *c, const float *n, uint32_t nTriangles) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    int rc = check_triangle_normals(c->nSceneTris, n, nTriangles);
    if (rc != PVOL_OK) return rc;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    DevPtr<float> dn;
    if (n && nTriangles) {
        if (!dn.alloc((size_t)nTriangles * 9)) return PVOL_E_NO_MEMORY;
        if (!ok(hipMemcpy(dn.get(), n, sizeof(float) * 9 * (size_t)nTriangles, hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
    }
    // commit: kernels of earlier batches may still read the old array.  Every check and the upload come first, so a rejected call
    // changes nothing; only a device copy that fails here is put back best effort (a second failure would leave the device copy of
    // the scene behind the host's, as in pvol_set_scene).
    if (!ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;
    const float *old = c->hs.triN;
    c->hs.triN = dn.get();
    if ((rc = pvol_push_scene(c)) != PVOL_OK) { c->hs.triN = old; pvol_push_scene(c); return rc; }
    c->dTriN = std::move(dn);
    return PVOL_OK;
}
