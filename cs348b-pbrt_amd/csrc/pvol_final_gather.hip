// pvol_final_gather.hip -- the tracing half of the final gather: what PhotonIntegrator::Li does with every gather ray of both
// loops from the construction of bounceRay to `L += Li / gatherSamples` (integrators/photonmap.cpp:219-231, :243-246, :265-278,
// :291-295).  The direction records come from gather_lookup_kernel<true> (pvol_gather.hip) through pvol_gather_directions_device,
// so they are the bytes that entry point returns; this unit traces them (trace kernel, one gather ray per lane), looks the
// radiance photon up with the walk pvol_radiance_lookup uses (pvol_radwalk_dev.h) and sums (sum kernel, lane = bin).  Nothing here
// is wired into surface_kernel yet.  No atomics: two runs agree bit for bit, and a query's result does not depend on
// which other queries share the call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>

#include "pvol_math.h"
#include "pvol_closest_dev.h"
#include "pvol_radwalk_dev.h"
#include "pvol_host.h"

#define FG_NONE 0xffffffffu
#define FG_RAY_SCRATCH 64u                /* bytes per gather ray: its pvol_gather_sample and its pvol_gather_ray */

static_assert(sizeof(pvol_gather_ray) == 32 && sizeof(pvol_gather_sample) == 32, "one record is two float4");

// One slice of queries.  Passed by value: nothing in it is indexed at run time but the grid's three-element arrays inside loops of
// three, which unroll; what is indexed by lane (sigma_a, sigma_s) is read from the scene in device memory.
struct FgArgs {
    const DevScene *scene;
    RadWalk walk;
    const float *radLo;                        // [radiance photons][30] in input order
    const float *p, *kd, *rayEps;              // [count][3], [count][30], [count]
    uint32_t count;
    int32_t nSamples;
    const pvol_gather_sample *dirB, *dirP;     // [count][nSamples]
    pvol_gather_ray *rayB, *rayP;              // [count][nSamples]
    float *L;                                  // [count][30]
    uint32_t *draws;                           // [count]
};

__device__ __forceinline__ void put_ray(pvol_gather_ray *o, float t, V3 n, uint32_t index, int32_t prim, uint32_t hit, uint32_t drew) {
    float4 *o4 = reinterpret_cast<float4 *>(o);
    o4[0] = make_float4(t, n.x, n.y, n.z);
    o4[1] = make_float4(__uint_as_float(index), __int_as_float(prim), __uint_as_float(hit), __uint_as_float(drew));
}

// One gather ray per lane; the 2 nSamples rays of a query are neighbours (the BSDF loop's, then the photon loop's), so a wave's
// rays leave from a few points.  photonmap.cpp:219-230 / :265-277: Intersect, nGather, the radiance lookup; the Transmittance's
// draw is counted here and its value left to the sum.
__global__ __launch_bounds__(LANES) void final_gather_trace_kernel(FgArgs A) {
    const size_t r = (size_t)blockIdx.x * LANES + threadIdx.x;
    const uint32_t perQuery = 2u * (uint32_t)A.nSamples;
    if (r >= (size_t)A.count * perQuery) return;
    const uint32_t q = (uint32_t)(r / perQuery), rem = (uint32_t)(r % perQuery);
    const bool photonLoop = rem >= (uint32_t)A.nSamples;
    const size_t slot = (size_t)q * A.nSamples + (photonLoop ? rem - (uint32_t)A.nSamples : rem);
    pvol_gather_ray *out = (photonLoop ? A.rayP : A.rayB) + slot;
    const float4 *d4 = reinterpret_cast<const float4 *>((photonLoop ? A.dirP : A.dirB) + slot);
    bool live = __float_as_uint(d4[1].w) == 1u;   // pvol_gather_sample::valid; a query that found fewer than 50 has none
    if (live) {                                   // fr.IsBlack(): the Lambertian of a black Kd reflects nothing
        live = false;
        for (int b = 0; b < 30 && !live; ++b) live = A.kd[30 * (size_t)q + b] != 0.f;
    }
    if (!live) { put_ray(out, 0.f, v3(0.f, 0.f, 0.f), 0u, 0, 0u, 0u); return; }
    const DevScene &S = *A.scene;
    const float4 d0 = d4[0];
    const V3 o = v3(A.p[3 * (size_t)q], A.p[3 * (size_t)q + 1], A.p[3 * (size_t)q + 2]), wi = v3(d0.x, d0.y, d0.z);
    Hit h;
    if (!surf_closest(S, o, wi, A.rayEps[q], &h)) { put_ray(out, 0.f, v3(0.f, 0.f, 0.f), FG_NONE, 0, 0u, 0u); return; }
    // Faceforward(gatherIsect.dg.nn, -bounceRay.d) (geometry.h:520-522) with the geometric normal
    V3 n = hit_ng(S, h);
    if (dot(n, -wi) < 0.f) n = -n;
    const float hp[3] = {h.p.x, h.p.y, h.p.z};
    const int64_t j = radiance_nearest(A.walk, hp, n.x, n.y, n.z);
    const uint32_t index = j >= 0 ? __float_as_uint(A.walk.g.pos4[j].w) : FG_NONE;
    const int32_t prim = (h.tri >= 0 && S.bvhNodes) ? __float_as_int(S.bvhTris[3 * h.tri].w) : h.tri;   // as the probe reports it
    // renderer->Transmittance(scene, bounceRay, NULL, rng, arena): one RandomFloat when there is a volume region (photonvolume.cpp:15-30)
    put_ray(out, h.t, n, index, prim, 1u, S.volKind != PVOL_VOLUME_NONE ? 1u : 0u);
}

// Lane = bin; two queries per wave in lanes 0..29 and 32..61 (the radiance_lo_kernel pattern), eight per block.  Walks the query's
// 2 nSamples records in the reference's order: Li += fr * (Lo * T) * weight per sample, L += Li / gatherSamples per loop.
__global__ __launch_bounds__(256) void final_gather_sum_kernel(FgArgs A) {
    const uint32_t q = blockIdx.x * 8u + (threadIdx.x >> 5);
    const int bin = threadIdx.x & 31;
    if (q >= A.count) return;
    const DevScene &S = *A.scene;
    const bool mine = bin < 30;
    const float fr = mine ? A.kd[30 * (size_t)q + bin] * K_INV_PI : 0.f;   // Lambertian::f, reflection.cpp:304-306
    const bool medium = S.volKind != PVOL_VOLUME_NONE;
    const float sigT = (mine && medium) ? S.sigA[bin] + S.sigS[bin] : 0.f;
    const V3 o = v3(A.p[3 * (size_t)q], A.p[3 * (size_t)q + 1], A.p[3 * (size_t)q + 2]);
    const float eps = A.rayEps[q];
    const int nS = A.nSamples;
    float L = 0.f, Li = 0.f;
    uint32_t drawn = 0u;
    for (int r = 0; r < 2 * nS; ++r) {
        const size_t slot = (size_t)q * nS + (r < nS ? r : r - nS);
        const float4 *ray4 = reinterpret_cast<const float4 *>((r < nS ? A.rayB : A.rayP) + slot);
        const float4 r1 = ray4[1];
        if (__float_as_uint(r1.z) != 0u) {   // hit
            drawn += __float_as_uint(r1.w);
            const uint32_t index = __float_as_uint(r1.x);
            if (index != FG_NONE) {
                const float4 d0 = reinterpret_cast<const float4 *>((r < nS ? A.dirB : A.dirP) + slot)[0];   // wi, weight
                float Lindir = mine ? A.radLo[30 * (size_t)index + bin] : 0.f;
                if (medium) {   // HomogeneousVolumeDensity::tau (homogeneous.h:78-82) over [ray_eps, t_hit]
                    RayD ray;
                    ray.o = o; ray.d = v3(d0.x, d0.y, d0.z); ray.mint = eps; ray.maxt = ray4[0].x;
                    float t0, t1, length = 0.f;
                    if (vol_intersect(S, ray, &t0, &t1)) length = len((ray.o + ray.d * t0) - (ray.o + ray.d * t1));
                    Lindir *= expf(-(sigT * length));
                }
                Li += (fr * Lindir) * d0.w;
            }
        }
        if (r == nS - 1 || r == 2 * nS - 1) { L += Li / (float)nS; Li = 0.f; }
    }
    if (mine) A.L[30 * (size_t)q + bin] = L;
    if (bin == 0) A.draws[q] = drawn;
}

extern "C" {

int pvol_check_final_gather(int haveCtx, const FinalGatherCheck *a, int haveScene, int volKind, int haveGather, int haveRad, uint32_t radN) {
    if (!haveCtx || !a) return PVOL_E_INVALID;
    // the argument faults of pvol_gather_directions (pvol_check_gather, what 3), restated: that function's order puts its own
    // "no gather map" directly behind them, which here comes after the scene and the medium
    if (!(a->maxDist > 0.f) || !std::isfinite(a->maxDist) || !(a->maxDist * a->maxDist > 0.f)) return PVOL_E_INVALID;
    if (a->nSamples < 1 || a->nSamples > 256) return PVOL_E_INVALID;
    if (!(a->cosGatherAngle > -1.f && a->cosGatherAngle < 1.f)) return PVOL_E_INVALID;
    if (a->count && (!a->p || !a->frames || !a->wo || !a->uBsdf || !a->uPhoton)) return PVOL_E_INVALID;
    if (a->count && (!a->kd || !a->rayEps || !a->L || !a->draws)) return PVOL_E_INVALID;
    if (!haveScene) return PVOL_E_NO_SCENE;
    if (is_density_region(volKind)) return PVOL_E_UNSUPPORTED;
    if (!haveGather) return PVOL_E_INVALID;
    if (!haveRad || !radN) return PVOL_E_INVALID;
    return PVOL_OK;
}

uint32_t pvol_final_gather_slice(int32_t nSamples, uint64_t bound) {
    // the header's bound is the largest: a slice then holds at most 2^22 gather rays, so ray and block numbers fit 32 bits
    return pvol_slice_items(bound, PVOL_FINAL_GATHER_SCRATCH_BYTES, 2ull * FG_RAY_SCRATCH * (uint64_t)std::max(nSamples, 1));
}

int pvol_final_gather_set_scratch_bound(pvol_ctx *c, uint64_t bytes) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    c->fg.bound = std::min<uint64_t>(bytes, PVOL_FINAL_GATHER_SCRATCH_BYTES);   // the hook only lowers the bound
    return PVOL_OK;
}

static int check_ctx(const pvol_ctx *c, const FinalGatherCheck *a) {
    return pvol_check_final_gather(c != 0, a, c && c->haveScene, c ? c->hs.volKind : 0, c && c->gather.have, c && c->rad.have, c ? c->rad.n : 0u);
}

int pvol_final_gather_device(pvol_ctx *c, const float *dP, const float *dFrames, const float *dWo, const float *dKd, const float *dRayEps, uint32_t count,
                             float maxDist, int32_t nSamples, float cosGatherAngle, const float *dUBsdf, const float *dUPhoton, float *dL,
                             uint32_t *dDraws, pvol_gather_ray *dRaysBsdf, pvol_gather_ray *dRaysPhoton, void *hipStream) {
    const FinalGatherCheck a = {dP, dFrames, dWo, dKd, dRayEps, count, maxDist, nSamples, cosGatherAngle, dUBsdf, dUPhoton, dL, dDraws};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // the context's state is read under the lock only
    const int rc0 = check_ctx(c, &a);
    if (rc0 != PVOL_OK) return rc0;
    int rc = PVOL_OK;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipStream_t stream = (hipStream_t)hipStream;
    const uint32_t slice = std::min(count, pvol_final_gather_slice(nSamples, c->fg.bound));
    const size_t sliceRecs = (size_t)slice * nSamples;   // records of one loop
    const bool ownRays = !dRaysBsdf || !dRaysPhoton;
    // an earlier call's kernels, on whatever stream, may still read the slices' scratch
    if (!c->fg.fence.wait(stream)) return PVOL_E_NO_DEVICE;
    if (!pvol_reserve(c->buf[PVOL_BUF_FG_DIRS], 2 * sliceRecs * sizeof(pvol_gather_sample), stream) ||
        (ownRays && !pvol_reserve(c->buf[PVOL_BUF_FG_RAYS], 2 * sliceRecs * sizeof(pvol_gather_ray), stream)))
        return PVOL_E_NO_MEMORY;
    pvol_gather_sample *dirs = pvol_buf<pvol_gather_sample>(c, PVOL_BUF_FG_DIRS);
    pvol_gather_ray *rays = pvol_buf<pvol_gather_ray>(c, PVOL_BUF_FG_RAYS);
    FgArgs A;
    memset(&A, 0, sizeof(A));
    A.scene = c->ds.get();
    A.walk = pvol_radiance_walk(c);
    A.radLo = c->rad.lo.get();
    A.nSamples = nSamples;
    // the slices follow one another on the stream, so each may reuse the scratch of the one before
    for (uint32_t q0 = 0; q0 < count; q0 += slice) {
        const uint32_t n = std::min(slice, count - q0);
        const size_t recs = (size_t)n * nSamples, first = (size_t)q0 * nSamples;
        pvol_gather_sample *dirB = dirs, *dirP = dirs + recs;
        rc = pvol_gather_directions_device(c, dP + 3 * (size_t)q0, dFrames + 9 * (size_t)q0, dWo + 3 * (size_t)q0, n, maxDist, nSamples, cosGatherAngle,
                                           dUBsdf + 3 * first, dUPhoton + 3 * first, dirB, dirP, hipStream);
        if (rc != PVOL_OK) return rc;
        A.p = dP + 3 * (size_t)q0; A.kd = dKd + 30 * (size_t)q0; A.rayEps = dRayEps + q0;
        A.count = n;
        A.dirB = dirB; A.dirP = dirP;
        A.rayB = dRaysBsdf ? dRaysBsdf + first : rays;
        A.rayP = dRaysPhoton ? dRaysPhoton + first : rays + recs;
        A.L = dL + 30 * (size_t)q0; A.draws = dDraws + q0;
        const size_t nRays = 2 * recs;
        hipLaunchKernelGGL(final_gather_trace_kernel, dim3((unsigned)((nRays + LANES - 1) / LANES)), dim3(LANES), 0, stream, A);
        if (!ok(hipGetLastError())) return PVOL_E_NO_DEVICE;
        hipLaunchKernelGGL(final_gather_sum_kernel, dim3((n + 7) / 8), dim3(256), 0, stream, A);
        if (!ok(hipGetLastError())) return PVOL_E_NO_DEVICE;
    }
    return c->fg.fence.record(stream) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

int pvol_final_gather(pvol_ctx *c, const float *p, const float *frames, const float *wo, const float *kd, const float *rayEps, uint32_t count,
                      float maxDist, int32_t nSamples, float cosGatherAngle, const float *uBsdf, const float *uPhoton, float *L, uint32_t *draws,
                      pvol_gather_ray *raysBsdf, pvol_gather_ray *raysPhoton) {
    const FinalGatherCheck a = {p, frames, wo, kd, rayEps, count, maxDist, nSamples, cosGatherAngle, uBsdf, uPhoton, L, draws};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    int rc = check_ctx(c, &a);
    if (rc != PVOL_OK) return rc;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const size_t n = count, nO = n * nSamples, nU = 3 * nO;
    HostStage st;
    const float *dP = st.in(p, 3 * n), *dFrames = st.in(frames, 9 * n), *dWo = st.in(wo, 3 * n), *dKd = st.in(kd, 30 * n), *dEps = st.in(rayEps, n);
    const float *dUB = st.in(uBsdf, nU), *dUP = st.in(uPhoton, nU);
    float *dL = st.out(L, 30 * n);
    uint32_t *dDraws = st.out(draws, n);
    pvol_gather_ray *dRB = st.out(raysBsdf, nO), *dRP = st.out(raysPhoton, nO);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = pvol_final_gather_device(c, dP, dFrames, dWo, dKd, dEps, count, maxDist, nSamples, cosGatherAngle, dUB, dUP, dL, dDraws, dRB, dRP, 0);
    if (rc != PVOL_OK) return rc;
    if (!ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;   // nothing is written unless all of it ran
    return st.download();
}

}  // extern "C"
