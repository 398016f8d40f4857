// pvol_probe.hip -- a ray probe for the tests, not part of include/pvol.h: hands chosen rays to the device's own hit routines on the
// scene pvol_set_scene uploaded and reads the answers back.  The kernel computes nothing itself; it calls
//   mode 0  surf_closest    (pvol_closest_dev.h)  one ray per lane: the surface kernel, the tile pre-pass, the specular recursion
//   mode 1  lane_occluded   (pvol_closest_dev.h)  one ray per lane: the per-lane any-hit of the march and surface kernels
//   mode 2  scene_occluded  (pvol_closest_dev.h)  one ray per wave, a triangle per lane: the any-hit of the wave-per-ray march kernels
//   mode 3  scene_closest   (pvol_closest_dev.h)  one ray per wave, a triangle per lane: the photon shooter's closest hit, maxt = inf
// and stores what they return.
#include "pvol_host.h"
#include "pvol_math.h"
#include "pvol_closest_dev.h"

#define PROBE_FLOATS 11   // t, rayEps, p, nn, dpdu
#define PROBE_INTS 3      // hit flag, primitive (triangle index in upload order, -1 - i: sphere i), material

// the record of a closest hit (modes 0 and 3)
__device__ __forceinline__ void probe_store(const DevScene &S, const Hit &h, float *of, int32_t *oi) {
    of[0] = h.t; of[1] = h.rayEps;
    of[2] = h.p.x; of[3] = h.p.y; of[4] = h.p.z;
    of[5] = h.nn.x; of[6] = h.nn.y; of[7] = h.nn.z;
    of[8] = h.dpdu.x; of[9] = h.dpdu.y; of[10] = h.dpdu.z;
    oi[0] = 1;
    oi[1] = (h.tri >= 0 && S.bvhNodes) ? __float_as_int(S.bvhTris[3 * h.tri].w) : h.tri;   // a hierarchy slot back to the upload order
    oi[2] = h.mat;
}

__global__ __launch_bounds__(LANES) void probe_kernel(const DevScene *scene, const pvol_ray *rays, uint32_t n, int mode, float *out, int32_t *outi) {
    const DevScene &S = *scene;
    const int lane = threadIdx.x;
    if (mode >= 2) {   // one wave per ray: every lane holds the same ray
        const uint32_t i = blockIdx.x;
        if (i >= n) return;
        const pvol_ray &r = rays[i];
        RayD vis;
        vis.o = v3(r.o[0], r.o[1], r.o[2]); vis.d = v3(r.d[0], r.d[1], r.d[2]); vis.mint = r.mint; vis.maxt = r.maxt;
        if (mode == 2) {
            const bool hit = scene_occluded(S, vis, lane);
            if (lane == 0) outi[(size_t)PROBE_INTS * i] = hit ? 1 : 0;
            return;
        }
        Hit h;
        float maxt = INFINITY;
        if (!scene_closest(S, *S.shootScene, vis.o, vis.d, vis.mint, &maxt, &h, lane)) return;
        if (lane == 0) probe_store(S, h, out + (size_t)PROBE_FLOATS * i, outi + (size_t)PROBE_INTS * i);
        return;
    }
    const uint32_t i = blockIdx.x * LANES + lane;
    if (i >= n) return;
    const pvol_ray &r = rays[i];
    const V3 o = v3(r.o[0], r.o[1], r.o[2]), d = v3(r.d[0], r.d[1], r.d[2]);
    int32_t *oi = outi + (size_t)PROBE_INTS * i;
    if (mode == 1) {
        RayD vis;
        vis.o = o; vis.d = d; vis.mint = r.mint; vis.maxt = r.maxt;
        oi[0] = lane_occluded(S, vis) ? 1 : 0;
        return;
    }
    Hit h;
    if (!surf_closest(S, o, d, r.mint, &h)) return;   // the buffers were zeroed: a miss stays all zero
    probe_store(S, h, out + (size_t)PROBE_FLOATS * i, oi);
}

// rays: n host pvol_ray (o, mint, d, maxt are read; the closest-hit modes 0 and 3 ignore maxt); out: n x 11 floats, outi: n x 3
// ints, both host.  Synchronous.  PVOL_E_INVALID, with nothing launched, for a null pointer, no scene, n == 0 or an unknown mode.
extern "C" int pvol_probe_hits(pvol_ctx *c, const pvol_ray *rays, uint32_t n, int mode, float *out, int32_t *outi) {
    if (!c || !rays || !out || !outi || n == 0 || mode < 0 || mode > 3) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->haveScene) return PVOL_E_INVALID;
    if (hipSetDevice(c->params.device) != hipSuccess) return PVOL_E_NO_DEVICE;
    DevPtr<pvol_ray> dRays;
    DevPtr<float> dOut;
    DevPtr<int32_t> dOutI;
    if (!dRays.alloc(n) || !dOut.alloc((size_t)PROBE_FLOATS * n) || !dOutI.alloc((size_t)PROBE_INTS * n)) return PVOL_E_NO_MEMORY;
    bool good = hipDeviceSynchronize() == hipSuccess &&
                hipMemcpy(dRays.get(), rays, sizeof(pvol_ray) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess &&
                hipMemset(dOut.get(), 0, sizeof(float) * PROBE_FLOATS * (size_t)n) == hipSuccess &&
                hipMemset(dOutI.get(), 0, sizeof(int32_t) * PROBE_INTS * (size_t)n) == hipSuccess;
    if (good) {
        const uint32_t blocks = mode >= 2 ? n : (n + LANES - 1) / LANES;
        hipLaunchKernelGGL(probe_kernel, dim3(blocks), dim3(LANES), 0, 0, c->ds.get(), dRays.get(), n, mode, dOut.get(), dOutI.get());
        good = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
               hipMemcpy(out, dOut.get(), sizeof(float) * PROBE_FLOATS * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(outi, dOutI.get(), sizeof(int32_t) * PROBE_INTS * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
    }
    return good ? PVOL_OK : PVOL_E_NO_DEVICE;
}
