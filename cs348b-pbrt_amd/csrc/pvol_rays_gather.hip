// pvol_rays_gather.hip -- the kernels pvol_radiance_gather_batch* adds to pvol_radiance_batch*'s slice walk (pvol_rays.hip):
// the final-gather branch of PhotonIntegrator::Li (integrators/photonmap.cpp:183-296) at every Lambertian hit of every member of the
// expanded array.  Between rays_emit_kernel and the volume batch
//     query: one member per lane repeats surf_closest as surface_kernel will, and writes the query pvol_final_gather_device answers
//            (a dead one, black kd, where the member has no Lambertian hit); every member gets a copy of its owner's sample rows
//     pvol_final_gather_device: Lg and the gather's draws per member
//     patch: rng_skip += draws, so the draws stand behind the hit's other surface draws and in front of the member's own volume Li()
// and behind surface_kernel
//     add:   Lv += T (.) Lg, the operation surface_kernel performed with Ls_matte; a stashed primary's row (0, 1) is left with
//            Ls_matte + Lg.
// A unit of its own on pvol_closest_dev.h, like pvol_final_gather.hip: the marching kernels are not recompiled.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pvol_math.h"
#include "pvol_closest_dev.h"
#include "pvol_host.h"

// One member per lane.  The hit is the one surface_kernel finds for this member: a segment's by `maxt >= mint && surf_closest`; a
// primary's too, once rays_patch_kernel has emptied the primaries that Scene::Intersect missed inside [mint, maxt] -- which runs after
// the volume batch, so the flag it goes by (SegInfo::pad[0]) is read here.
__global__ __launch_bounds__(LANES) void rays_gather_query_kernel(RaysGatherArgs A) {
    const uint32_t m = blockIdx.x * LANES + threadIdx.x;
    if (m >= A.total) return;
    const DevScene &S = *A.scene;
    const pvol_ray pr = A.rays[m];
    const SegInfo si = A.info[m];
    const bool owned = si.sample < A.n;   // always, unless the count and the emit pass disagreed and left a slot unwritten
    const bool primary = owned && m + 1u == A.offset[si.sample + 1u];
    const V3 o = v3(pr.o[0], pr.o[1], pr.o[2]), d = v3(pr.d[0], pr.d[1], pr.d[2]);
    Hit h;
    h.tri = 0; h.mat = 0; h.t = 0.f; h.rayEps = 0.f; h.p = h.nn = h.dpdu = v3(0.f, 0.f, 0.f);
    const bool hit = owned && (!primary || si.pad[0]) && pr.maxt >= pr.mint && surf_closest(S, o, d, pr.mint, &h);
    const DevMaterial &mat = S.shootScene->mats[h.mat];
    const bool lambert = hit && mat.kind == PVOL_MATERIAL_MATTE && mat.nBxdf > 0;   // MatteMaterial::GetBSDF: a Lambertian only for a non-black Kd
    // a dead query still goes through the lookup: a finite point and a unit frame, and a black kd, which is what kills it
    V3 p = v3(0.f, 0.f, 0.f), nn = v3(0.f, 0.f, 1.f), dpdu = v3(1.f, 0.f, 0.f), ng = nn, wo = nn;
    float eps = 0.f;
    if (lambert) { p = h.p; nn = h.nn; dpdu = h.dpdu; ng = hit_ng(S, h); wo = -d; eps = h.rayEps; }
    float *qp = A.p + 3 * (size_t)m, *qf = A.frames + 9 * (size_t)m, *qw = A.wo + 3 * (size_t)m, *qk = A.kd + 30 * (size_t)m;
    qp[0] = p.x; qp[1] = p.y; qp[2] = p.z;
    qf[0] = nn.x; qf[1] = nn.y; qf[2] = nn.z; qf[3] = dpdu.x; qf[4] = dpdu.y; qf[5] = dpdu.z; qf[6] = ng.x; qf[7] = ng.y; qf[8] = ng.z;
    qw[0] = wo.x; qw[1] = wo.y; qw[2] = wo.z;
    for (int b = 0; b < 30; ++b) qk[b] = lambert ? mat.kd[b] : 0.f;
    A.rayEps[m] = eps;
}

// One float per thread: member m's rows are its owner's, Sample being shared down the recursion (core/integrator.cpp:198, :243)
__global__ __launch_bounds__(256) void rays_gather_rows_kernel(RaysGatherArgs A) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t per = 3u * (uint32_t)A.nSamples;
    if (k >= (size_t)A.total * per) return;
    const uint32_t m = (uint32_t)(k / per), r = (uint32_t)(k % per);
    const uint32_t owner = A.info[m].sample;
    const size_t src = (size_t)(owner < A.n ? owner : 0u) * per + r;
    A.mUBsdf[k] = A.uBsdf[src];
    A.mUPhoton[k] = A.uPhoton[src];
}

__global__ __launch_bounds__(256) void rays_gather_patch_kernel(RaysGatherArgs A) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m < A.total) A.rays[m].rng_skip += A.gDraws[m];
}

// per caller ray: the gather's draws over its block
__global__ __launch_bounds__(256) void rays_gather_draws_kernel(RaysGatherArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    uint32_t g = 0u;
    for (uint32_t m = A.offset[i]; m < A.offset[i + 1u]; ++m) g += A.gDraws[m];
    A.gatherDraws[i] = g;
}

// Lane = bin, two members per wave (lanes 0..29 and 32..61).  A member without a gather keeps its bytes: nothing is added to it.
__global__ __launch_bounds__(256) void rays_gather_add_kernel(RaysGatherArgs A) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t m = k >> 5;
    const uint32_t b = (uint32_t)(k & 31u);
    if (m >= A.total || b >= 30u) return;
    const float lg = A.Lg[30 * m + b];
    float *row = A.rows + 60 * m;
    if (lg != 0.f) row[b] += row[30u + b] * lg;
}

extern "C" hipError_t pvol_launch_rays_gather_query(const RaysGatherArgs *a, hipStream_t stream) {
    const size_t floats = (size_t)a->total * 3u * (size_t)a->nSamples;
    hipLaunchKernelGGL(rays_gather_query_kernel, dim3((a->total + LANES - 1) / LANES), dim3(LANES), 0, stream, *a);
    hipLaunchKernelGGL(rays_gather_rows_kernel, dim3((unsigned)((floats + 255u) / 256u)), dim3(256), 0, stream, *a);
    return hipGetLastError();
}
extern "C" hipError_t pvol_launch_rays_gather_patch(const RaysGatherArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(rays_gather_patch_kernel, dim3((a->total + 255u) / 256u), dim3(256), 0, stream, *a);
    if (a->gatherDraws) hipLaunchKernelGGL(rays_gather_draws_kernel, dim3((a->n + 255u) / 256u), dim3(256), 0, stream, *a);
    return hipGetLastError();
}
extern "C" hipError_t pvol_launch_rays_gather_add(const RaysGatherArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(rays_gather_add_kernel, dim3((unsigned)(((size_t)a->total * 32u + 255u) / 256u)), dim3(256), 0, stream, *a);
    return hipGetLastError();
}
