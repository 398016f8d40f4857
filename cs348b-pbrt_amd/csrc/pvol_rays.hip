// pvol_rays.hip -- the host side of pvol_radiance_batch*: SamplerRenderer::Li (renderers/samplerrenderer.cpp:228-251, :95-97) for rays
// the caller generated.  The kernels of the pre-pass and the fold are pvol_rays_dev.h's (compiled in pvol_march.hip,
// beside spec_surface and surface_kernel, which they use); this unit checks the call, walks the rays in slices, and per slice runs
//   count -> exclusive scan (hipCUB) -> emit + stream table -> pvol_launch_batch (the path pvol_li_batch_device takes, SPECTRAL)
//   -> patch + surface_kernel in its spectral mode (surface integrator on) -> compose.
// No atomics of its own; the block sizes are known before anything is written.
// pvol_radiance_gather_batch*  is the same walk with the final gather at every member's Lambertian hit: the queries
// (pvol_rays_gather.hip) and pvol_final_gather_device between emit and the volume batch, Lv += T (.) Lg behind surface_kernel.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include "pvol_host.h"

extern "C" {

int pvol_radiance_batch_check(int haveCtx, const RadianceBatchCheck *a, int haveScene, int volKind, int surfOn) {
    if (!haveCtx || !a) return PVOL_E_INVALID;
    if (a->outputKind != PVOL_OUT_SPECTRAL && a->outputKind != PVOL_OUT_XYZ) return PVOL_E_INVALID;
    if ((a->nRays && !a->rays) || (a->nStreams && !a->streams)) return PVOL_E_INVALID;
    if (a->nRays && (!a->out || !a->out->L)) return PVOL_E_INVALID;
    if (!haveScene) return PVOL_E_NO_SCENE;
    if (surfOn && is_density_region(volKind)) return PVOL_E_UNSUPPORTED;   // the shadow rays' tau() offsets are drawn values
    return PVOL_OK;
}

uint32_t pvol_radiance_max_segments(int specOn, int32_t maxSpecularDepth) {
    if (!specOn || maxSpecularDepth < 2) return 0u;
    return (1u << std::min<int32_t>(maxSpecularDepth, SPEC_MAX_DEPTH)) - 2u;
}

uint32_t pvol_radiance_slice(uint32_t maxSegments, uint64_t bound) {
    return pvol_slice_items(bound, PVOL_RADIANCE_SCRATCH_BYTES, ((uint64_t)maxSegments + 1u) * PVOL_RADIANCE_RAY_SCRATCH + PVOL_RADIANCE_CALLER_SCRATCH);
}

int pvol_radiance_gather_check(int haveCtx, const RadianceGatherCheck *a, int haveScene, int volKind, int surfOn, uint32_t indirectN, int haveGather,
                               int haveRad, uint32_t radN) {
    if (!haveCtx || !a) return PVOL_E_INVALID;
    if (a->outputKind != PVOL_OUT_SPECTRAL && a->outputKind != PVOL_OUT_XYZ) return PVOL_E_INVALID;
    if ((a->nRays && !a->rays) || (a->nStreams && !a->streams)) return PVOL_E_INVALID;
    if (a->nRays && (!a->out || !a->out->L)) return PVOL_E_INVALID;
    const pvol_gather_params *g = a->gather;
    if (!g) return PVOL_E_INVALID;
    // the argument faults of pvol_gather_directions, as pvol_check_final_gather restates them
    if (!(g->max_dist > 0.f) || !std::isfinite(g->max_dist) || !(g->max_dist * g->max_dist > 0.f)) return PVOL_E_INVALID;
    if (g->n_samples < 1 || g->n_samples > 256) return PVOL_E_INVALID;
    if (!(g->cos_gather_angle > -1.f && g->cos_gather_angle < 1.f)) return PVOL_E_INVALID;
    if (a->nRays && (!g->u_bsdf || !g->u_photon)) return PVOL_E_INVALID;
    if (!haveScene) return PVOL_E_NO_SCENE;
    if (is_density_region(volKind)) return PVOL_E_UNSUPPORTED;
    if (!surfOn) return PVOL_E_INVALID;       // the gather is a term of PhotonIntegrator::Li
    if (indirectN) return PVOL_E_INVALID;     // the gather or LPhoton(indirectMap), never both (photonmap.cpp:183, :307)
    if (!haveGather) return PVOL_E_INVALID;
    if (!haveRad || !radN) return PVOL_E_INVALID;
    return PVOL_OK;
}

uint32_t pvol_radiance_gather_slice(int32_t nSamples, uint64_t bound) {
    return pvol_slice_items(bound, PVOL_RADIANCE_SCRATCH_BYTES,
                            (uint64_t)PVOL_RADIANCE_RAY_SCRATCH + PVOL_RADIANCE_GATHER_SCRATCH(std::max(nSamples, 1)) + PVOL_RADIANCE_CALLER_SCRATCH);
}

uint32_t pvol_radiance_slice_cut(const uint32_t *offset, uint32_t n, uint64_t budget) { return offset ? rays_slice_cut(offset, n, budget) : 0u; }

int pvol_radiance_slice_streams(const pvol_stream *streams, uint32_t nStreams, uint32_t nRays, uint32_t r0, uint32_t r1, uint32_t *s,
                                pvol_stream *table, uint32_t *out3, uint32_t *maxRays) {
    if (!streams || !s || !table || !out3 || !maxRays || *s > nStreams || !(r0 < r1 && r1 <= nRays)) return PVOL_E_INVALID;
    if (!streams_partition(streams, nStreams, nRays, maxRays)) return PVOL_E_INVALID;
    std::vector<pvol_stream> t;
    const RaysSliceStreams w = rays_slice_streams(streams, nStreams, r0, r1, nRays, *s, t);
    std::copy(t.begin(), t.end(), table);
    out3[0] = w.s0; out3[1] = w.n; out3[2] = w.continued;
    return PVOL_OK;
}

int pvol_radiance_set_scratch_bound(pvol_ctx *c, uint64_t bytes) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    c->rr.bound = std::min<uint64_t>(bytes, PVOL_RADIANCE_SCRATCH_BYTES);   // the hook only lowers the bound
    return PVOL_OK;
}

}  // extern "C"

static int check_ctx(const pvol_ctx *c, const RadianceBatchCheck *a) {
    return pvol_radiance_batch_check(c != 0, a, c && c->haveScene, c ? c->hs.volKind : 0, c && c->hs.surf.enabled != 0);
}
static int check_ctx(const pvol_ctx *c, const RadianceGatherCheck *a) {
    return pvol_radiance_gather_check(c != 0, a, c && c->haveScene, c ? c->hs.volKind : 0, c && c->hs.surf.enabled != 0,
                                      c ? c->hs.surf.map[SURF_MAP_INDIRECT].nPhotons : 0u, c && c->gather.have, c && c->rad.have, c ? c->rad.n : 0u);
}

// what pvol_radiance_gather_batch* adds to the walk: the caller's parameters with DEVICE sample arrays, and where gather_draws goes
struct RaysGather { pvol_gather_params g; uint32_t *gatherDraws; };

// The call, slice by slice, on device arrays.  hs: host copy of the caller's stream table (already checked).  Caller holds apiMu and has
// the device set.
static int radiance_slices(pvol_ctx *c, const pvol_ray *dRays, uint32_t nRays, pvol_stream *dStreams, const std::vector<pvol_stream> &hs,
                           int outputKind, const pvol_radiance_out &out, hipStream_t stream, const RaysGather *gather = 0) {
    const uint32_t nStreams = (uint32_t)hs.size();
    const bool surfOn = c->hs.surf.enabled != 0, specOn = surfOn && c->specOn;
    const uint32_t maxSeg = pvol_radiance_max_segments(specOn, c->hs.surf.maxSpecularDepth);
    // A slice is sized for rays that spawn nothing, counted, and cut back to the longest run of its rays whose blocks fit the bound: sizing
    // it for the worst case (30 spawned rays each at depth 5) would make slices of a few thousand rays, launches too small for the device
    const uint64_t budget = c->rr.bound ? c->rr.bound : PVOL_RADIANCE_SCRATCH_BYTES;
    const uint64_t perExpanded = (uint64_t)PVOL_RADIANCE_RAY_SCRATCH + (gather ? PVOL_RADIANCE_GATHER_SCRATCH(gather->g.n_samples) : 0u);
    const uint32_t slice = std::min(nRays, gather ? pvol_radiance_gather_slice(gather->g.n_samples, budget) : pvol_radiance_slice(0, budget));
    // an earlier call's kernels, on whatever stream, may still read the scratch
    if (!c->rr.fence.wait(stream)) return PVOL_E_NO_DEVICE;
    size_t tempBytes = 0;
    if (!ok(hipcub::DeviceScan::ExclusiveSum((void *)0, tempBytes, (const uint32_t *)0, (uint32_t *)0, (int)(slice + 1u), stream))) return PVOL_E_NO_DEVICE;
    if (!pvol_reserve(c->buf[PVOL_BUF_RR_COUNT], sizeof(uint32_t) * 2 * ((size_t)slice + 1), stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_RR_TEMP], std::max<size_t>(tempBytes, 16), stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_RR_STASH], surfOn ? sizeof(float) * 60 * (size_t)slice : 0, stream))
        return PVOL_E_NO_MEMORY;
    const size_t width = outputKind == PVOL_OUT_SPECTRAL ? 60 : 4;
    const RegionLaunchers &K = pvol_launchers(c->hs.volKind);
    std::vector<pvol_stream> table;
    std::vector<uint32_t> hostOffset;
    uint32_t s = 0;   // the first stream that may reach into the slice
    for (uint32_t r0 = 0; r0 < nRays;) {
        uint32_t n = std::min(slice, nRays - r0);
        RaysArgs A;
        memset(&A, 0, sizeof(A));
        A.scene = c->ds.get(); A.in = dRays + r0; A.n = n; A.surfOn = surfOn; A.specOn = specOn; A.spectral = outputKind == PVOL_OUT_SPECTRAL;
        A.count = pvol_buf<uint32_t>(c, PVOL_BUF_RR_COUNT); A.offset = A.count + (size_t)slice + 1;
        A.stash = pvol_buf<float>(c, PVOL_BUF_RR_STASH);
        uint32_t total = 0;
        size_t tb = c->buf[PVOL_BUF_RR_TEMP].bytes;
        if (!ok(pvol_launch_rays_count(&A, stream)) ||
            !ok(hipcub::DeviceScan::ExclusiveSum(pvol_buf<unsigned char>(c, PVOL_BUF_RR_TEMP), tb, (const uint32_t *)A.count, (uint32_t *)A.offset, (int)(n + 1u), stream)) ||
            !ok(hipMemcpyAsync(&total, A.offset + n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) || !ok(hipStreamSynchronize(stream)))
            return PVOL_E_NO_DEVICE;
        if (n > 1 && !rays_slice_fits(total, n, budget, perExpanded)) {   // cut: the scan comes back only where the candidate does not fit
            hostOffset.resize((size_t)n + 1);
            if (!ok(hipMemcpy(hostOffset.data(), A.offset, sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
            A.n = n = rays_slice_cut(hostOffset.data(), n, budget, perExpanded);
            total = hostOffset[n];
        }
        const uint32_t r1 = r0 + n;
        table.clear();
        const RaysSliceStreams w = rays_slice_streams(hs.data(), nStreams, r0, r1, nRays, s, table);
        const uint32_t s0 = w.s0, ns = w.n;
        const bool continued = w.continued;
        if (!pvol_reserve(c->buf[PVOL_BUF_RR_STREAMS], sizeof(pvol_stream) * std::max<size_t>(ns, 1), stream)) return PVOL_E_NO_MEMORY;
        pvol_stream *dTable = pvol_buf<pvol_stream>(c, PVOL_BUF_RR_STREAMS);
        // the table is read from pageable memory that the next slice rewrites: wait for the copy
        if (ns && (!ok(hipMemcpyAsync(dTable, table.data(), sizeof(pvol_stream) * ns, hipMemcpyHostToDevice, stream)) || !ok(hipStreamSynchronize(stream))))
            return PVOL_E_NO_DEVICE;
        A.L = out.L + width * (size_t)r0;
        A.surfXyz = out.surf_xyz ? out.surf_xyz + 3 * (size_t)r0 : 0; A.tHit = out.t_hit ? out.t_hit + r0 : 0;
        A.outDraws = out.draws ? out.draws + r0 : 0; A.surfDraws = out.surf_draws ? out.surf_draws + r0 : 0;
        A.nSegments = out.n_segments ? out.n_segments + r0 : 0;
        if (total < n || (uint64_t)total > (uint64_t)n * (maxSeg + 1u)) return PVOL_E_NO_DEVICE;   // cannot happen: the count pass bounds every block
        if (!pvol_reserve(c->buf[PVOL_BUF_RR_RAYS], sizeof(pvol_ray) * (size_t)total, stream) || !pvol_reserve(c->buf[PVOL_BUF_RR_INFO], sizeof(SegInfo) * (size_t)total, stream) ||
            !pvol_reserve(c->buf[PVOL_BUF_RR_ROWS], sizeof(float) * 60 * (size_t)total, stream) || !pvol_reserve(c->buf[PVOL_BUF_RR_DRAWS], sizeof(uint32_t) * (size_t)total, stream))
            return PVOL_E_NO_MEMORY;
        A.rays = pvol_buf<pvol_ray>(c, PVOL_BUF_RR_RAYS); A.info = pvol_buf<SegInfo>(c, PVOL_BUF_RR_INFO);
        A.rows = pvol_buf<float>(c, PVOL_BUF_RR_ROWS);
        uint32_t *dDraws = pvol_buf<uint32_t>(c, PVOL_BUF_RR_DRAWS);
        A.draws = dDraws;
        if (!ok(pvol_launch_rays_emit(&A, dTable, ns, continued ? dStreams + s0 : 0, stream)) ||
            !ok(hipMemsetAsync(A.rows, 0, sizeof(float) * 60 * (size_t)total, stream)) || !ok(hipMemsetAsync(dDraws, 0, sizeof(uint32_t) * (size_t)total, stream)))
            return PVOL_E_NO_DEVICE;
        RaysGatherArgs G;
        memset(&G, 0, sizeof(G));
        if (gather) {   // Lg and its draws for every member, the draws in front of the member's own volume Li()
            const size_t nS = (size_t)gather->g.n_samples, t = total;
            if (!pvol_reserve(c->buf[PVOL_BUF_RG_QUERY], sizeof(float) * 46 * t, stream) || !pvol_reserve(c->buf[PVOL_BUF_RG_U], sizeof(float) * 6 * nS * t, stream) ||
                !pvol_reserve(c->buf[PVOL_BUF_RG_OUT], sizeof(float) * 31 * t, stream))
                return PVOL_E_NO_MEMORY;
            float *q = pvol_buf<float>(c, PVOL_BUF_RG_QUERY), *u = pvol_buf<float>(c, PVOL_BUF_RG_U), *o = pvol_buf<float>(c, PVOL_BUF_RG_OUT);
            G.scene = c->ds.get(); G.rays = A.rays; G.info = A.info; G.offset = A.offset; G.total = total; G.n = n; G.nSamples = gather->g.n_samples;
            G.uBsdf = gather->g.u_bsdf + 3 * nS * r0; G.uPhoton = gather->g.u_photon + 3 * nS * r0;
            G.p = q; G.frames = q + 3 * t; G.wo = q + 12 * t; G.kd = q + 15 * t; G.rayEps = q + 45 * t;
            G.mUBsdf = u; G.mUPhoton = u + 3 * nS * t;
            G.Lg = o; G.gDraws = (uint32_t *)(o + 30 * t);
            G.rows = A.rows; G.gatherDraws = gather->gatherDraws ? gather->gatherDraws + r0 : 0;
            if (!ok(pvol_launch_rays_gather_query(&G, stream))) return PVOL_E_NO_DEVICE;
            const int rc = pvol_final_gather_device(c, G.p, G.frames, G.wo, G.kd, G.rayEps, total, gather->g.max_dist, gather->g.n_samples,
                                                    gather->g.cos_gather_angle, G.mUBsdf, G.mUPhoton, G.Lg, G.gDraws, 0, 0, stream);
            if (rc != PVOL_OK) return rc;
            if (!ok(pvol_launch_rays_gather_patch(&G, stream))) return PVOL_E_NO_DEVICE;
        }
        if (ns) {
            BatchArgs b = {};   // maxRaysPerStream 0: the table lives on the device, as for pvol_li_batch_device
            b.rays = A.rays; b.nRays = total; b.streams = dTable; b.nStreams = ns; b.outputKind = PVOL_OUT_SPECTRAL; b.out = A.rows; b.draws = dDraws;
            b.stream = stream;
            const int rc = pvol_launch_batch(c, b);
            if (rc != PVOL_OK) return rc;
        }
        if (surfOn) {   // Ls at the matte hits of every member, T (.) Ls added into the segments' Lv, Ls itself left in the primaries' rows
            SurfArgs su = {};
            su.scene = c->ds.get(); su.rays = A.rays; su.nRays = total; su.out = A.rows; su.counters = c->dCounters.get(); su.spectral = 1;
            const uint32_t nWaves = (uint32_t)std::min<unsigned long long>(((unsigned long long)total + 63) / 64, (unsigned long long)c->nCU * 24ull);
            if (!ok(pvol_launch_rays_patch(&A, stream)) || !ok(K.surface(&su, nWaves, stream))) return PVOL_E_NO_DEVICE;
            if (gather && !ok(pvol_launch_rays_gather_add(&G, stream))) return PVOL_E_NO_DEVICE;   // Ls_matte + Lg, where Ls_matte went
        }
        if (!ok(pvol_launch_rays_compose(&A, dTable, ns, dStreams + s0, stream))) return PVOL_E_NO_DEVICE;
        r0 = r1;
    }
    return c->rr.fence.record(stream) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

extern "C" {

int pvol_radiance_batch_device(pvol_ctx *c, const pvol_ray *dRays, uint32_t nRays, pvol_stream *dStreams, uint32_t nStreams, int outputKind,
                               const pvol_radiance_out *out, void *hipStream) {
    const RadianceBatchCheck a = {dRays, dStreams, nRays, nStreams, outputKind, out};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // the context's state is read under the lock only
    const int rc0 = check_ctx(c, &a);
    if (rc0 != PVOL_OK) return rc0;
    // VolumeIntegrator "single": served within the render driver's limit, refused beyond it before anything is launched or written
    if (const int rs = pvol_single_caller_status(c)) return rs;
    if (!nRays || !nStreams) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipStream_t stream = (hipStream_t)hipStream;
    std::vector<pvol_stream> hs(nStreams);   // read on the caller's stream: ordered behind whatever produced the table
    if (!ok(hipMemcpyAsync(hs.data(), dStreams, sizeof(pvol_stream) * (size_t)nStreams, hipMemcpyDeviceToHost, stream)) ||
        !ok(hipStreamSynchronize(stream))) return PVOL_E_NO_DEVICE;
    if (!streams_partition(hs.data(), nStreams, nRays, 0)) return PVOL_E_INVALID;
    return radiance_slices(c, dRays, nRays, dStreams, hs, outputKind, *out, stream);
}

int pvol_radiance_batch(pvol_ctx *c, const pvol_ray *rays, uint32_t nRays, pvol_stream *streams, uint32_t nStreams, int outputKind,
                        const pvol_radiance_out *out) {
    const RadianceBatchCheck a = {rays, streams, nRays, nStreams, outputKind, out};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // from the upload to the copy-back: the launches share the context's scratch
    int rc = check_ctx(c, &a);
    if (rc != PVOL_OK) return rc;
    // VolumeIntegrator "single": served within the render driver's limit, refused beyond it before anything is launched or written
    if (const int rs = pvol_single_caller_status(c)) return rs;
    if (!nRays || !nStreams) return PVOL_OK;
    if (!streams_partition(streams, nStreams, nRays, 0)) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const size_t width = outputKind == PVOL_OUT_SPECTRAL ? 60 : 4, n = nRays;
    HostStage st;
    const pvol_ray *dRays = st.in(rays, n);
    const pvol_radiance_out d = {st.out(out->L, width * n), st.out(out->surf_xyz, 3 * n), st.out(out->t_hit, n), st.out(out->draws, n),
                                 st.out(out->surf_draws, n), st.out(out->n_segments, n)};
    pvol_stream *dStreams = st.inout(streams, nStreams);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = radiance_slices(c, dRays, nRays, dStreams, std::vector<pvol_stream>(streams, streams + nStreams), outputKind, d, 0);
    if (rc == PVOL_OK && !ok(hipDeviceSynchronize())) rc = PVOL_E_NO_DEVICE;
    if (rc == PVOL_OK) rc = pvol_check_errors(c);
    return rc != PVOL_OK ? rc : st.download();   // nothing is written unless all of it ran
}

int pvol_radiance_gather_batch_device(pvol_ctx *c, const pvol_ray *dRays, uint32_t nRays, pvol_stream *dStreams, uint32_t nStreams, int outputKind,
                                      const pvol_gather_params *gather, const pvol_radiance_gather_out *out, void *hipStream) {
    const RadianceGatherCheck a = {dRays, dStreams, nRays, nStreams, outputKind, out, gather};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (c->volInt == PVOL_VOLINT_SINGLE) return PVOL_E_UNSUPPORTED;   // no final gather under VolumeIntegrator "single" 
    const int rc0 = check_ctx(c, &a);
    if (rc0 != PVOL_OK) return rc0;
    if (!nRays || !nStreams) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipStream_t stream = (hipStream_t)hipStream;
    std::vector<pvol_stream> hs(nStreams);
    if (!ok(hipMemcpyAsync(hs.data(), dStreams, sizeof(pvol_stream) * (size_t)nStreams, hipMemcpyDeviceToHost, stream)) ||
        !ok(hipStreamSynchronize(stream))) return PVOL_E_NO_DEVICE;
    if (!streams_partition(hs.data(), nStreams, nRays, 0)) return PVOL_E_INVALID;
    const pvol_radiance_out o = {out->L, out->surf_xyz, out->t_hit, out->draws, out->surf_draws, out->n_segments};
    const RaysGather g = {*gather, out->gather_draws};
    return radiance_slices(c, dRays, nRays, dStreams, hs, outputKind, o, stream, &g);
}

int pvol_radiance_gather_batch(pvol_ctx *c, const pvol_ray *rays, uint32_t nRays, pvol_stream *streams, uint32_t nStreams, int outputKind,
                               const pvol_gather_params *gather, const pvol_radiance_gather_out *out) {
    const RadianceGatherCheck a = {rays, streams, nRays, nStreams, outputKind, out, gather};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // from the upload to the copy-back
    if (c->volInt == PVOL_VOLINT_SINGLE) return PVOL_E_UNSUPPORTED;   // no final gather under VolumeIntegrator "single" 
    int rc = check_ctx(c, &a);
    if (rc != PVOL_OK) return rc;
    if (!nRays || !nStreams) return PVOL_OK;
    if (!streams_partition(streams, nStreams, nRays, 0)) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const size_t width = outputKind == PVOL_OUT_SPECTRAL ? 60 : 4, n = nRays, nU = 3 * n * (size_t)gather->n_samples;
    HostStage st;
    const pvol_ray *dRays = st.in(rays, n);
    RaysGather g = {*gather, 0};
    g.g.u_bsdf = st.in(gather->u_bsdf, nU); g.g.u_photon = st.in(gather->u_photon, nU);
    const pvol_radiance_out d = {st.out(out->L, width * n), st.out(out->surf_xyz, 3 * n), st.out(out->t_hit, n), st.out(out->draws, n),
                                 st.out(out->surf_draws, n), st.out(out->n_segments, n)};
    g.gatherDraws = st.out(out->gather_draws, n);
    pvol_stream *dStreams = st.inout(streams, nStreams);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = radiance_slices(c, dRays, nRays, dStreams, std::vector<pvol_stream>(streams, streams + nStreams), outputKind, d, 0, &g);
    if (rc == PVOL_OK && !ok(hipDeviceSynchronize())) rc = PVOL_E_NO_DEVICE;
    if (rc == PVOL_OK) rc = pvol_check_errors(c);
    return rc != PVOL_OK ? rc : st.download();   // nothing is written unless all of it ran
}

}  // extern "C"
