// pvol_render_host.hip -- the render driver, SURVEY 8(f)-1: host side of pvol_render_tasks_device.  pvol_render_plan decides everything
// a call can decide without a device; render_batch enqueues one batch of the plan; render_share is one rank's part of a
// frame, behind pvol_render_frame_ranks here and pvol_render_frame_group (pvol_group.hip).  No kernel lives here: the per-task
// sampler/camera kernel is pvol_tile_dev.h (compiled with the march kernels), the film kernels are pvol_tile.hip.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include <rccl/rccl.h>   // types and enums only: the library is bound at run time (pvol_rccl_symbol)

#include "pvol_host.h"

// ------------------------------------------------------------------------------------------ the plan
// The sampler carries the sample extent (the window's own, pvol_film_sample_extent, or any other): every size below -- the tasks'
// sub-windows, the batches, the work buffers, the debug records -- comes from it, and only the splat reads the window.
static int render_check(const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                        const uint32_t *taskIds, uint32_t nTaskIds, bool havePixels, bool haveScene) {
    if (!camera || !smp || !film_ok(film) || !pvol_window_ok(film, window) || (nTaskIds && !taskIds) || !havePixels) return PVOL_E_INVALID;
    if (!haveScene) return PVOL_E_NO_SCENE;
    const uint32_t spp = smp->pixel_samples;
    if (spp == 0 || (spp & (spp - 1)) || spp > PVOL_MAX_PIXEL_SAMPLES) return PVOL_E_INVALID;   // LDSampler rounds up to a power of two itself
    if (camera->lens_radius != 0.f) return PVOL_E_UNSUPPORTED;
    if (smp->n1d_count > PVOL_MAX_SAMPLE_ARRAYS || smp->n2d_count > PVOL_MAX_SAMPLE_ARRAYS) return PVOL_E_LIMIT;
    if (smp->scatter_index >= smp->n1d_count || smp->n1d[smp->scatter_index] != 1) return PVOL_E_INVALID;
    if (smp->n_tasks == 0 || smp->x_end < smp->x_start || smp->y_end < smp->y_start) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < nTaskIds; ++i) if (taskIds[i] >= smp->n_tasks) return PVOL_E_INVALID;
    return PVOL_OK;
}

RenderPlan pvol_render_plan(const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                            const uint32_t *taskIds, uint32_t nTaskIds, bool havePixels, bool haveScene, bool surfOn, bool specOn,
                            int64_t tileBatchRays) {
    RenderPlan p;
    memset(&p.tile, 0, sizeof(p.tile));
    p.batchRays = 0;
    p.rc = render_check(camera, film, window, smp, taskIds, nTaskIds, havePixels, haveScene);
    if (p.rc != PVOL_OK) return p;

    TileArgs &T = p.tile;
    memcpy(T.r2c, camera->raster_to_camera, sizeof(T.r2c));
    memcpy(T.c2w, camera->camera_to_world, sizeof(T.c2w));
    T.shutterOpen = camera->shutter_open; T.shutterClose = camera->shutter_close;
    T.spp = smp->pixel_samples; T.n1dCount = smp->n1d_count; T.n2dCount = smp->n2d_count;
    memcpy(T.n1d, smp->n1d, sizeof(T.n1d));
    memcpy(T.n2d, smp->n2d, sizeof(T.n2d));
    T.scatterIndex = smp->scatter_index;

    // batches of tasks bounded by the work-buffer budget (rays 48 B + xy 8 B + XYZ 16 B per sample)
    p.batchRays = std::min<uint64_t>(tileBatchRays > 0 ? (uint64_t)tileBatchRays : (uint64_t)256 << 20, 0xfffff000u);
    p.win = std::vector<int32_t>(4 * (size_t)nTaskIds);
    p.count = std::vector<uint64_t>(nTaskIds);
    for (uint32_t i = 0; i < nTaskIds; ++i) {
        p.count[i] = pvol_task_samples(smp, taskIds[i], &p.win[4 * (size_t)i]);
        if (p.count[i] > p.batchRays) { p.rc = PVOL_E_LIMIT; return p; }
    }
    p.streams = std::vector<pvol_stream>(nTaskIds);
    uint64_t doneRays = 0;
    for (uint32_t b0 = 0; b0 < nTaskIds;) {
        RenderBatch b = {};
        b.b0 = b0; b.b1 = b0; b.doneRays = doneRays;
        while (b.b1 < nTaskIds && b.nRays + p.count[b.b1] <= p.batchRays) {
            pvol_stream &s = p.streams[b.b1];
            memset(&s, 0, sizeof(s));
            s.seed = taskIds[b.b1];          // RNG rng(taskNum), samplerrenderer.cpp:73
            s.first_ray = (uint32_t)b.nRays;
            s.n_rays = (uint32_t)p.count[b.b1];
            b.nRays += p.count[b.b1];
            b.maxRays = std::max<uint32_t>(b.maxRays, (uint32_t)p.count[b.b1]);
            ++b.b1;
        }
        const uint64_t nStreams = b.b1 - b.b0;
        b.surfOn = surfOn && b.nRays;
        b.specOn = b.surfOn && specOn;
        // work buffers; with the surface integrator every sample's T, with specular surfaces in view a link word per sample (its segments)
        const uint64_t want[7] = {std::max<uint64_t>(sizeof(pvol_ray) * b.nRays, 64), std::max<uint64_t>(8 * b.nRays, 64),
                                  std::max<uint64_t>(16 * b.nRays, 64), sizeof(pvol_stream) * nStreams, 16 * nStreams,
                                  b.surfOn ? sizeof(TauRec) * b.nRays : 0, b.specOn ? 4 * b.nRays : 0};
        memcpy(b.want, want, sizeof(want));
        p.batches.push_back(b);
        doneRays += b.nRays;
        b0 = b.b1;
    }
    return p;
}

// The plan as words, for the tests: flags = {dPixels given, haveScene, surface integrator on, specOn}.  Writes to out[0, cap) and returns the
// words of the whole record: rc, then -- only when rc is PVOL_OK -- batchRays, the tasks and the batches; of TileArgs spp, n1dCount, n2dCount,
// scatterIndex, n1d, n2d and the bits of shutterOpen, shutterClose, r2c, c2w; per task x0, x1, y0, y1, samples and its stream (seed, first_ray,
// n_rays, reserved, start_draw, end_draw); per batch b0, b1, nRays, maxRays, doneRays, surfOn, specOn and the seven sizes.
extern "C" size_t pvol_render_plan_flat(const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                                        const uint32_t *taskIds, uint32_t nTaskIds, const int32_t *flags, int64_t tileBatchRays, uint64_t *out,
                                        size_t cap) {
    if (!flags) return 0;
    const RenderPlan p = pvol_render_plan(camera, film, window, smp, taskIds, nTaskIds, flags[0] != 0, flags[1] != 0, flags[2] != 0, flags[3] != 0,
                                          tileBatchRays);
    size_t n = 0;
    auto put = [&](uint64_t v) { if (n < cap) out[n] = v; ++n; };
    auto bits = [&](float f) { uint32_t u; memcpy(&u, &f, 4); put(u); };
    put((uint64_t)(int64_t)p.rc);
    if (p.rc != PVOL_OK) return n;
    put(p.batchRays); put(p.count.size()); put(p.batches.size());
    const TileArgs &T = p.tile;
    put(T.spp); put(T.n1dCount); put(T.n2dCount); put(T.scatterIndex);
    for (uint32_t v : T.n1d) put(v);
    for (uint32_t v : T.n2d) put(v);
    bits(T.shutterOpen); bits(T.shutterClose);
    for (float f : T.r2c) bits(f);
    for (float f : T.c2w) bits(f);
    for (size_t i = 0; i < p.count.size(); ++i) {
        for (int k = 0; k < 4; ++k) put((uint64_t)(int64_t)p.win[4 * i + k]);
        put(p.count[i]);
        const pvol_stream &s = p.streams[i];
        put(s.seed); put(s.first_ray); put(s.n_rays); put(s.reserved); put(s.start_draw); put(s.end_draw);
    }
    for (const RenderBatch &b : p.batches) {
        put(b.b0); put(b.b1); put(b.nRays); put(b.maxRays); put(b.doneRays); put((uint64_t)b.surfOn); put((uint64_t)b.specOn);
        for (uint64_t w : b.want) put(w);
    }
    return n;
}

// ------------------------------------------------------------------------------------------ the executor
namespace {
// A call that fails after it (or the pvol_launch_batch it called) opened a phase would leave that interval open, and the next
// pvol_get_phase_ms would charge the gap up to the next call's first mark to it: every exit but the one that sets `keep` closes it.
struct PhaseClose {
    pvol_ctx *c; hipStream_t stream; size_t marks0; bool keep = false;
    static size_t marks(pvol_ctx *c) { std::lock_guard<std::mutex> g(c->timer.mu); return c->phases.marks.size(); }
    ~PhaseClose() {
        if (keep) return;
        bool open;
        {
            std::lock_guard<std::mutex> g(c->timer.mu);
            open = c->phases.marks.size() > marks0 && c->phases.marks.back().first != PVOL_PHASE_END;
        }
        if (open) pvol_phase_mark(c, stream, PVOL_PHASE_END);
    }
};

// One batch of the plan, enqueued on `stream`: reserve, upload its stream table and windows, generate + march (pvol_launch_batch), the
// surface term, the splat, the debug records.
int render_batch(pvol_ctx *c, const RenderPlan &plan, const RenderBatch &b, const pvol_film *film, const pvol_film_window *window,
                 float *dPixels, const pvol_render_debug *debug, hipStream_t stream) {
    const uint32_t nStreams = b.b1 - b.b0;
    const uint64_t nRays = b.nRays;
    for (int i = 0; i < 5; ++i) if (!pvol_reserve(c->buf[PVOL_BUF_TILE_RAYS + i], b.want[i], stream)) return PVOL_E_NO_MEMORY;
    if (!pvol_reserve(c->buf[PVOL_BUF_TAU], b.want[5], stream) || !pvol_reserve(c->buf[PVOL_BUF_SPEC_LINK], b.want[6], stream)) return PVOL_E_NO_MEMORY;
    pvol_ray *dRays = pvol_buf<pvol_ray>(c, PVOL_BUF_TILE_RAYS);
    float *dXY = pvol_buf<float>(c, PVOL_BUF_TILE_XY), *dOut = pvol_buf<float>(c, PVOL_BUF_TILE_OUT);
    pvol_stream *dStreams = pvol_buf<pvol_stream>(c, PVOL_BUF_TILE_STREAMS);
    int4 *dWin = pvol_buf<int4>(c, PVOL_BUF_TILE_WINDOWS);
    TauRec *dTau = pvol_buf<TauRec>(c, PVOL_BUF_TAU);
    uint32_t *dSpecLink = pvol_buf<uint32_t>(c, PVOL_BUF_SPEC_LINK);
    // the previous batch's kernels still read the buffers: these copies are ordered behind them on `stream`
    if (!ok(hipMemcpyAsync(dStreams, &plan.streams[b.b0], sizeof(pvol_stream) * nStreams, hipMemcpyHostToDevice, stream)) ||
        !ok(hipMemcpyAsync(dWin, &plan.win[4 * (size_t)b.b0], 16 * (size_t)nStreams, hipMemcpyHostToDevice, stream)))
        return PVOL_E_NO_DEVICE;
    if (!ok(hipStreamSynchronize(stream))) return PVOL_E_NO_DEVICE;   // the copies read pageable host memory of the plan
    TileArgs T = plan.tile;
    T.windows = dWin; T.rays = dRays; T.xy = dXY;
    T.specOn = b.specOn; T.specLink = b.specOn ? dSpecLink : 0;
    if (b.specOn && !ok(hipMemsetAsync(dSpecLink, 0, 4 * nRays, stream))) return PVOL_E_NO_DEVICE;
    if (nRays) {
        float *const surfOut = debug && debug->d_surf_xyz ? debug->d_surf_xyz + 3 * b.doneRays : 0;
        BatchArgs a = {};
        a.rays = dRays; a.nRays = (uint32_t)nRays; a.streams = dStreams; a.nStreams = nStreams; a.outputKind = PVOL_OUT_XYZ; a.out = dOut;
        a.maxRaysPerStream = b.maxRays; a.tile = &T; a.stream = stream;
        a.tauOut = b.surfOn ? dTau : 0; a.specSurfOut = b.specOn ? surfOut : 0;
        int rc = pvol_launch_batch(c, a);
        if (rc != PVOL_OK) return rc;
        if (b.surfOn) {   // Ls of PhotonIntegrator::Li, composed as T * Ls + Lvi (samplerrenderer.cpp:95-97)
            SurfArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.link = b.specOn ? dSpecLink : 0;
            sa.scene = c->ds.get(); sa.rays = dRays; sa.nRays = (uint32_t)nRays; sa.out = dOut; sa.tau = dTau;
            sa.surfOut = surfOut;
            sa.counters = c->dCounters.get();
            const unsigned long long groups = (nRays + 63) / 64;
            pvol_phase_mark(c, stream, PVOL_PHASE_SURFACE);
            if (!ok(pvol_launchers(c->hs.volKind).surface(&sa, (uint32_t)std::min<unsigned long long>(groups, (unsigned long long)c->nCU * 24ull), stream)))
                return PVOL_E_NO_DEVICE;
        }
        pvol_phase_mark(c, stream, PVOL_PHASE_FILM);
        rc = film_add(c, film, window, dXY, dOut, 4, nRays, 1, dPixels, stream);
        pvol_phase_mark(c, stream, PVOL_PHASE_END);
        if (rc != PVOL_OK) return rc;
    }
    if (debug) {
        if (debug->d_rays && nRays) hipMemcpyAsync(debug->d_rays + b.doneRays, dRays, sizeof(pvol_ray) * nRays, hipMemcpyDeviceToDevice, stream);
        if (debug->d_image_xy && nRays) hipMemcpyAsync(debug->d_image_xy + 2 * b.doneRays, dXY, 8 * nRays, hipMemcpyDeviceToDevice, stream);
        if (debug->d_xyz && nRays) hipMemcpyAsync(debug->d_xyz + 4 * b.doneRays, dOut, 16 * nRays, hipMemcpyDeviceToDevice, stream);
        if (debug->d_streams) hipMemcpyAsync(debug->d_streams + b.b0, dStreams, sizeof(pvol_stream) * nStreams, hipMemcpyDeviceToDevice, stream);
    }
    return PVOL_OK;
}
}  // namespace

extern "C" int pvol_render_tasks_window_device(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window,
                                               const pvol_sampler *smp, const uint32_t *taskIds, uint32_t nTaskIds, float *dPixels,
                                               const pvol_render_debug *debug, void *hipStream) {
    if (!c) return PVOL_E_INVALID;
    RenderPlan plan = pvol_render_plan(camera, film, window, smp, taskIds, nTaskIds, dPixels != 0, c->haveScene, c->hs.surf.enabled != 0, c->specOn,
                                       pvol_read_knobs().tileBatchRays);
    if (plan.rc != PVOL_OK) return plan.rc;
    {   // VolumeIntegrator "single": what the driver does not serve is refused before anything is launched or written
        std::lock_guard<std::recursive_mutex> api(c->apiMu);
        const int rc = pvol_single_render_status(c);
        if (rc != PVOL_OK) return rc;
    }
#ifdef PVOL_TIMING_KNOBS   // timing experiments only (tools/tile_debug_*.sh build with it): every knob gives WRONG images and stream
                           // positions, so the shipped library does not read the variable at all
    pvol_env_tile_debug(pvol_env_get, &plan.tile.debugSkip);
#endif
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // the work buffers and launch scratch live in the context
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const hipStream_t stream = (hipStream_t)hipStream;
    PhaseClose phases{c, stream, PhaseClose::marks(c)};
    for (const RenderBatch &b : plan.batches) {
        const int rc = render_batch(c, plan, b, film, window, dPixels, debug, stream);
        if (rc != PVOL_OK) return rc;
    }
    phases.keep = true;
    return PVOL_OK;
}
extern "C" int pvol_render_tasks_device(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_sampler *smp,
                                        const uint32_t *taskIds, uint32_t nTaskIds, float *dPixels, const pvol_render_debug *debug,
                                        void *hipStream) {
    return pvol_render_tasks_window_device(c, camera, film, 0, smp, taskIds, nTaskIds, dPixels, debug, hipStream);
}

// ------------------------------------------------------------------------------------------ multi-GPU frame (north_star)
// It returns its status in front of any collective: a caller that must reach one whatever the status (a rank whose peers already wait
// in ncclReduce) can do so with the status in hand.
int render_share(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                 uint32_t rank, uint32_t nRanks, float *dPixels, hipStream_t stream) {
    uint32_t n = 0;
    pvol_partition_tasks(smp->n_tasks, rank, nRanks, 0, 0, &n);
    std::vector<uint32_t> ids(n);
    pvol_partition_tasks(smp->n_tasks, rank, nRanks, ids.data(), n, &n);
    const pvol_film_window w = pvol_window_or_full(film, window);
    {   // ... the film's zeroing included
        std::lock_guard<std::recursive_mutex> api(c->apiMu);
        const int rc = pvol_single_render_status(c);
        if (rc != PVOL_OK) return rc;
    }
    if (!ok(hipMemsetAsync(dPixels, 0, sizeof(float) * 4 * (size_t)w.x_pixel_count * w.y_pixel_count, stream))) return PVOL_E_NO_DEVICE;
    return pvol_render_tasks_window_device(c, camera, film, window, smp, ids.data(), n, dPixels, 0, stream);
}

typedef ncclResult_t (*nccl_reduce_fn)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t);

// One rank of an N-GPU frame: its share of the render tasks into its own film (the window's pixels), ONE ncclReduce(sum) of the film to rank 0
// (the Gaussian filter splats across tile borders, film/image.cpp:82-134, so tiles cannot simply be gathered), resolve on rank 0.
// Every rank holds the whole photon map beforehand: pvol_preprocess with the same seeds on each rank, or pvol_preprocess_ranks,
// which shares the shoot and leaves the same map on all of them.
extern "C" int pvol_render_frame_ranks_window(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window,
                                              const pvol_sampler *smp, uint32_t rank, uint32_t nRanks, void *ncclComm, float *dPixels,
                                              float *dRgb, void *hipStream) {
    if (!c || !smp || !film_ok(film) || !pvol_window_ok(film, window) || !dPixels || !nRanks || rank >= nRanks) return PVOL_E_INVALID;
    if (nRanks > 1 && !ncclComm) return PVOL_E_INVALID;
    nccl_reduce_fn reduce = 0;
    if (nRanks > 1 && !(reduce = (nccl_reduce_fn)pvol_rccl_symbol("ncclReduce"))) return PVOL_E_NO_DEVICE;   // no RCCL in reach
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipStream_t stream = (hipStream_t)hipStream;
    int rc = render_share(c, camera, film, window, smp, rank, nRanks, dPixels, stream);
    if (rc != PVOL_OK) return rc;
    const pvol_film_window w = pvol_window_or_full(film, window);
    const size_t nFloats = (size_t)w.x_pixel_count * w.y_pixel_count * 4;
    if (nRanks > 1 && reduce(dPixels, dPixels, nFloats, ncclFloat, ncclSum, 0, (ncclComm_t)ncclComm, stream) != ncclSuccess) return PVOL_E_NO_DEVICE;
    if (rank == 0 && dRgb) rc = pvol_film_resolve_window_device(c, film, window, dPixels, dRgb, hipStream);
    return rc;
}
extern "C" int pvol_render_frame_ranks(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_sampler *smp,
                                       uint32_t rank, uint32_t nRanks, void *ncclComm, float *dPixels, float *dRgb, void *hipStream) {
    return pvol_render_frame_ranks_window(c, camera, film, 0, smp, rank, nRanks, ncclComm, dPixels, dRgb, hipStream);
}
