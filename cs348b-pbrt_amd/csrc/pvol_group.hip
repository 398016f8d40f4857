// pvol_group.hip -- several GPUs from one process (pvol_preprocess_group, pvol_render_frame_group): one host thread per context
// drives the multi-rank entry points, an in-process all-gather joins the sharded shoot, and film_sum_kernel adds the contexts' films
// on context 0's device.  Nothing here is fed by RCCL.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "pvol_host.h"

#define PVOL_GROUP_MAX_CTX 64u

// dst[i] += staged[0][i] + ... + staged[nStaged-1][i], added in that order whatever the schedule, so the sum is a pure function of
// the films.  A pixel is one float4 (Lxyz, weightSum): every lane moves 16 B at a time, (nStaged + 1) reads and one write per pixel.
__global__ void __launch_bounds__(256) film_sum_kernel(float4 *__restrict__ dst, const float4 *__restrict__ staged, uint32_t nStaged,
                                                       uint64_t nPix) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nPix; i += stride) {
        float4 a = dst[i];
        for (uint32_t r = 0; r < nStaged; ++r) {
            const float4 s = staged[(uint64_t)r * nPix + i];
            a.x += s.x; a.y += s.y; a.z += s.z; a.w += s.w;
        }
        dst[i] = a;
    }
}

namespace {
// The in-process all-gather of pvol_preprocess_group (a pvol_shoot_comm host all-gather): a barrier and one staging buffer, rank-major.
// An exchange has two phases.  Each rank copies its part in; the last to arrive opens the table for reading.  Each rank then copies the
// whole table out; the last to finish lets the next exchange begin.  A rank whose thread has returned never arrives again, so an
// exchange still waiting for one fails, and so does every exchange after it: the shoot turns that into PVOL_E_NO_DEVICE.
struct Gather {
    std::mutex mu;
    std::condition_variable cv;
    uint32_t n = 0;
    std::vector<unsigned char> stage;
    uint64_t bytes = 0;
    uint32_t arrived = 0;   // ranks that have copied their part into the open exchange
    uint32_t reading = 0;   // ranks yet to copy the last complete table out
    uint64_t done = 0;      // complete exchanges
    bool broken = false;
    std::vector<char> gone;      // rank's thread has returned
    std::vector<char> starved;   // an exchange failed on this rank
    bool anyGone() const { return std::find(gone.begin(), gone.end(), 1) != gone.end(); }
};
struct GatherRank {
    Gather *g;
    uint32_t rank;
};

int group_allgather(void *user, const void *send, void *recv, uint64_t bytes) {
    const GatherRank &me = *(const GatherRank *)user;
    Gather &g = *me.g;
    std::unique_lock<std::mutex> lk(g.mu);
    auto fail = [&] {
        g.broken = true;
        g.starved[me.rank] = 1;
        g.cv.notify_all();
        return -1;
    };
    g.cv.wait(lk, [&] { return g.reading == 0 || g.broken; });
    if (g.broken || g.anyGone()) return fail();
    if (g.arrived == 0) {
        g.bytes = bytes;
        try { g.stage.resize(bytes * g.n); } catch (...) { return fail(); }
    } else if (bytes != g.bytes) {
        return fail();   // the ranks are not in the same exchange
    }
    if (bytes) memcpy(&g.stage[me.rank * bytes], send, bytes);
    const uint64_t mine = g.done;
    if (++g.arrived == g.n) {
        g.arrived = 0;
        g.reading = g.n;
        ++g.done;
        g.cv.notify_all();
    } else {
        g.cv.wait(lk, [&] { return g.done != mine || g.broken || g.anyGone(); });
        if (g.done == mine) return fail();
    }
    lk.unlock();   // the table stays put until every rank has read it
    if (bytes) memcpy(recv, g.stage.data(), bytes * g.n);
    lk.lock();
    if (--g.reading == 0) g.cv.notify_all();
    return 0;
}

void leave(Gather &g, uint32_t rank) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.gone[rank] = 1;
    g.cv.notify_all();
}

bool distinct(pvol_ctx *const *ctxs, uint32_t n) {
    std::vector<pvol_ctx *> v(ctxs, ctxs + n);
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) == v.end();
}

// Runs body(i) on one thread per context and joins them all.  A thread that cannot be started gets PVOL_E_NO_MEMORY and onFail(i).
template <class Body, class OnFail>
void run_threads(uint32_t n, std::vector<int> &rc, Body body, OnFail onFail) {
    std::vector<std::thread> th;
    th.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        try {
            th.emplace_back([&rc, body, i] { rc[i] = body(i); });
        } catch (...) {
            for (uint32_t j = i; j < n; ++j) { rc[j] = PVOL_E_NO_MEMORY; onFail(j); }
            break;
        }
    }
    for (std::thread &t : th) t.join();
}

// Puts the calling thread's current device back on the way out: the group calls run work on several devices from the caller's thread.
struct KeepDevice {
    int dev = -1;
    KeepDevice() { if (!ok(hipGetDevice(&dev))) dev = -1; }
    ~KeepDevice() { if (dev >= 0) hipSetDevice(dev); }
};
}  // namespace

extern "C" int pvol_preprocess_group(pvol_ctx *const *ctxs, uint32_t n, uint32_t n_tasks, uint32_t block_paths) {
    if (!ctxs || n == 0 || n > PVOL_GROUP_MAX_CTX || n_tasks == 0 || n_tasks > 65536 || block_paths == 0 || block_paths > 4096)
        return PVOL_E_INVALID;
    for (uint32_t i = 0; i < n; ++i) if (!ctxs[i]) return PVOL_E_INVALID;
    if (!distinct(ctxs, n)) return PVOL_E_INVALID;
    // what pvol_preprocess_ranks could return before its first exchange, found here so that no thread is started to wait for it
    {
        KeepDevice keep;
        for (uint32_t i = 0; i < n; ++i) {
            if (!ctxs[i]->haveScene) return PVOL_E_NO_SCENE;
            if (!ok(hipSetDevice(ctxs[i]->params.device))) return PVOL_E_NO_DEVICE;
        }
    }
    Gather g;
    g.n = n;
    g.gone.assign(n, 0);
    g.starved.assign(n, 0);
    std::vector<GatherRank> who(n);
    std::vector<pvol_shoot_comm> comm(n);
    for (uint32_t i = 0; i < n; ++i) {
        who[i] = {&g, i};
        comm[i].nccl_comm = 0;
        comm[i].allgather = group_allgather;
        comm[i].user = &who[i];
    }
    std::vector<int> rc(n, PVOL_OK);
    run_threads(n, rc, [&](uint32_t i) {
        const int r = pvol_preprocess_ranks(ctxs[i], n_tasks, block_paths, i, n, &comm[i]);
        leave(g, i);
        return r;
    }, [&](uint32_t i) { leave(g, i); });
    // a context that failed on its own (an exchange never failed on it) is the cause; the others only saw it leave
    for (uint32_t i = 0; i < n; ++i) if (rc[i] != PVOL_OK && !g.starved[i]) return rc[i];
    for (uint32_t i = 0; i < n; ++i) if (rc[i] != PVOL_OK) return rc[i];
    return PVOL_OK;
}

extern "C" int pvol_render_frame_group_window(pvol_ctx *const *ctxs, uint32_t n, const pvol_camera *camera, const pvol_film *film,
                                              const pvol_film_window *window, const pvol_sampler *smp, float *const *dPixels, float *dRgb,
                                              void *const *hipStreams) {
    if (!ctxs || !dPixels || !camera || !film || !smp || n == 0 || n > PVOL_GROUP_MAX_CTX) return PVOL_E_INVALID;
    if (film->x_resolution <= 0 || film->y_resolution <= 0 || !pvol_window_ok(film, window)) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < n; ++i)
        if (!ctxs[i] || !dPixels[i] || ((uintptr_t)dPixels[i] & 15u)) return PVOL_E_INVALID;   // film_sum_kernel moves float4 pixels
    if (!distinct(ctxs, n)) return PVOL_E_INVALID;
    // every film, the staging buffer and the sum hold the window's pixels (film/image.cpp:54), not the resolution's
    const pvol_film_window win = pvol_window_or_full(film, window);
    const uint64_t nPix = (uint64_t)win.x_pixel_count * (uint64_t)win.y_pixel_count;
    const size_t filmBytes = sizeof(float4) * nPix;
    auto streamOf = [&](uint32_t i) { return hipStreams ? (hipStream_t)hipStreams[i] : (hipStream_t)0; };
    KeepDevice keep;
    pvol_ctx *const root = ctxs[0];

    // every context renders its share into its own film; pvol_render_tasks_device synchronises its stream between task batches, so
    // only a thread per context keeps the devices busy at once
    std::vector<int> rc(n, PVOL_OK);
    run_threads(n, rc, [&](uint32_t i) -> int {
        pvol_ctx *c = ctxs[i];
        std::lock_guard<std::recursive_mutex> api(c->apiMu);
        if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
        const hipStream_t s = streamOf(i);
        // the root's last reduce (stage copies, sum, resolve) may still be reading this film
        if (root->groupStageEv.get() && !ok(hipStreamWaitEvent(s, root->groupStageEv.get(), 0))) return PVOL_E_NO_DEVICE;
        const int r = render_share(c, camera, film, window, smp, i, n, dPixels[i], s);
        if (r != PVOL_OK || i == 0) return r;
        if (!c->groupFilmEv.create()) return PVOL_E_NO_DEVICE;
        return ok(hipEventRecord(c->groupFilmEv.get(), s)) ? PVOL_OK : PVOL_E_NO_DEVICE;
    }, [](uint32_t) {});
    for (uint32_t i = 0; i < n; ++i) if (rc[i] != PVOL_OK) return rc[i];

    // the reduce, all on the root's stream: wait for every film, stage films 1 .. n-1 next to the root's, add them, resolve
    std::lock_guard<std::recursive_mutex> api(root->apiMu);
    if (!ok(hipSetDevice(root->params.device))) return PVOL_E_NO_DEVICE;
    const hipStream_t s0 = streamOf(0);
    if (n > 1) {
        DevBuf &stage = root->buf[PVOL_BUF_GROUP_STAGE];
        const size_t need = filmBytes * (n - 1);
        if (need > stage.bytes && root->groupStageEv.get() && !ok(hipEventSynchronize(root->groupStageEv.get()))) return PVOL_E_NO_DEVICE;   // the last sum read it
        if (!pvol_reserve(stage, need, s0)) return PVOL_E_NO_MEMORY;
        float4 *const dStage = (float4 *)stage.p.get();
        if (!root->groupStageEv.create()) return PVOL_E_NO_DEVICE;
        const int dev0 = root->params.device;
        for (uint32_t i = 1; i < n; ++i) {
            if (!ok(hipStreamWaitEvent(s0, ctxs[i]->groupFilmEv.get(), 0)) ||
                !ok(hipMemcpyPeerAsync(dStage + (size_t)(i - 1) * nPix, dev0, dPixels[i], ctxs[i]->params.device, filmBytes, s0)))
                return PVOL_E_NO_DEVICE;
        }
        const uint64_t blocks = std::min<uint64_t>((nPix + 255) / 256, (uint64_t)root->nCU * 8);
        hipLaunchKernelGGL(film_sum_kernel, dim3((uint32_t)blocks), dim3(256), 0, s0, (float4 *)dPixels[0], dStage,
                           n - 1, nPix);
        if (!ok(hipGetLastError())) return PVOL_E_NO_DEVICE;
    }
    int rc0 = dRgb ? pvol_film_resolve_window_device(root, film, window, dPixels[0], dRgb, s0) : PVOL_OK;
    if (n > 1 && rc0 == PVOL_OK && !ok(hipEventRecord(root->groupStageEv.get(), s0))) rc0 = PVOL_E_NO_DEVICE;
    return rc0;
}
extern "C" int pvol_render_frame_group(pvol_ctx *const *ctxs, uint32_t n, const pvol_camera *camera, const pvol_film *film,
                                       const pvol_sampler *smp, float *const *dPixels, float *dRgb, void *const *hipStreams) {
    return pvol_render_frame_group_window(ctxs, n, camera, film, 0, smp, dPixels, dRgb, hipStreams);
}
