// pvol_li_coalesce.hip -- per-sample calls in batches: pvol_li_many, and the coalescer behind pvol_li (include/pvol.h).
//
// A batch of n calls is n streams of one ray each, every stream with its caller's live MT19937 state: the sliced path a lone
// pvol_li takes (pvol_launch_batch with an initial state: RESOLVE + REPLAY, slice of 64 slots per stream), so no kernel mixes
// two calls.  One host-to-device copy, the launches, one device-to-host copy and one wait, all on the context's own stream,
// through staging buffers kept by the context (no allocation per batch once they have grown).  That stream is a blocking one
// and also waits for the context's batches still in flight on other streams: a batch reuses the context's scratch, so it runs
// after whatever pvol_li_batch_device / pvol_render_tasks_device left running, as the lone path's null-stream copies did.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>

#include "pvol_dev.h"

#include "pvol_host.h"

// Staging of one batch of n calls (offsets in bytes, sections packed by n so that one copy moves each direction):
//   in : rays [n] | streams [n] | states [n][625]
//   out: Lv,T [n][60] | states [n][625] | status [n] | the gate word of the backups (one uint32)
static size_t in_bytes(size_t n) { return n * (sizeof(pvol_ray) + sizeof(pvol_stream) + 625 * 4); }
static size_t out_bytes(size_t n) { return n * (60 * 4 + 625 * 4 + 4) + 16; }

// caller holds apiMu; nothing of an earlier batch is in flight (every batch waits for its stream).  All or nothing: a failure leaves
// no host staging and cap 0 (the device halves, PVOL_BUF_LI_IN / _OUT, go with the context's other buffers)
static int reserve_staging(pvol_ctx *c, uint32_t n) {
    LiCoalescer &co = c->co;
    if (!co.stream.create()) return PVOL_E_NO_DEVICE;   // blocking: behind the null stream
    if (n <= co.cap) return PVOL_OK;
    const uint32_t cap = std::min(PVOL_LI_MAX_BATCH, std::max(n, 2 * co.cap));
    co.hostIn.reset(); co.hostOut.reset(); co.cap = 0;
    if (!co.hostIn.alloc(in_bytes(cap)) || !co.hostOut.alloc(out_bytes(cap)) ||
        !pvol_reserve(c->buf[PVOL_BUF_LI_IN], in_bytes(cap), co.stream.get()) || !pvol_reserve(c->buf[PVOL_BUF_LI_OUT], out_bytes(cap), co.stream.get())) {
        (void)hipGetLastError();
        co.hostIn.reset(); co.hostOut.reset();
        return PVOL_E_NO_MEMORY;
    }
    co.cap = cap;
    return PVOL_OK;
}

static void count(pvol_ctx *c, int slot, uint64_t v) {
    std::lock_guard<std::mutex> lk(c->co.mu);
    c->co.stats[slot] += v;
}

// One launch of n validated calls (caller holds apiMu, n within the staging and record limits).
static void run_piece(pvol_ctx *c, LiRequest *const *req, uint32_t n) {
    auto failAll = [&](int rc) { for (uint32_t i = 0; i < n; ++i) req[i]->rc = rc; };
    int rc = reserve_staging(c, n);
    if (rc != PVOL_OK) return failAll(rc);
    const LiCoalescer &co = c->co;
    const size_t oStreams = (size_t)n * sizeof(pvol_ray), oStatesIn = oStreams + (size_t)n * sizeof(pvol_stream);
    const size_t oStatesOut = (size_t)n * 60 * 4, oStatus = oStatesOut + (size_t)n * 625 * 4, oGate = oStatus + (size_t)n * 4;
    pvol_ray *hRays = reinterpret_cast<pvol_ray *>(co.hostIn.get());
    pvol_stream *hStreams = reinterpret_cast<pvol_stream *>(co.hostIn.get() + oStreams);
    uint32_t *hStates = reinterpret_cast<uint32_t *>(co.hostIn.get() + oStatesIn);
    for (uint32_t i = 0; i < n; ++i) {
        hRays[i] = *req[i]->ray;
        memset(&hStreams[i], 0, sizeof(pvol_stream));
        hStreams[i].first_ray = i;
        hStreams[i].n_rays = 1;
        memcpy(hStates + (size_t)i * 625, req[i]->mt, 624 * 4);
        hStates[(size_t)i * 625 + 624] = (uint32_t)*req[i]->mti;
    }
    hipStream_t s = co.stream.get();
    unsigned char *devIn = pvol_buf<unsigned char>(c, PVOL_BUF_LI_IN), *devOut = pvol_buf<unsigned char>(c, PVOL_BUF_LI_OUT);
    float *dOut = reinterpret_cast<float *>(devOut);
    int32_t *dStatus = reinterpret_cast<int32_t *>(devOut + oStatus);
    bool good = pvol_order_after_pending(c, s) == PVOL_OK && ok(hipMemcpyAsync(devIn, co.hostIn.get(), in_bytes(n), hipMemcpyHostToDevice, s)) &&
                ok(hipMemsetAsync(dOut, 0, oStatesOut, s)) && ok(hipMemsetAsync(dStatus, 0, (size_t)n * 4, s));
    rc = good ? PVOL_OK : PVOL_E_NO_DEVICE;
    if (rc == PVOL_OK) {
        BatchArgs b = {};
        b.rays = reinterpret_cast<const pvol_ray *>(devIn); b.nRays = n; b.streams = reinterpret_cast<pvol_stream *>(devIn + oStreams); b.nStreams = n;
        b.outputKind = PVOL_OUT_SPECTRAL; b.out = dOut; b.initState = reinterpret_cast<const uint32_t *>(devIn + oStatesIn);
        b.finalState = reinterpret_cast<uint32_t *>(devOut + oStatesOut); b.maxRaysPerStream = 1; b.stream = s; b.status = dStatus;
        rc = pvol_launch_batch(c, b);
    }
    // a PVOL_E_LIMIT of this batch is in its rays' status only (report_limit): the context's shared count is left alone
    if (rc == PVOL_OK)
        good = ok(hipMemcpyAsync(co.hostOut.get(), devOut, oGate, hipMemcpyDeviceToHost, s)) &&
               ok(hipMemcpyAsync(co.hostOut.get() + oGate, c->dWords.get() + 1, 4, hipMemcpyDeviceToHost, s)) && ok(hipStreamSynchronize(s));
    if (rc == PVOL_OK && !good) rc = PVOL_E_NO_DEVICE;
    if (rc != PVOL_OK) { (void)hipGetLastError(); hipStreamSynchronize(s); return failAll(rc); }
    // The gated backups (li_replay_kernel behind li_group_kernel's replay form) redo EVERY stream of a batch when the hand-over
    // list overflowed, which would change the last bits of calls that did not need it.  Such a batch is redone call by call
    // from the inputs, exactly as lone pvol_li calls.
    const uint32_t gate = *reinterpret_cast<const uint32_t *>(co.hostOut.get() + oGate);
    if (gate != 0u && n > 1) {
        count(c, 4, 1);
        for (uint32_t i = 0; i < n; ++i) req[i]->rc = pvol_li_lone(c, req[i]->ray, req[i]->mt, req[i]->mti, req[i]->Lv, req[i]->T);
        return;
    }
    const float *hOut = reinterpret_cast<const float *>(co.hostOut.get());
    const uint32_t *hFinal = reinterpret_cast<const uint32_t *>(co.hostOut.get() + oStatesOut);
    const int32_t *hStatus = reinterpret_cast<const int32_t *>(co.hostOut.get() + oStatus);
    uint64_t failed = 0;
    for (uint32_t i = 0; i < n; ++i) {
        LiRequest &r = *req[i];
        r.rc = hStatus[i];
        if (r.rc != PVOL_OK) { ++failed; continue; }   // as a lone pvol_li: nothing written
        memcpy(r.Lv, hOut + (size_t)i * 60, 30 * 4);
        memcpy(r.T, hOut + (size_t)i * 60 + 30, 30 * 4);
        memcpy(r.mt, hFinal + (size_t)i * 625, 624 * 4);
        *r.mti = (int32_t)hFinal[(size_t)i * 625 + 624];
    }
    if (failed) count(c, 5, failed);
}

// Every call holds a record slice of 64 slots (the sliced path's floor): a batch whose slices would outgrow the 4 GB record budget of
// the plan (a VolumeGrid with a long step plan) is launched in pieces of this many calls.
extern "C" uint32_t pvol_li_piece(int maxSteps, int grid, uint32_t n) {
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(n, ((size_t)4 << 30) / (pvol_rec_stride(maxSteps, grid != 0) * 64)));
}

// Runs n <= PVOL_LI_MAX_BATCH validated calls; every request's rc is set, its buffers written where it is PVOL_OK.
static void run_batch(pvol_ctx *c, LiRequest *const *req, uint32_t n) {
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->haveScene) { for (uint32_t i = 0; i < n; ++i) req[i]->rc = PVOL_E_NO_SCENE; return; }
    if (!ok(hipSetDevice(c->params.device))) { for (uint32_t i = 0; i < n; ++i) req[i]->rc = PVOL_E_NO_DEVICE; return; }
    const uint32_t piece = pvol_li_piece(c->hs.maxSteps, is_density_region(c->hs.volKind), n);
    for (uint32_t b = 0; b < n; b += piece) run_piece(c, req + b, std::min(piece, n - b));
}

// Leader / followers: every caller queues its request; the first that finds no batch in flight leads one (up to coMaxBatch
// requests from the front of the queue), the others wait for theirs to be done or for the leadership to come free.
int pvol_li_coalesced(pvol_ctx *c, const pvol_ray *ray, uint32_t *mt, int32_t *mti, float *Lv, float *T) {
    LiRequest r = {ray, mt, mti, Lv, T, PVOL_OK, false};
    LiCoalescer &co = c->co;
    std::unique_lock<std::mutex> lk(co.mu);
    if (co.busy) co.stats[3] += 1;
    co.queue.push_back(&r);
    co.more.notify_one();
    std::vector<LiRequest *> batch;
    while (!r.done) {
        if (co.busy) { co.done.wait(lk); continue; }
        co.busy = true;
        const uint32_t maxB = std::max(1u, co.maxBatch.load(std::memory_order_relaxed));
        if (co.maxWaitUs && co.queue.size() < maxB)   // idle leader: a moment for more callers to join
            co.more.wait_for(lk, std::chrono::microseconds(co.maxWaitUs), [&] { return co.queue.size() >= maxB; });
        const size_t n = std::min<size_t>(co.queue.size(), maxB);
        batch.assign(co.queue.begin(), co.queue.begin() + n);
        co.queue.erase(co.queue.begin(), co.queue.begin() + n);
        lk.unlock();
        run_batch(c, batch.data(), (uint32_t)n);
        lk.lock();
        for (LiRequest *q : batch) q->done = true;
        co.stats[0] += n;
        co.stats[1] += 1;
        co.stats[2] = std::max<uint64_t>(co.stats[2], n);
        co.busy = false;
        co.done.notify_all();   // the served callers return; one of the rest leads the next batch
    }
    return r.rc;
}

extern "C" {

int pvol_li_many(pvol_ctx *c, const pvol_ray *rays, uint32_t n, uint32_t *mt, int32_t *mti, float *Lv, float *T, int32_t *status) {
    if (!c) return PVOL_E_INVALID;
    if (n == 0) return PVOL_OK;
    if (!rays || !mt || !mti || !Lv || !T) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < n; ++i)
        if (mti[i] < 0 || mti[i] > 624) return PVOL_E_INVALID;
    std::vector<LiRequest> req(n);
    std::vector<LiRequest *> ptr(n);
    for (uint32_t i = 0; i < n; ++i) {
        req[i] = LiRequest{rays + i, mt + (size_t)i * 624, mti + i, Lv + (size_t)i * 30, T + (size_t)i * 30, PVOL_OK, false};
        ptr[i] = &req[i];
    }
    for (uint32_t b = 0; b < n; b += PVOL_LI_MAX_BATCH) run_batch(c, ptr.data() + b, std::min(PVOL_LI_MAX_BATCH, n - b));
    int first = PVOL_OK;
    for (uint32_t i = 0; i < n; ++i) {
        if (status) status[i] = req[i].rc;
        if (first == PVOL_OK) first = req[i].rc;
    }
    return first;
}

int pvol_set_li_coalescing(pvol_ctx *c, uint32_t max_batch, uint32_t max_wait_us) {
    if (max_batch > PVOL_LI_MAX_BATCH || max_wait_us > PVOL_LI_MAX_WAIT_US || !c) return PVOL_E_INVALID;
    std::lock_guard<std::mutex> lk(c->co.mu);
    c->co.maxBatch.store(max_batch > 1 ? max_batch : 0u, std::memory_order_relaxed);
    c->co.maxWaitUs = max_wait_us;
    return PVOL_OK;
}

int pvol_get_li_coalescing_stats(pvol_ctx *c, uint64_t *out6, int reset) {
    if (!c || !out6) return PVOL_E_INVALID;
    std::lock_guard<std::mutex> lk(c->co.mu);
    memcpy(out6, c->co.stats, sizeof(c->co.stats));
    if (reset) memset(c->co.stats, 0, sizeof(c->co.stats));
    return PVOL_OK;
}

}  // extern "C"
