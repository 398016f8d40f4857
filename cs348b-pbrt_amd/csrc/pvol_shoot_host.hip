// pvol_shoot_host.hip -- host side of PhotonShooter::Preprocess (core/photonshooter.cpp:457-526):
// rounds of one 4096-path block per live virtual task on the device, merged in task order with the
// reference's bookkeeping (running nshot, per-task *Done flags, the "unable to store enough photons"
// abort, photonshooter.cpp:280-356), then the search-structure build.  One driver serves the single-GPU
// shoot and the shoot sharded over ranks (see "the shoot driver" below).
#include <math.h>
#include <string.h>
#include <chrono>
#include <algorithm>
#include <vector>

#include <stdlib.h>
#include <mutex>
#include <rccl/rccl.h>   // types and enums only: the library is bound at run time (pvol_rccl_symbol)

#include "pvol_host.h"
#include "pvol_shoot_args.h"

static bool ok(hipError_t e) { return e == hipSuccess; }

namespace {
struct DevArr {   // device array of floats that grows geometrically, keeping the `used` floats it holds
    float *d = 0;
    size_t cap = 0, used = 0;
    bool resize(size_t n) {
        if (n > cap) {
            size_t nc = std::max(n, cap * 2 + 1024);
            float *nd = 0;
            if (!ok(hipMalloc(&nd, sizeof(float) * nc))) return false;
            if (used && d) hipMemcpy(nd, d, sizeof(float) * used, hipMemcpyDeviceToDevice);
            hipFree(d);
            d = nd; cap = nc;
        }
        used = n;
        return true;
    }
};
struct Buffers {   // one rank's block pools and round tables
    uint32_t *stateA = 0, *stateB = 0, *halton = 0, *flags = 0, *localCounts = 0, *localSurfKind = 0;
    float *localPhotons = 0, *localSurf = 0, *localRad = 0;
    unsigned long long *stats = 0;
    uint32_t *seg = 0;         // host-built segment tables of a round: 3 words per task for the volume merge, 8 for the surface merge
    float *segNshot = 0;
    uint32_t *taskIds = 0;     // slot -> task (ShootArgs::taskIds), only with a communicator
    void release() {
        hipFree(stateA); hipFree(stateB); hipFree(halton); hipFree(flags); hipFree(localCounts); hipFree(localSurfKind);
        hipFree(localPhotons); hipFree(localSurf); hipFree(localRad); hipFree(stats); hipFree(seg); hipFree(segNshot); hipFree(taskIds);
    }
};
}  // namespace

extern "C" void pvol_free_surface_stores(pvol_ctx *c) {
    for (int k = 0; k < 3; ++k) c->surf[k] = pvol_ctx::SurfStore();
    c->dRad.reset(); c->nRad = 0;
    c->surfKept = false;
}

extern "C" int pvol_surface_photon_count(pvol_ctx *c, int kind, uint32_t *n, uint32_t *nPaths) {
    if (!c || kind < 0 || kind > 2 || !n) return PVOL_E_INVALID;
    *n = c->surf[kind].n;
    if (nPaths) *nPaths = c->surf[kind].nPaths;
    return PVOL_OK;
}
extern "C" int pvol_download_surface_photons(pvol_ctx *c, int kind, float *p, float *wo, float *alpha, uint32_t capacity) {
    if (!c || kind < 0 || kind > 2 || !p || !wo || !alpha) return PVOL_E_INVALID;
    const uint32_t n = std::min(capacity, c->surf[kind].n);
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const bool good = ok(hipMemcpy(p, c->surf[kind].p.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                      ok(hipMemcpy(wo, c->surf[kind].wo.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                      ok(hipMemcpy(alpha, c->surf[kind].alpha.get(), sizeof(float) * 30 * (size_t)n, hipMemcpyDeviceToHost));
    return good ? PVOL_OK : PVOL_E_NO_DEVICE;
}
extern "C" int pvol_radiance_photon_count(pvol_ctx *c, uint32_t *n) {
    if (!c || !n) return PVOL_E_INVALID;
    *n = c->nRad;
    return PVOL_OK;
}
extern "C" int pvol_download_radiance_photons(pvol_ctx *c, float *p, float *nrm, float *rhoR, float *rhoT, uint32_t capacity) {
    if (!c || !p || !nrm || !rhoR || !rhoT) return PVOL_E_INVALID;
    const uint32_t n = std::min(capacity, c->nRad);
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    std::vector<float> rec(8 * (size_t)n);
    if (!ok(hipMemcpy(rec.data(), c->dRad.get(), sizeof(float) * 8 * (size_t)n, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(p + 3 * (size_t)i, &rec[8 * (size_t)i], 12);
        memcpy(nrm + 3 * (size_t)i, &rec[8 * (size_t)i + 3], 12);
        int mi;
        memcpy(&mi, &rec[8 * (size_t)i + 6], 4);
        // rho_r / rho_t of the surface's BSDF (photonshooter.cpp:185-188): the only non-specular BxDF on this path is the
        // Lambertian, whose rho() is its reflectance whatever the samples (core/reflection.h:222-223); no transmissive one
        const DevMaterial &m = c->hsh.mats[(mi >= 0 && mi < c->hsh.nMats) ? mi : 0];
        for (int b = 0; b < 30; ++b) { rhoR[30 * (size_t)i + b] = m.kind == PVOL_MATERIAL_MATTE ? m.kd[b] : 0.f; rhoT[30 * (size_t)i + b] = 0.f; }
    }
    return PVOL_OK;
}

extern "C" int pvol_get_preprocess_seconds(pvol_ctx *c, double *out2) {
    if (!c || !out2) return PVOL_E_INVALID;
    out2[0] = c->prepSeconds[0]; out2[1] = c->prepSeconds[1];
    return PVOL_OK;
}

extern "C" int pvol_get_shoot_stats(pvol_ctx *c, uint64_t *out12) {
    if (!c || !out12) return PVOL_E_INVALID;
    memcpy(out12, c->shootStats, sizeof(c->shootStats));
    return PVOL_OK;
}

// ------------------------------------------------------------------------------------------ the shoot driver
// One driver runs both pvol_preprocess_ranks and pvol_preprocess_blocks.  Rank r shoots only the tasks pvol_partition_tasks deals
// it.  Every merge decision is a pure function of the round's count table, so after one all-gather of the count rows per round every
// rank runs the same merge and builds the same plan; its own taken rows go to a rank-local array in global merge order (alpha already
// divided by the running nshot), and one all-gather of those arrays at the end lets every rank place all rows where the single-rank
// merge puts them.  pvol_preprocess_blocks is the one-rank case with no communicator: its exchanges are plain copies, shoot_kernel
// gets no task list, and its rank-local arrays, which hold every task's rows, are the stores.
extern "C" int pvol_partition_tasks(uint32_t nTasks, uint32_t rank, uint32_t nRanks, uint32_t *outIds, uint32_t capacity, uint32_t *nOut);

namespace {
typedef ncclResult_t (*nccl_allgather_fn)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);

// One all-gather: every rank gives `bytes` bytes and receives n_ranks x bytes, rank-major.  Host exchanges (count rows, status,
// counters) stage through device memory on the RCCL branch; device exchanges (photon rows) stage through host memory on the
// callback branch only.  With no communicator a host exchange is an untimed copy and no device exchange takes place.
struct Exchange {
    const pvol_shoot_comm *comm = 0;   // 0: the single-GPU shoot, rank 0 of 1
    nccl_allgather_fn gather = 0;
    uint32_t nRanks = 1;
    void *dStage = 0;
    size_t dStageBytes = 0;
    std::vector<unsigned char> hSend, hRecv;
    double seconds = 0.0;
    ~Exchange() { hipFree(dStage); }
    bool nccl(const void *dSend, void *dRecv, size_t bytes) {
        return gather(dSend, dRecv, bytes, ncclUint8, (ncclComm_t)comm->nccl_comm, 0) == ncclSuccess && ok(hipStreamSynchronize(0));
    }
    bool host(const void *send, void *recv, size_t bytes) {
        if (!comm) { memcpy(recv, send, bytes); return true; }
        const auto t0 = std::chrono::steady_clock::now();
        bool good;
        if (gather) {
            const size_t need = bytes * (nRanks + 1);
            if (need > dStageBytes) {
                hipFree(dStage); dStage = 0; dStageBytes = 0;
                if (!ok(hipMalloc(&dStage, need))) return false;
                dStageBytes = need;
            }
            unsigned char *ds = (unsigned char *)dStage;
            good = ok(hipMemcpy(ds, send, bytes, hipMemcpyHostToDevice)) && nccl(ds, ds + bytes, bytes) &&
                   ok(hipMemcpy(recv, ds + bytes, bytes * nRanks, hipMemcpyDeviceToHost));
        } else {
            good = comm->allgather(comm->user, send, recv, bytes) == 0;
        }
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return good;
    }
    bool device(const void *dSend, void *dRecv, size_t bytes) {   // timed whole, staging included
        const auto t0 = std::chrono::steady_clock::now();
        bool good;
        if (gather) {
            good = nccl(dSend, dRecv, bytes);
        } else {
            hSend.resize(bytes); hRecv.resize(bytes * nRanks);
            good = ok(hipMemcpy(hSend.data(), dSend, bytes, hipMemcpyDeviceToHost)) && comm->allgather(comm->user, hSend.data(), hRecv.data(), bytes) == 0 &&
                   ok(hipMemcpy(dRecv, hRecv.data(), bytes * nRanks, hipMemcpyHostToDevice));
        }
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return good;
    }
};

// The rows of one store: who appended which rows where.  Segments are in global order; local[r] counts rank r's rows so far.
struct Plan {
    std::vector<uint32_t> src, local, global;
    std::vector<uint64_t> localRows;
    uint64_t rows = 0;
    void reset(uint32_t nRanks) { src.clear(); local.clear(); global.clear(); localRows.assign(nRanks, 0); rows = 0; }
    void add(uint32_t r, uint32_t n) {
        if (!n) return;
        src.push_back(r); local.push_back((uint32_t)localRows[r]); global.push_back((uint32_t)rows);
        localRows[r] += n; rows += n;
    }
    uint64_t most() const { uint64_t m = 0; for (uint64_t v : localRows) m = std::max(m, v); return m; }
};

// One store of the shoot (volume, caustic, direct, indirect or radiance): this rank's rows in global merge order, one array per
// field (p, wi|wo, alpha; or the radiance record) of `width` floats a row, and the plan of every rank's rows.
struct Store {
    int nFields;
    uint32_t width[3];
    DevArr f[3];
    Plan plan;
    bool reserve(uint32_t rank) {   // room for this rank's rows of the plan, keeping those merged before
        for (int i = 0; i < nFields; ++i)
            if (!f[i].resize(width[i] * plan.localRows[rank])) return false;
        return true;
    }
};

// All-gathers every rank's local rows of one store and places them in global order into freshly allocated dst[f]
// ([plan.rows][width]).  All ranks call it with the same plan, hence the same sizes, and all return the same code unless the
// exchange itself fails (PVOL_E_NO_DEVICE).  With no communicator the rank's own arrays are the store and move to dst.
int gather_store(Exchange &X, Store &s, uint32_t rank, float **dst) {
    if (!X.comm) {
        for (int f = 0; f < s.nFields; ++f) { dst[f] = s.f[f].d; s.f[f].d = 0; }
        return PVOL_OK;
    }
    for (int f = 0; f < s.nFields; ++f) dst[f] = 0;
    const Plan &plan = s.plan;
    if (!plan.rows) return PVOL_OK;
    const uint64_t M = plan.most(), mine = plan.localRows[rank];
    uint32_t rowWords = 0;
    for (int f = 0; f < s.nFields; ++f) rowWords += s.width[f];
    const size_t sendBytes = sizeof(float) * (size_t)M * rowWords;
    // the plan's bounds, checked before any device index is formed from it
    for (size_t i = 0; i < plan.src.size(); ++i) {
        const uint64_t end = i + 1 < plan.src.size() ? plan.global[i + 1] : plan.rows;
        if (plan.src[i] >= X.nRanks || (uint64_t)plan.local[i] + (end - plan.global[i]) > plan.localRows[plan.src[i]]) return PVOL_E_INVALID;
    }
    float *send = 0, *recv = 0;
    uint32_t *dSeg = 0;
    const size_t nSeg = plan.src.size();
    int rc = PVOL_OK;
    if (!ok(hipMalloc(&send, sendBytes)) || !ok(hipMalloc(&recv, sendBytes * X.nRanks)) || !ok(hipMalloc(&dSeg, sizeof(uint32_t) * 3 * nSeg))) rc = PVOL_E_NO_MEMORY;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f)
        if (!ok(hipMalloc(&dst[f], sizeof(float) * (size_t)plan.rows * s.width[f]))) rc = PVOL_E_NO_MEMORY;
    uint64_t fieldOff = 0;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f) {   // the rank's block: field f's M x width floats, then the next field
        if (mine && !ok(hipMemcpy(send + fieldOff, s.f[f].d, sizeof(float) * (size_t)mine * s.width[f], hipMemcpyDeviceToDevice))) rc = PVOL_E_NO_DEVICE;
        fieldOff += M * s.width[f];
    }
    if (rc == PVOL_OK && !(ok(hipMemcpy(dSeg, plan.src.data(), sizeof(uint32_t) * nSeg, hipMemcpyHostToDevice)) &&
                           ok(hipMemcpy(dSeg + nSeg, plan.local.data(), sizeof(uint32_t) * nSeg, hipMemcpyHostToDevice)) &&
                           ok(hipMemcpy(dSeg + 2 * nSeg, plan.global.data(), sizeof(uint32_t) * nSeg, hipMemcpyHostToDevice)) &&
                           ok(hipDeviceSynchronize())))
        rc = PVOL_E_NO_DEVICE;
    // every rank says whether its buffers are ready before any row moves: a rank that failed above must not leave the others
    // waiting in the collective, nor enter it without buffers
    const uint32_t status = (uint32_t)rc;
    std::vector<uint32_t> all(X.nRanks);
    if (!X.host(&status, all.data(), sizeof(status))) rc = PVOL_E_NO_DEVICE;
    for (uint32_t r = 0; r < X.nRanks && rc == PVOL_OK; ++r) rc = (int)(int32_t)all[r];
    if (rc == PVOL_OK && !X.device(send, recv, sendBytes)) rc = PVOL_E_NO_DEVICE;
    fieldOff = 0;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f) {
        PlaceArgs P;
        P.recv = recv; P.rankStride = M * rowWords; P.fieldOff = fieldOff; P.width = s.width[f];
        P.segSrc = dSeg; P.segLocal = dSeg + nSeg; P.segGlobal = dSeg + 2 * nSeg; P.nSeg = (uint32_t)nSeg; P.nRows = plan.rows; P.dst = dst[f];
        if (!ok(pvol_launch_place_rows(&P, 0))) rc = PVOL_E_NO_DEVICE;
        fieldOff += M * s.width[f];
    }
    if (rc == PVOL_OK && !ok(hipDeviceSynchronize())) rc = PVOL_E_NO_DEVICE;
    hipFree(send); hipFree(recv); hipFree(dSeg);
    if (rc != PVOL_OK) for (int f = 0; f < s.nFields; ++f) { hipFree(dst[f]); dst[f] = 0; }
    return rc;
}

int shoot(pvol_ctx *c, uint32_t n_tasks, uint32_t block_paths, uint32_t rank, Exchange &X) {
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    pvol_free_photons(c);
    pvol_free_surface_stores(c);
    memset(c->shootStats, 0, sizeof(c->shootStats));
    c->prepSeconds[0] = c->prepSeconds[1] = 0.0;
    c->exchangeSeconds = 0.0;
    if (c->hs.nLights == 0) return pvol_push_scene(c);   // photonshooter.cpp:459: decided by the scene, the same on every rank
    int rc = pvol_push_scene(c);
    if (rc != PVOL_OK) return rc;

    const auto tShoot0 = std::chrono::steady_clock::now();
    const uint32_t T = n_tasks, R = X.nRanks;
    const uint32_t blockSize = block_paths;
    const uint32_t giveUpShot = 4096;   // the reference's constant in its give-up test (photonshooter.cpp:283-290), whatever the block
    const size_t SW = pvol_shoot_state_words();
    const bool keep = c->params.keep_surface_photons != 0;
    uint32_t L = 0;   // this rank's tasks: ids[i] = rank + i * R lives in slot i
    pvol_partition_tasks(T, rank, R, 0, 0, &L);
    std::vector<uint32_t> ids(L);
    pvol_partition_tasks(T, rank, R, ids.data(), L, &L);
    const uint32_t Lpad = (T + R - 1) / R;   // rank 0's share, the largest
    const uint32_t Ls = std::max<uint32_t>(L, 1);
    // Room for one block of one task.  Spectral splitting stores up to ~3 photons per path but the usual yield is
    // ~10 photons per 4096-path block, so the pools start small (L x 256 x 144 B) and a round in which some task outgrew
    // one is REDONE with a larger pool from the saved RNG states (the round is a pure function of them): nothing is dropped
    // and nothing is sized for the worst case.
    uint32_t capMax = (uint32_t)std::min<size_t>(65536, std::max<size_t>(256, ((size_t)48 << 30) / ((size_t)Ls * 144)));
    // PVOL_SHOOT_RANK_CAP_MAX lowers this rank's largest block pool, on a single GPU too: a test sets it on one rank to make that
    // rank alone fail
    if (const char *e = getenv("PVOL_SHOOT_RANK_CAP_MAX")) { const long v = atol(e); if (v > 0) capMax = std::min<uint32_t>(capMax, (uint32_t)v); }
    uint32_t cap = std::min<uint32_t>(256, capMax), capS = keep ? std::min<uint32_t>(256, capMax) : 1, capR = keep ? 64 : 1;
    Buffers B;
    int localRc = PVOL_OK;   // this rank's own error, reported to all at the next exchange
    bool good = ok(hipMalloc(&B.stateA, sizeof(uint32_t) * SW * (size_t)Ls)) && ok(hipMalloc(&B.stateB, sizeof(uint32_t) * SW * (size_t)Ls)) &&
                ok(hipMalloc(&B.halton, sizeof(uint32_t) * 48 * (size_t)Ls)) && ok(hipMalloc(&B.flags, sizeof(uint32_t) * Ls)) &&
                ok(hipMalloc(&B.localCounts, sizeof(uint32_t) * 8 * (size_t)Ls)) &&
                ok(hipMalloc(&B.localPhotons, sizeof(float) * 36 * (size_t)cap * Ls)) && ok(hipMalloc(&B.stats, sizeof(unsigned long long) * 8)) &&
                ok(hipMalloc(&B.localSurf, sizeof(float) * 36 * (size_t)capS * Ls)) && ok(hipMalloc(&B.localSurfKind, sizeof(uint32_t) * (size_t)capS * Ls)) &&
                ok(hipMalloc(&B.localRad, sizeof(float) * 8 * (size_t)capR * Ls)) &&
                ok(hipMalloc(&B.seg, sizeof(uint32_t) * 11 * (size_t)Ls)) && ok(hipMalloc(&B.segNshot, sizeof(float) * Ls)) &&
                (!X.comm || ok(hipMalloc(&B.taskIds, sizeof(uint32_t) * Ls))) && ok(hipMemset(B.stats, 0, sizeof(unsigned long long) * 8));
    if (!good) localRc = PVOL_E_NO_MEMORY;

    ShootArgs A;
    A.scene = c->ds.get(); A.shoot = c->dsh.get(); A.nTasks = L; A.stateIn = B.stateA; A.stateOut = B.stateA; A.halton = B.halton; A.flags = B.flags;
    A.localPhotons = B.localPhotons; A.localCounts = B.localCounts; A.cap = cap; A.stats = B.stats; A.init = 1;
    A.localSurf = B.localSurf; A.localSurfKind = B.localSurfKind; A.capS = capS; A.localRad = B.localRad; A.capR = capR; A.keepSurface = keep ? 1 : 0;
    A.gridVolume = is_density_region(c->hs.volKind) ? 1 : 0;
    // the shooter's compilation for the medium's Density() (pvol_region_exp.h)
    const auto launchShoot = c->hs.volKind == PVOL_VOLUME_EXPONENTIAL ? pvol_launch_shoot_exp : pvol_launch_shoot;
    A.blockPaths = blockSize;
    A.taskIds = B.taskIds;   // null with no communicator: slot == task
    if (localRc == PVOL_OK && L && !((!X.comm || ok(hipMemcpy(B.taskIds, ids.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice))) &&
                                     ok(launchShoot(&A, 0)) && ok(hipDeviceSynchronize())))
        localRc = PVOL_E_NO_DEVICE;
    A.init = 0;
    A.stateOut = B.stateB;

    const pvol_params &P = c->params;
    std::vector<uint32_t> flags(T), localFlags(Ls);
    // exchanged per round: a status word, then the count rows of the rank's slots (read there from the device), padded to Lpad rows
    const size_t rowWords = 1 + 8 * (size_t)Lpad;
    std::vector<uint32_t> sendRow(rowWords), table(rowWords * R);
    uint32_t *const localCounts = &sendRow[1];
    // this rank's own appends of a round: volume {slot, count, local offset} and surface {slot, nSurf, take, off[4], nRad}
    std::vector<uint32_t> vTask, vCount, vOff, sTask, sN, sTake, sOff, sRad;
    std::vector<float> vNshot;
    Store S[5] = {{3, {3, 3, 30}}, {3, {3, 3, 30}}, {3, {3, 3, 30}}, {3, {3, 3, 30}}, {1, {8}}};   // volume, caustic, direct, indirect, radiance
    for (Store &s : S) s.plan.reset(R);
    unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    flags.assign(T, (P.n_caustic_photons == 0 ? 1u : 0u) | (P.n_indirect_photons == 0 ? 2u : 0u) | (P.n_volume_photons == 0 ? 4u : 0u));
    uint32_t nshot = 0;
    uint64_t nCaustic = 0, nIndirect = 0, nDirect = 0, nRadTotal = 0;
    uint32_t nCausticPaths = 0, nIndirectPaths = 0, nDirectPaths = 0;
    size_t nVolume = 0;
    bool abortTasks = false;
    uint32_t stallRounds = 0;
    rc = PVOL_OK;
    // the status words of the last exchange: the lowest-ranked nonzero one, or PVOL_OK
    auto agreed = [&](const uint32_t *words, size_t stride) {
        for (uint32_t r = 0; r < R; ++r) if (words[r * stride]) return (int)(int32_t)words[r * stride];
        return (int)PVOL_OK;
    };
    auto unsuccessful = [](uint32_t needed, uint64_t found, uint32_t shot) { return (found < needed && (found == 0 || found < shot / 1024)); };   // photonshooter.cpp:37-39
    for (;;) {
        bool anyLive = false;
        for (uint32_t t = 0; t < T; ++t) anyLive = anyLive || !(flags[t] & 8u);
        if (!anyLive) break;
        for (uint32_t i = 0; i < L; ++i) localFlags[i] = flags[ids[i]];
        if (localRc == PVOL_OK && L && !ok(hipMemcpy(B.flags, localFlags.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice))) localRc = PVOL_E_NO_DEVICE;
        bool redo = false;
        do {   // the rank's own round: one block per live task, redone from the same states if one of its blocks outgrew a pool
            redo = false;
            if (localRc != PVOL_OK || !L) break;
            unsigned long long rs[8];
            if (!ok(hipMemset(B.stats, 0, sizeof(rs))) || !ok(launchShoot(&A, 0)) ||
                !ok(hipMemcpy(localCounts, B.localCounts, sizeof(uint32_t) * 8 * (size_t)L, hipMemcpyDeviceToHost)) ||
                !ok(hipMemcpy(rs, B.stats, sizeof(rs), hipMemcpyDeviceToHost))) { localRc = PVOL_E_NO_DEVICE; break; }
            uint32_t most = 0, mostS = 0, mostR = 0;
            for (uint32_t i = 0; i < L; ++i) {
                if (localFlags[i] & 8u) continue;
                if (!(localFlags[i] & 4u)) most = std::max(most, localCounts[8 * (size_t)i]);
                mostS = std::max(mostS, localCounts[8 * (size_t)i + 4]);
                mostR = std::max(mostR, localCounts[8 * (size_t)i + 5]);
            }
            if (most > cap) {
                if (most > capMax) { localRc = PVOL_E_LIMIT; break; }
                cap = std::min<uint32_t>(capMax, std::max<uint32_t>(most + most / 4, cap * 4));
                hipFree(B.localPhotons); B.localPhotons = 0;
                if (!ok(hipMalloc(&B.localPhotons, sizeof(float) * 36 * (size_t)cap * L))) { localRc = PVOL_E_NO_MEMORY; break; }
                A.localPhotons = B.localPhotons; A.cap = cap;
                redo = true;
            }
            if (keep && mostS > capS) {
                if (mostS > capMax) { localRc = PVOL_E_LIMIT; break; }
                capS = std::min<uint32_t>(capMax, std::max<uint32_t>(mostS + mostS / 4, capS * 4));
                hipFree(B.localSurf); hipFree(B.localSurfKind); B.localSurf = 0; B.localSurfKind = 0;
                if (!ok(hipMalloc(&B.localSurf, sizeof(float) * 36 * (size_t)capS * L)) || !ok(hipMalloc(&B.localSurfKind, sizeof(uint32_t) * (size_t)capS * L))) { localRc = PVOL_E_NO_MEMORY; break; }
                A.localSurf = B.localSurf; A.localSurfKind = B.localSurfKind; A.capS = capS;
                redo = true;
            }
            if (keep && mostR > capR) {
                capR = std::max<uint32_t>(mostR + mostR / 4, capR * 4);
                hipFree(B.localRad); B.localRad = 0;
                if (!ok(hipMalloc(&B.localRad, sizeof(float) * 8 * (size_t)capR * L))) { localRc = PVOL_E_NO_MEMORY; break; }
                A.localRad = B.localRad; A.capR = capR;
                redo = true;
            }
            if (!redo) for (int i = 0; i < 8; ++i) st[i] += rs[i];
        } while (redo);
        if (localRc == PVOL_OK && L) { const uint32_t *tmp = A.stateIn; A.stateIn = A.stateOut; A.stateOut = const_cast<uint32_t *>(tmp); }   // the round stands
        // the count exchange: every rank learns the round's whole table and whether any rank failed
        sendRow[0] = (uint32_t)localRc;
        if (!X.host(sendRow.data(), table.data(), sizeof(uint32_t) * rowWords)) { rc = PVOL_E_NO_DEVICE; break; }
        if (const int e = agreed(table.data(), rowWords)) { rc = e; break; }
        // merge in task order (photonshooter.cpp:280-351), on the whole round's table: every rank takes the same decisions
        vTask.clear(); vCount.clear(); vOff.clear(); vNshot.clear();
        sTask.clear(); sN.clear(); sTake.clear(); sOff.clear(); sRad.clear();
        const size_t volBefore = nVolume;
        const uint64_t causticBefore = nCaustic, indirectBefore = nIndirect;
        for (uint32_t t = 0; t < T; ++t) {
            uint32_t &fl = flags[t];
            if (fl & 8u) continue;
            if (abortTasks) { fl |= 8u; continue; }
            if (nshot > 500000 && (unsuccessful(P.n_caustic_photons, nCaustic, giveUpShot) || unsuccessful(P.n_indirect_photons, nIndirect, giveUpShot) ||
                                   unsuccessful(P.n_volume_photons, nVolume, giveUpShot))) {
                nVolume = 0; nCaustic = nIndirect = 0; nRadTotal = 0;   // photonshooter.cpp:292-298 erases caustic, indirect, volume, radiance
                abortTasks = true;
                fl |= 8u;
                rc = PVOL_E_SHOOT_FAILED;
                continue;
            }
            nshot += blockSize;
            const uint32_t owner = t % R, slot = t / R;   // task t sits in slot t / R of rank t % R
            const uint32_t *lc = &table[owner * rowWords + 1 + 8 * (size_t)slot];
            uint32_t take = 0;
            if (!(fl & 2u)) {
                take |= 2u | 4u;
                nIndirectPaths += blockSize; nDirectPaths += blockSize;
                nIndirect += lc[3];
                if (nIndirect >= P.n_indirect_photons) fl |= 2u;
                nDirect += lc[2];
            }
            if (!(fl & 1u)) {
                take |= 1u;
                nCausticPaths += blockSize;
                nCaustic += lc[1];
                if (nCaustic >= P.n_caustic_photons) fl |= 1u;
            }
            if (keep && (lc[4] || lc[5])) {
                // kind k's records of the block number lc[1 + k]; they go to store k only when bit k of `take` is set
                const uint32_t n[4] = {(take & 1u) ? lc[1] : 0u, (take & 2u) ? lc[2] : 0u, (take & 4u) ? lc[3] : 0u, lc[5]};
                if (owner == rank) {
                    sTask.push_back(slot); sN.push_back(lc[4]); sTake.push_back(take); sRad.push_back(lc[5]);
                    for (int k = 0; k < 4; ++k) sOff.push_back((uint32_t)S[1 + k].plan.localRows[rank]);
                }
                for (int k = 0; k < 4; ++k) S[1 + k].plan.add(owner, n[k]);
            }
            nRadTotal += keep ? lc[5] : 0;
            if (!(fl & 4u)) {
                if (lc[0]) {
                    if (owner == rank) { vTask.push_back(slot); vCount.push_back(lc[0]); vOff.push_back((uint32_t)S[0].plan.localRows[rank]); vNshot.push_back(float(nshot)); }
                    S[0].plan.add(owner, lc[0]);
                    nVolume += lc[0];
                }
                if (nVolume >= P.n_volume_photons) fl |= 4u;
            }
            if ((fl & 7u) == 7u) fl |= 8u;
        }
        if (abortTasks) continue;   // the stores are erased (their plans are never used); the next pass finds every task finished
        if (localRc == PVOL_OK && !vTask.empty()) {   // this rank's taken volume rows, alpha / running nshot (pvol_launch_merge)
            if (!S[0].reserve(rank)) localRc = PVOL_E_NO_MEMORY;
            else {
                MergeArgs M;
                const size_t n = vTask.size();
                M.localPhotons = B.localPhotons; M.cap = cap; M.srcTask = B.seg; M.count = B.seg + Ls; M.dstOff = B.seg + 2 * (size_t)Ls; M.nshot = B.segNshot;
                M.nSeg = (uint32_t)n; M.p = S[0].f[0].d; M.wi = S[0].f[1].d; M.alpha = S[0].f[2].d;
                if (!(ok(hipMemcpy(B.seg, vTask.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(B.seg + Ls, vCount.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(B.seg + 2 * (size_t)Ls, vOff.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(B.segNshot, vNshot.data(), sizeof(float) * n, hipMemcpyHostToDevice)) &&
                      ok(pvol_launch_merge(&M, 0)) && ok(hipDeviceSynchronize())))
                    localRc = PVOL_E_NO_DEVICE;
            }
        }
        if (localRc == PVOL_OK && keep && !sTask.empty()) {   // ... and its surface records and radiance photons (pvol_launch_merge_surface)
            bool g3 = true;
            for (int k = 1; k < 5 && g3; ++k) g3 = S[k].reserve(rank);
            if (!g3) localRc = PVOL_E_NO_MEMORY;
            else {
                SurfMergeArgs M;
                const size_t n = sTask.size();
                uint32_t *d = B.seg + 3 * (size_t)Ls;
                M.localSurf = B.localSurf; M.localSurfKind = B.localSurfKind; M.capS = capS; M.localRad = B.localRad; M.capR = capR;
                M.srcTask = d; M.nSurf = d + Ls; M.take = d + 2 * (size_t)Ls; M.nRad = d + 3 * (size_t)Ls; M.dstOff = d + 4 * (size_t)Ls;
                M.nSeg = (uint32_t)n;
                for (int k = 0; k < 3; ++k) { M.p[k] = S[1 + k].f[0].d; M.wo[k] = S[1 + k].f[1].d; M.alpha[k] = S[1 + k].f[2].d; }
                M.rad = S[4].f[0].d;
                if (!(ok(hipMemcpy(d, sTask.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(d + Ls, sN.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(d + 2 * (size_t)Ls, sTake.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(d + 3 * (size_t)Ls, sRad.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice)) &&
                      ok(hipMemcpy(d + 4 * (size_t)Ls, sOff.data(), sizeof(uint32_t) * 4 * n, hipMemcpyHostToDevice)) &&
                      ok(pvol_launch_merge_surface(&M, 0)) && ok(hipDeviceSynchronize())))
                    localRc = PVOL_E_NO_DEVICE;
            }
        }
        // The reference has no exit for a store that stops growing after a good start (its `unsuccessful` test, photonshooter.cpp:37-39,
        // passes once found >= 4): e.g. a matte scene whose "caustic" photons all come through the medium, after the volume map is
        // full -- it would shoot forever.  Here 256 rounds in a row without a single photon for any store still wanted end the
        // pass the way the reference's own abort does (stores erased, PVOL_E_SHOOT_FAILED), decided on the global counts.
        const bool progress = nCaustic != causticBefore || nIndirect != indirectBefore || nVolume != volBefore;
        stallRounds = progress ? 0u : stallRounds + 1u;
        if (stallRounds >= 256u) {
            nVolume = 0; nCaustic = nIndirect = 0; nRadTotal = 0;
            for (uint32_t t = 0; t < T; ++t) flags[t] |= 8u;
            abortTasks = true;
            rc = PVOL_E_SHOOT_FAILED;
        }
    }
    // the last exchange: status (an error of the last round's appends) and the work counters, summed over the ranks
    if (rc == PVOL_OK || rc == PVOL_E_SHOOT_FAILED) {
        uint64_t sendFin[9];
        std::vector<uint64_t> finAll(9 * (size_t)R);
        sendFin[0] = (uint32_t)localRc;
        for (int i = 0; i < 8; ++i) sendFin[1 + i] = st[i];
        if (!X.host(sendFin, finAll.data(), sizeof(sendFin))) rc = PVOL_E_NO_DEVICE;
        else {
            int e = PVOL_OK;
            for (uint32_t r = 0; r < R && e == PVOL_OK; ++r) e = (int)(int32_t)(uint32_t)finAll[9 * (size_t)r];
            if (e != PVOL_OK) rc = e;
            for (int i = 0; i < 8; ++i) { st[i] = 0; for (uint32_t r = 0; r < R; ++r) st[i] += finAll[9 * (size_t)r + 1 + i]; }
        }
    }
    // paths, follow_calls, no_hit, march_steps, interactions, absorbed, stored_volume, caustic, direct, indirect, split_children, nshot
    c->shootStats[0] = st[0]; c->shootStats[1] = st[1]; c->shootStats[2] = st[2]; c->shootStats[3] = st[3]; c->shootStats[4] = st[4];
    c->shootStats[5] = st[5]; c->shootStats[6] = nVolume; c->shootStats[7] = nCaustic; c->shootStats[8] = nDirect; c->shootStats[9] = nIndirect;
    c->shootStats[10] = st[6]; c->shootStats[11] = nshot;
    if (rc == PVOL_OK && st[7] != 0) rc = PVOL_E_LIMIT;   // a frame stack overflowed on some rank: never silently drop photons
    B.release();
    // the stores: every rank's rows placed in global merge order; the surface stores go to the context whatever happens to the volume map
    if (rc == PVOL_OK && keep) {
        const uint64_t cnt[3] = {nCaustic, nDirect, nIndirect};
        const uint32_t paths[3] = {nCausticPaths, nDirectPaths, nIndirectPaths};
        for (int k = 0; k < 3 && rc == PVOL_OK; ++k) {
            float *dst[3] = {0, 0, 0};
            rc = gather_store(X, S[1 + k], rank, dst);
            if (rc == PVOL_OK && S[1 + k].plan.rows != cnt[k]) rc = PVOL_E_INVALID;
            c->surf[k].p.reset(dst[0]); c->surf[k].wo.reset(dst[1]); c->surf[k].alpha.reset(dst[2]);
            c->surf[k].n = (uint32_t)cnt[k]; c->surf[k].nPaths = paths[k];
        }
        float *dstR = 0;
        if (rc == PVOL_OK) rc = gather_store(X, S[4], rank, &dstR);
        if (rc == PVOL_OK && S[4].plan.rows != nRadTotal) rc = PVOL_E_INVALID;
        c->dRad.reset(dstR); c->nRad = (uint32_t)nRadTotal;
        c->surfKept = true;
        if (rc != PVOL_OK) pvol_free_surface_stores(c);
    }
    float *raw[3] = {0, 0, 0};
    if (rc == PVOL_OK && nVolume) {
        rc = gather_store(X, S[0], rank, raw);
        if (rc == PVOL_OK && S[0].plan.rows != nVolume) rc = PVOL_E_INVALID;
    }
    for (Store &s : S)
        for (DevArr &a : s.f) hipFree(a.d);
    c->prepSeconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - tShoot0).count();
    c->exchangeSeconds = X.seconds;
    if (rc != PVOL_OK || nVolume == 0) {
        for (float *a : raw) hipFree(a);
        return rc;
    }
    // hand the merged arrays to the context and build the search structure
    std::vector<float> hostP(3 * nVolume);
    if (!ok(hipMemcpy(hostP.data(), raw[0], sizeof(float) * 3 * nVolume, hipMemcpyDeviceToHost))) { for (float *a : raw) hipFree(a); return PVOL_E_NO_DEVICE; }
    c->dRawP.reset(raw[0]); c->dRawWi.reset(raw[1]); c->dRawAlpha.reset(raw[2]);
    const auto tBuild0 = std::chrono::steady_clock::now();
    rc = pvol_finish_map(c, (uint32_t)nVolume, hostP.data());
    hipDeviceSynchronize();
    c->prepSeconds[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - tBuild0).count();
    return rc;
}
}  // namespace

extern "C" int pvol_preprocess(pvol_ctx *c, uint32_t n_tasks) { return pvol_preprocess_blocks(c, n_tasks, 4096); }

extern "C" int pvol_preprocess_blocks(pvol_ctx *c, uint32_t n_tasks, uint32_t block_paths) {
    if (!c || n_tasks == 0 || n_tasks > 65536 || block_paths == 0 || block_paths > 4096) return PVOL_E_INVALID;
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    Exchange X;   // no communicator: rank 0 of 1
    return shoot(c, n_tasks, block_paths, 0, X);
}

extern "C" int pvol_preprocess_ranks(pvol_ctx *c, uint32_t n_tasks, uint32_t block_paths, uint32_t rank, uint32_t n_ranks,
                                     const pvol_shoot_comm *comm) {
    // argument checks first: none of them touches the context or the device
    if (!c || n_tasks == 0 || n_tasks > 65536 || block_paths == 0 || block_paths > 4096 || n_ranks == 0 || rank >= n_ranks || !comm)
        return PVOL_E_INVALID;
    if ((comm->nccl_comm != 0) == (comm->allgather != 0)) return PVOL_E_INVALID;   // exactly one of the two
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    Exchange X;
    X.comm = comm; X.nRanks = n_ranks;
    if (comm->nccl_comm && !(X.gather = (nccl_allgather_fn)pvol_rccl_symbol("ncclAllGather"))) return PVOL_E_NO_DEVICE;   // no RCCL in reach
    return shoot(c, n_tasks, block_paths, rank, X);
}

extern "C" int pvol_get_exchange_seconds(pvol_ctx *c, double *out) {
    if (!c || !out) return PVOL_E_INVALID;
    *out = c->exchangeSeconds;
    return PVOL_OK;
}
