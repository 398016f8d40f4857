// pvol_shoot_host.hip -- host side of PhotonShooter::Preprocess (core/photonshooter.cpp:457-526): rounds of one 4096-path block per
// live virtual task on the device, merged in task order with the reference's bookkeeping (running nshot, per-task *Done flags, the
// "unable to store enough photons" abort, photonshooter.cpp:280-356), then the search-structure build.  The bookkeeping is ShootMerge
// (pvol_shoot_merge.h: pure, tested on the CPU); this unit drives the device with what it decides.  One driver serves the single-GPU shoot and
// the shoot sharded over ranks (see "the shoot driver" below).  A DevPtr (pvol_host.h) holds every device allocation: no path frees by hand.
#include <string.h>
#include <chrono>
#include <stdlib.h>
#include <rccl/rccl.h>   // types and enums only: the library is bound at run time (pvol_rccl_symbol)

#include "pvol_host.h"
#include "pvol_shoot_args.h"
#include "pvol_shoot_merge.h"

namespace {
struct DevArr {   // device array of floats that grows geometrically, keeping the `used` floats it holds
    DevPtr<float> d;
    size_t cap = 0, used = 0;
    bool resize(size_t n) {
        if (n > cap) {
            const size_t nc = std::max(n, cap * 2 + 1024);
            DevPtr<float> nd;
            if (!nd.alloc(nc)) return false;
            if (used && d.get()) hipMemcpy(nd.get(), d.get(), sizeof(float) * used, hipMemcpyDeviceToDevice);
            d = std::move(nd); cap = nc;
        }
        used = n;
        return true;
    }
};
struct Buffers {   // one rank's block pools and round tables
    DevPtr<uint32_t> stateA, stateB, halton, flags, localCounts, localSurfKind;
    DevPtr<float> localPhotons, localSurf, localRad;
    DevPtr<unsigned long long> stats;
    DevPtr<uint32_t> seg;      // host-built segment tables of a round: 3 words per task for the volume merge, 8 for the surface merge
    DevPtr<float> segNshot;
    DevPtr<uint32_t> taskIds;  // slot -> task (ShootArgs::taskIds), only with a communicator
    // the block pools: room for `cap` photons, `capS` surface records, `capR` radiance photons a slot
    bool photons(size_t cap, size_t slots) { return localPhotons.alloc(36 * cap * slots); }
    bool surface(size_t capS, size_t slots) { return localSurf.alloc(36 * capS * slots) && localSurfKind.alloc(capS * slots); }
    bool radiance(size_t capR, size_t slots) { return localRad.alloc(8 * capR * slots); }
};
}  // namespace

extern "C" void pvol_free_surface_stores(pvol_ctx *c) {
    for (int k = 0; k < 3; ++k) c->surf[k] = pvol_ctx::SurfStore();
    c->dRad.reset(); c->nRad = 0;
    c->surfKept = false;
    c->rad = RadianceResult();   // what pvol_compute_radiance made of them
    c->gather = GatherMap();     // ... and pvol_build_gather_map
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
// it.  Every merge decision is a pure function of the round's count table (ShootMerge), so after one all-gather of the count rows
// per round every rank runs the same merge and builds the same plan; its own taken rows go to a rank-local array in global merge
// order (alpha already divided by the running nshot), and one all-gather of those arrays at the end lets every rank place all rows
// where the single-rank merge puts them.  pvol_preprocess_blocks is the one-rank case with no communicator: its exchanges are plain
// copies, shoot_kernel gets no task list, and its rank-local arrays, which hold every task's rows, are the stores.
extern "C" int pvol_partition_tasks(uint32_t nTasks, uint32_t rank, uint32_t nRanks, uint32_t *outIds, uint32_t capacity, uint32_t *nOut);

// ShootMerge replayed over `nTables` recorded count tables (rowWords() x R words each), or until no task is live, for
// cfg = {T, R, rank, blockPaths, keep, caustic, indirect, volume photons wanted}.  Writes to out[0, cap) and returns the words of the
// whole record: the rounds consumed; after each round 12 words of state, then flags and the rank's nine append vectors (vNshot as
// its value); at the end the five plans (src, local, global, localRows, then rows).  Every vector follows its length.  0: no such shoot.
extern "C" size_t pvol_shoot_merge_replay(const uint32_t *cfg, const uint32_t *tables, uint32_t nTables, uint64_t *out, size_t cap) {
    if (!cfg || !cfg[0] || !cfg[1] || cfg[2] >= cfg[1] || (nTables && !tables)) return 0;
    ShootMerge m(cfg[0], cfg[1], cfg[3], cfg[4] != 0, cfg[5], cfg[6], cfg[7]);
    size_t n = 0;
    auto put = [&](uint64_t v) { if (n < cap) out[n] = v; ++n; };
    auto putAll = [&](const auto &v) { put(v.size()); for (auto x : v) put((uint64_t)x); };
    put(0);
    uint32_t rounds = 0;
    for (; rounds < nTables && m.anyLive(); ++rounds) {
        const ShootAppends &a = m.round(tables + rounds * m.rowWords() * m.R, cfg[2]);
        for (uint64_t v : {(uint64_t)(int64_t)m.status, (uint64_t)m.nshot, m.nVolume, m.nCaustic, m.nDirect, m.nIndirect, m.nRadTotal, (uint64_t)m.nCausticPaths,
                           (uint64_t)m.nDirectPaths, (uint64_t)m.nIndirectPaths, (uint64_t)m.abortTasks, (uint64_t)m.stallRounds}) put(v);
        putAll(m.flags); putAll(a.vTask); putAll(a.vCount); putAll(a.vOff); putAll(a.vNshot);
        putAll(a.sTask); putAll(a.sN); putAll(a.sTake); putAll(a.sRad); putAll(a.sOff);
    }
    if (cap) out[0] = rounds;
    for (const Plan &p : m.plan) { putAll(p.src); putAll(p.local); putAll(p.global); putAll(p.localRows); put(p.rows); }
    return n;
}

namespace {
typedef ncclResult_t (*nccl_allgather_fn)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);

// One all-gather: every rank gives `bytes` bytes and receives n_ranks x bytes, rank-major.  Host exchanges (count rows, status,
// counters) stage through device memory on the RCCL branch; device exchanges (photon rows) stage through host memory on the
// callback branch only.  With no communicator a host exchange is an untimed copy and no device exchange takes place.
struct Exchange {
    const pvol_shoot_comm *comm = 0;   // 0: the single-GPU shoot, rank 0 of 1
    nccl_allgather_fn gather = 0;
    uint32_t nRanks = 1;
    DevPtr<unsigned char> dStage;
    size_t dStageBytes = 0;
    std::vector<unsigned char> hSend, hRecv;
    double seconds = 0.0;
    bool nccl(const void *dSend, void *dRecv, size_t bytes) {
        return gather(dSend, dRecv, bytes, ncclUint8, (ncclComm_t)comm->nccl_comm, 0) == ncclSuccess && ok(hipStreamSynchronize(0));
    }
    bool host(const void *send, void *recv, size_t bytes) {
        if (!comm) { memcpy(recv, send, bytes); return true; }
        const auto t0 = std::chrono::steady_clock::now();
        bool good;
        if (gather) {
            const size_t need = bytes * (nRanks + 1);
            if (need > dStageBytes && !(dStageBytes = dStage.alloc(need) ? need : 0)) return false;
            unsigned char *ds = dStage.get();
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

// One store of the shoot (volume, caustic, direct, indirect or radiance, in ShootMerge's order): this rank's rows in global merge
// order, one array per field (p, wi|wo, alpha; or the radiance record) of `width` floats a row.  ShootMerge::plan has every rank's rows.
struct Store {
    int nFields;
    uint32_t width[3];
    DevArr f[3];
    bool reserve(uint64_t rows) {   // room for this rank's rows of the plan, keeping those merged before
        for (int i = 0; i < nFields; ++i)
            if (!f[i].resize(width[i] * rows)) return false;
        return true;
    }
};

template <class T> bool upload(T *dst, const std::vector<T> &v) { return ok(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice)); }

// All-gathers every rank's local rows of one store and places them in global order into freshly allocated dst[f]
// ([plan.rows][width]).  All ranks call it with the same plan, hence the same sizes, and all return the same code unless the
// exchange itself fails (PVOL_E_NO_DEVICE).  With no communicator the rank's own arrays are the store and move to dst.
int gather_store(Exchange &X, Store &s, const Plan &plan, uint32_t rank, DevPtr<float> *dst) {
    if (!X.comm) for (int f = 0; f < s.nFields; ++f) dst[f] = std::move(s.f[f].d);
    if (!X.comm || !plan.rows) return PVOL_OK;
    const uint64_t M = plan.most(), mine = plan.localRows[rank];
    uint32_t rowWords = 0;
    for (int f = 0; f < s.nFields; ++f) rowWords += s.width[f];
    const size_t sendFloats = (size_t)M * rowWords;
    // the plan's bounds, checked before any device index is formed from it
    for (size_t i = 0; i < plan.src.size(); ++i) {
        const uint64_t end = i + 1 < plan.src.size() ? plan.global[i + 1] : plan.rows;
        if (plan.src[i] >= X.nRanks || (uint64_t)plan.local[i] + (end - plan.global[i]) > plan.localRows[plan.src[i]]) return PVOL_E_INVALID;
    }
    DevPtr<float> send, recv;
    DevPtr<uint32_t> dSeg;
    const size_t nSeg = plan.src.size();
    int rc = PVOL_OK;
    if (!send.alloc(sendFloats) || !recv.alloc(sendFloats * X.nRanks) || !dSeg.alloc(3 * nSeg)) rc = PVOL_E_NO_MEMORY;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f)
        if (!dst[f].alloc((size_t)plan.rows * s.width[f])) rc = PVOL_E_NO_MEMORY;
    uint64_t fieldOff = 0;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f) {   // the rank's block: field f's M x width floats, then the next field
        if (mine && !ok(hipMemcpy(send.get() + fieldOff, s.f[f].d.get(), sizeof(float) * (size_t)mine * s.width[f], hipMemcpyDeviceToDevice))) rc = PVOL_E_NO_DEVICE;
        fieldOff += M * s.width[f];
    }
    if (rc == PVOL_OK && !(upload(dSeg.get(), plan.src) && upload(dSeg.get() + nSeg, plan.local) && upload(dSeg.get() + 2 * nSeg, plan.global) && ok(hipDeviceSynchronize())))
        rc = PVOL_E_NO_DEVICE;
    // every rank says whether its buffers are ready before any row moves: a rank that failed above must not leave the others
    // waiting in the collective, nor enter it without buffers
    const uint32_t status = (uint32_t)rc;
    std::vector<uint32_t> all(X.nRanks);
    if (!X.host(&status, all.data(), sizeof(status))) rc = PVOL_E_NO_DEVICE;
    for (uint32_t r = 0; r < X.nRanks && rc == PVOL_OK; ++r) rc = (int)(int32_t)all[r];
    if (rc == PVOL_OK && !X.device(send.get(), recv.get(), sizeof(float) * sendFloats)) rc = PVOL_E_NO_DEVICE;
    fieldOff = 0;
    for (int f = 0; f < s.nFields && rc == PVOL_OK; ++f) {
        PlaceArgs P;
        P.recv = recv.get(); P.rankStride = M * rowWords; P.fieldOff = fieldOff; P.width = s.width[f];
        P.segSrc = dSeg.get(); P.segLocal = dSeg.get() + nSeg; P.segGlobal = dSeg.get() + 2 * nSeg; P.nSeg = (uint32_t)nSeg; P.nRows = plan.rows; P.dst = dst[f].get();
        if (!ok(pvol_launch_place_rows(&P, 0))) rc = PVOL_E_NO_DEVICE;
        fieldOff += M * s.width[f];
    }
    if (rc == PVOL_OK && !ok(hipDeviceSynchronize())) rc = PVOL_E_NO_DEVICE;
    if (rc != PVOL_OK) for (int f = 0; f < s.nFields; ++f) dst[f].reset();
    return rc;
}

// This rank's taken volume rows of a round go to its volume store, alpha / running nshot (pvol_launch_merge).  The segment tables
// live in B.seg at multiples of Ls, the rank's slots: 3 Ls words here, the 8 Ls of the surface merge behind them.
int merge_volume(const ShootArgs &A, const Buffers &B, uint32_t Ls, const ShootAppends &a, Store &s, uint64_t rows) {
    if (!s.reserve(rows)) return PVOL_E_NO_MEMORY;
    uint32_t *d = B.seg.get();
    MergeArgs M;
    M.localPhotons = A.localPhotons; M.cap = A.cap; M.srcTask = d; M.count = d + Ls; M.dstOff = d + 2 * (size_t)Ls; M.nshot = B.segNshot.get();
    M.nSeg = (uint32_t)a.vTask.size(); M.p = s.f[0].d.get(); M.wi = s.f[1].d.get(); M.alpha = s.f[2].d.get();
    return upload(d, a.vTask) && upload(d + Ls, a.vCount) && upload(d + 2 * (size_t)Ls, a.vOff) && upload(B.segNshot.get(), a.vNshot) &&
           ok(pvol_launch_merge(&M, 0)) && ok(hipDeviceSynchronize()) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

// ... and its surface records and radiance photons to stores S[1..4] (pvol_launch_merge_surface)
int merge_surface(const ShootArgs &A, const Buffers &B, uint32_t Ls, const ShootAppends &a, Store *S, const Plan *plan, uint32_t rank) {
    for (int k = 1; k < 5; ++k)
        if (!S[k].reserve(plan[k].localRows[rank])) return PVOL_E_NO_MEMORY;
    uint32_t *d = B.seg.get() + 3 * (size_t)Ls;
    SurfMergeArgs M;
    M.localSurf = A.localSurf; M.localSurfKind = A.localSurfKind; M.capS = A.capS; M.localRad = A.localRad; M.capR = A.capR;
    M.srcTask = d; M.nSurf = d + Ls; M.take = d + 2 * (size_t)Ls; M.nRad = d + 3 * (size_t)Ls; M.dstOff = d + 4 * (size_t)Ls; M.nSeg = (uint32_t)a.sTask.size();
    for (int k = 0; k < 3; ++k) { M.p[k] = S[1 + k].f[0].d.get(); M.wo[k] = S[1 + k].f[1].d.get(); M.alpha[k] = S[1 + k].f[2].d.get(); }
    M.rad = S[4].f[0].d.get();
    return upload(d, a.sTask) && upload(d + Ls, a.sN) && upload(d + 2 * (size_t)Ls, a.sTake) && upload(d + 3 * (size_t)Ls, a.sRad) &&
           upload(d + 4 * (size_t)Ls, a.sOff) && ok(pvol_launch_merge_surface(&M, 0)) && ok(hipDeviceSynchronize()) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

// The rounds of the shoot on this rank: while the merge finds a task live, shoot one block per live task of the rank's own (redone with larger
// pools if a block outgrew one), exchange the count rows, merge, append the rank's taken rows to S.  Returns PVOL_OK or the code the ranks agreed
// on at an exchange; *localRcOut: this rank's own error not yet told to the others; st: its work counters.  The pools and round tables live only here.
int shoot_rounds(pvol_ctx *c, uint32_t rank, Exchange &X, ShootMerge &merge, Store *S, unsigned long long *st, int *localRcOut) {
    const uint32_t T = merge.T, R = merge.R;
    const bool keep = merge.keep;
    const size_t SW = pvol_shoot_state_words();
    uint32_t L = 0;   // this rank's tasks: ids[i] = rank + i * R lives in slot i
    pvol_partition_tasks(T, rank, R, 0, 0, &L);
    std::vector<uint32_t> ids(L);
    pvol_partition_tasks(T, rank, R, ids.data(), L, &L);
    const uint32_t Ls = std::max<uint32_t>(L, 1);
    // Room for one block of one task.  Spectral splitting stores up to ~3 photons per path but the usual yield is
    // ~10 photons per 4096-path block, so the pools start small (L x 256 x 144 B) and a round in which some task outgrew
    // one is REDONE with a larger pool from the saved RNG states (the round is a pure function of them): nothing is dropped
    // and nothing is sized for the worst case.
    uint32_t capMax = (uint32_t)std::min<size_t>(65536, std::max<size_t>(256, ((size_t)48 << 30) / ((size_t)Ls * 144)));
    const ShootKnobs knobs = pvol_env_shoot(pvol_env_get);   // test knobs, a positive value lowers (pvol_env.h)
    capMax = env_lowered(capMax, knobs.rankCapMax);
    uint32_t cap = std::min<uint32_t>(256, capMax), capS = keep ? std::min<uint32_t>(256, capMax) : 1, capR = keep ? 64 : 1;
    cap = env_lowered(cap, knobs.poolStart); capS = env_lowered(capS, knobs.poolStart); capR = env_lowered(capR, knobs.poolStart);
    Buffers B;
    int &localRc = *localRcOut;   // reported to all at the next exchange
    if (!(B.stateA.alloc(SW * Ls) && B.stateB.alloc(SW * Ls) && B.halton.alloc(48 * (size_t)Ls) && B.flags.alloc(Ls) && B.localCounts.alloc(8 * (size_t)Ls) &&
          B.photons(cap, Ls) && B.stats.alloc(8) && B.surface(capS, Ls) && B.radiance(capR, Ls) && B.seg.alloc(11 * (size_t)Ls) && B.segNshot.alloc(Ls) &&
          (!X.comm || B.taskIds.alloc(Ls)) && ok(hipMemset(B.stats.get(), 0, sizeof(unsigned long long) * 8))))
        localRc = PVOL_E_NO_MEMORY;

    ShootArgs A;
    A.scene = c->ds.get(); A.shoot = c->dsh.get(); A.nTasks = L; A.stateIn = B.stateA.get(); A.stateOut = B.stateA.get(); A.halton = B.halton.get(); A.flags = B.flags.get();
    A.localCounts = B.localCounts.get(); A.stats = B.stats.get(); A.init = 1; A.keepSurface = keep ? 1 : 0;
    const auto pointPools = [&] {
        A.localPhotons = B.localPhotons.get(); A.cap = cap;
        A.localSurf = B.localSurf.get(); A.localSurfKind = B.localSurfKind.get(); A.capS = capS; A.localRad = B.localRad.get(); A.capR = capR;
    };
    pointPools();
    A.gridVolume = is_density_region(c->hs.volKind) ? 1 : 0; A.blockPaths = merge.blockPaths;
    // the shooter's compilation for the medium's Density() (pvol_region_exp.h)
    const auto launchShoot = c->hs.volKind == PVOL_VOLUME_EXPONENTIAL ? pvol_launch_shoot_exp : pvol_launch_shoot;
    A.taskIds = B.taskIds.get();   // null with no communicator: slot == task
    if (localRc == PVOL_OK && L && !((!X.comm || ok(hipMemcpy(B.taskIds.get(), ids.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice))) &&
                                     ok(launchShoot(&A, 0)) && ok(hipDeviceSynchronize())))
        localRc = PVOL_E_NO_DEVICE;
    A.init = 0; A.stateOut = B.stateB.get();

    std::vector<uint32_t> localFlags(Ls);
    // exchanged per round: a status word, then the count rows of the rank's slots (read there from the device), padded to Lpad rows
    const size_t rowWords = merge.rowWords();
    std::vector<uint32_t> sendRow(rowWords), table(rowWords * R);
    uint32_t *const localCounts = &sendRow[1];
    bool redo = false;
    // A pool some block outgrew (`most` > `have`): a larger one by the pools' growth rule, at most `limit` (the radiance pool has no
    // ceiling of its own), ShootArgs pointed at it, and the round is redone
    const auto regrow = [&](uint32_t most, uint32_t &have, uint32_t limit, bool (Buffers::*pool)(size_t, size_t)) {
        if (most <= have) return true;
        if (most > limit) { localRc = PVOL_E_LIMIT; return false; }
        have = std::min<uint32_t>(limit, std::max<uint32_t>(most + most / 4, have * 4));
        if (!(B.*pool)(have, L)) { localRc = PVOL_E_NO_MEMORY; return false; }
        pointPools();
        redo = true;
        return true;
    };
    while (merge.anyLive()) {
        for (uint32_t i = 0; i < L; ++i) localFlags[i] = merge.flags[ids[i]];
        if (localRc == PVOL_OK && L && !ok(hipMemcpy(B.flags.get(), localFlags.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice))) localRc = PVOL_E_NO_DEVICE;
        do {   // the rank's own round: one block per live task, redone from the same states if one of its blocks outgrew a pool
            redo = false;
            if (localRc != PVOL_OK || !L) break;
            unsigned long long rs[8];
            if (!ok(hipMemset(B.stats.get(), 0, sizeof(rs))) || !ok(launchShoot(&A, 0)) ||
                !ok(hipMemcpy(localCounts, B.localCounts.get(), sizeof(uint32_t) * 8 * (size_t)L, hipMemcpyDeviceToHost)) ||
                !ok(hipMemcpy(rs, B.stats.get(), sizeof(rs), hipMemcpyDeviceToHost))) { localRc = PVOL_E_NO_DEVICE; break; }
            uint32_t most = 0, mostS = 0, mostR = 0;
            for (uint32_t i = 0; i < L; ++i) {
                if (localFlags[i] & 8u) continue;
                if (!(localFlags[i] & 4u)) most = std::max(most, localCounts[8 * (size_t)i]);
                mostS = std::max(mostS, localCounts[8 * (size_t)i + 4]);
                mostR = std::max(mostR, localCounts[8 * (size_t)i + 5]);
            }
            if (!regrow(most, cap, capMax, &Buffers::photons) ||
                (keep && !(regrow(mostS, capS, capMax, &Buffers::surface) && regrow(mostR, capR, UINT32_MAX, &Buffers::radiance)))) break;
            if (!redo) for (int i = 0; i < 8; ++i) st[i] += rs[i];
        } while (redo);
        if (localRc == PVOL_OK && L) { const uint32_t *tmp = A.stateIn; A.stateIn = A.stateOut; A.stateOut = const_cast<uint32_t *>(tmp); }   // the round stands
        // the count exchange: every rank learns the round's whole table and whether any rank failed (the lowest-ranked nonzero status)
        sendRow[0] = (uint32_t)localRc;
        if (!X.host(sendRow.data(), table.data(), sizeof(uint32_t) * rowWords)) return PVOL_E_NO_DEVICE;
        for (uint32_t r = 0; r < R; ++r) if (table[r * rowWords]) return (int)(int32_t)table[r * rowWords];
        // merge in task order on the whole round's table: every rank takes the same decisions
        const ShootAppends &a = merge.round(table.data(), rank);
        if (localRc == PVOL_OK && !a.vTask.empty()) localRc = merge_volume(A, B, Ls, a, S[0], merge.plan[0].localRows[rank]);
        if (localRc == PVOL_OK && keep && !a.sTask.empty()) localRc = merge_surface(A, B, Ls, a, S, merge.plan, rank);
    }
    return PVOL_OK;
}

int shoot(pvol_ctx *c, uint32_t n_tasks, uint32_t block_paths, uint32_t rank, Exchange &X) {
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    pvol_free_photons(c);
    pvol_free_surface_stores(c);
    memset(c->shootStats, 0, sizeof(c->shootStats));
    c->prepSeconds[0] = c->prepSeconds[1] = c->exchangeSeconds = 0.0;
    if (c->hs.nLights == 0) return pvol_push_scene(c);   // photonshooter.cpp:459: decided by the scene, the same on every rank
    int rc = pvol_push_scene(c);
    if (rc != PVOL_OK) return rc;

    const auto tShoot0 = std::chrono::steady_clock::now();
    const uint32_t R = X.nRanks;
    const pvol_params &P = c->params;
    const bool keep = P.keep_surface_photons != 0;
    ShootMerge merge(n_tasks, R, block_paths, keep, P.n_caustic_photons, P.n_indirect_photons, P.n_volume_photons);
    Store S[5] = {{3, {3, 3, 30}}, {3, {3, 3, 30}}, {3, {3, 3, 30}}, {3, {3, 3, 30}}, {1, {8}}};   // volume, caustic, direct, indirect, radiance
    unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int localRc = PVOL_OK;   // this rank's own error
    rc = shoot_rounds(c, rank, X, merge, S, st, &localRc);
    if (rc == PVOL_OK) rc = merge.status;
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
    const uint64_t nVolume = merge.nVolume;
    // paths, follow_calls, no_hit, march_steps, interactions, absorbed, stored_volume, caustic, direct, indirect, split_children, nshot
    const uint64_t stats[12] = {st[0], st[1], st[2], st[3], st[4], st[5], nVolume, merge.nCaustic, merge.nDirect, merge.nIndirect, st[6], merge.nshot};
    memcpy(c->shootStats, stats, sizeof(stats));
    if (rc == PVOL_OK && st[7] != 0) rc = PVOL_E_LIMIT;   // a frame stack overflowed on some rank: never silently drop photons
    // the stores: every rank's rows placed in global merge order; the surface stores go to the context whatever happens to the volume map
    if (rc == PVOL_OK && keep) {
        const uint64_t cnt[3] = {merge.nCaustic, merge.nDirect, merge.nIndirect};
        const uint32_t paths[3] = {merge.nCausticPaths, merge.nDirectPaths, merge.nIndirectPaths};
        for (int k = 0; k < 3 && rc == PVOL_OK; ++k) {
            DevPtr<float> dst[3];
            rc = gather_store(X, S[1 + k], merge.plan[1 + k], rank, dst);
            if (rc == PVOL_OK && merge.plan[1 + k].rows != cnt[k]) rc = PVOL_E_INVALID;
            c->surf[k].p = std::move(dst[0]); c->surf[k].wo = std::move(dst[1]); c->surf[k].alpha = std::move(dst[2]);
            c->surf[k].n = (uint32_t)cnt[k]; c->surf[k].nPaths = paths[k];
        }
        if (rc == PVOL_OK) rc = gather_store(X, S[4], merge.plan[4], rank, &c->dRad);
        if (rc == PVOL_OK && merge.plan[4].rows != merge.nRadTotal) rc = PVOL_E_INVALID;
        c->nRad = (uint32_t)merge.nRadTotal;
        c->surfKept = true;
        if (rc != PVOL_OK) pvol_free_surface_stores(c);
    }
    DevPtr<float> raw[3];
    if (rc == PVOL_OK && nVolume) {
        rc = gather_store(X, S[0], merge.plan[0], rank, raw);
        if (rc == PVOL_OK && merge.plan[0].rows != nVolume) rc = PVOL_E_INVALID;
    }
    for (Store &s : S)
        for (DevArr &a : s.f) a.d.reset();   // the rank-local arrays go before the build allocates
    c->prepSeconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - tShoot0).count();
    c->exchangeSeconds = X.seconds;
    if (rc != PVOL_OK || nVolume == 0) return rc;
    // hand the merged arrays to the context and build the search structure
    std::vector<float> hostP(3 * nVolume);
    if (!ok(hipMemcpy(hostP.data(), raw[0].get(), sizeof(float) * 3 * nVolume, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
    c->dRawP = std::move(raw[0]); c->dRawWi = std::move(raw[1]); c->dRawAlpha = std::move(raw[2]);
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
