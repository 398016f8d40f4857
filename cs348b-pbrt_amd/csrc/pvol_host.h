// pvol_host.h -- host-side internals shared by every unit with host code: the owners of device memory, events, streams and pinned memory, the context, the
// kernels' launchers, the plans and the test entries that are no part of include/pvol.h
#ifndef PVOL_HOST_H
#define PVOL_HOST_H
#include <hip/hip_runtime.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <vector>
#include "pvol_dev.h"
#include "pvol_env.h"
#include "pvol_rays_plan.h"

static bool ok(hipError_t e) { return e == hipSuccess; }

#define PVOL_LOCAL __attribute__((visibility("hidden")))   // shared by the host units, not an export of the library

// The one owner of a device allocation: move-only, freed by its destructor.  alloc() frees what it held; a failed hipMalloc leaves
// it empty and HIP's last error cleared.
template <class T> struct PVOL_LOCAL DevPtr {
    DevPtr() {}
    DevPtr(DevPtr &&o) : p(o.release()) {}
    DevPtr &operator=(DevPtr &&o) { reset(o.release()); return *this; }
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { reset(); }
    bool alloc(size_t count) {
        reset();
        if (hipMalloc(&p, sizeof(T) * count) == hipSuccess) return true;
        p = 0; (void)hipGetLastError();
        return false;
    }
    T *get() const { return p; }
    T *release() { T *q = p; p = 0; return q; }
    void reset(T *q = 0) { if (p) hipFree(p); p = q; }
private:
    T *p = 0;
};

// The one owner of a HIP handle: move-only, 0 until the deriving owner makes it, given to Free by the destructor.
template <class H, hipError_t (*Free)(H)> struct PVOL_LOCAL DevHandle {
    DevHandle() {}
    DevHandle(DevHandle &&o) : h(o.h) { o.h = 0; }
    DevHandle &operator=(DevHandle &&o) { std::swap(h, o.h); return *this; }
    DevHandle(const DevHandle &) = delete;
    DevHandle &operator=(const DevHandle &) = delete;
    ~DevHandle() { reset(); }
    H get() const { return h; }
    void reset() { if (h) Free(h); h = 0; }
protected:
    H h = 0;
};
// An event, created on first use: for ordering only, or (timing) one that hipEventElapsedTime accepts.
struct PVOL_LOCAL DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
    bool create(bool timing = false) {
        if (h || ok(timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming))) return true;
        h = 0;
        return false;
    }
};
// A blocking stream (ordered behind the null stream), created on first use.
struct PVOL_LOCAL DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
    bool create() {
        if (h || ok(hipStreamCreate(&h))) return true;
        h = 0;
        return false;
    }
};
// Pinned host memory.  alloc() frees what it held; a failed hipHostMalloc leaves it empty and HIP's last error cleared.
struct PVOL_LOCAL PinnedBuf : DevHandle<void *, hipHostFree> {
    bool alloc(size_t bytes) {
        reset();
        if (hipHostMalloc(&h, bytes, hipHostMallocDefault) == hipSuccess) return true;
        h = 0; (void)hipGetLastError();
        return false;
    }
    unsigned char *get() const { return (unsigned char *)h; }
};

// What lets a call on any stream reuse scratch of the context behind the previous call's kernels: wait() in front of
// the first reserve, record() behind the last launch.  Both false on a HIP error.
struct PVOL_LOCAL ScratchFence {
    bool wait(hipStream_t stream) { return ev.get() ? ok(hipStreamWaitEvent(stream, ev.get(), 0)) : ev.create(); }
    bool record(hipStream_t stream) { return ok(hipEventRecord(ev.get(), stream)); }
private:
    DevEvent ev;
};

// The device copies of one host-array call: move-only, freed by its destructor.  in / out / inout allocate the copy of
// `count` items and register its upload / copy-back / both, scratch only allocates; a NULL host array gives a NULL device pointer and
// nothing to copy.  upload(): PVOL_E_NO_MEMORY if any allocation failed, before anything is uploaded; either copy loop runs in the
// order of registration and returns PVOL_E_NO_DEVICE at the first failure.  download() is the only place the caller's arrays are
// written: the entry point calls it once everything ran.
struct PVOL_LOCAL HostStage {
    HostStage() {}
    HostStage(HostStage &&) = default;
    HostStage &operator=(HostStage &&) = default;
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    template <class T> T *in(const T *host, size_t count) { return host ? (T *)add((void *)host, sizeof(T) * count, UP) : 0; }
    template <class T> T *out(T *host, size_t count) { return host ? (T *)add(host, sizeof(T) * count, DOWN) : 0; }
    template <class T> T *inout(T *host, size_t count) { return host ? (T *)add(host, sizeof(T) * count, UP | DOWN) : 0; }
    template <class T> T *scratch(size_t count) { return (T *)add(0, sizeof(T) * count, 0); }
    int upload() const { return noMemory ? PVOL_E_NO_MEMORY : copy(UP); }
    int download() const { return copy(DOWN); }
private:
    enum { UP = 1, DOWN = 2 };
    struct Item { DevPtr<unsigned char> d; void *host; size_t bytes; int dir; };
    std::vector<Item> items;
    bool noMemory = false;
    void *add(void *host, size_t bytes, int dir) {
        Item it;
        if (!it.d.alloc(bytes)) { noMemory = true; return 0; }
        it.host = host; it.bytes = bytes; it.dir = dir;
        items.push_back(std::move(it));
        return items.back().d.get();
    }
    int copy(int dir) const {
        for (const Item &it : items)
            if ((it.dir & dir) && !ok(dir == UP ? hipMemcpy(it.d.get(), it.host, it.bytes, hipMemcpyHostToDevice)
                                                : hipMemcpy(it.host, it.d.get(), it.bytes, hipMemcpyDeviceToHost)))
                return PVOL_E_NO_DEVICE;
        return PVOL_OK;
    }
};

// Items per slice of a sliced entry point: as many as keep `bytesPerItem` each within `bound` bytes (0 or more than `cap`: that),
// whole runs of 64 where that many fit, never fewer than one.
static inline uint32_t pvol_slice_items(uint64_t bound, uint64_t cap, uint64_t bytesPerItem) {
    if (!bound || bound > cap) bound = cap;
    uint64_t n = bound / bytesPerItem;
    if (n >= 64) n -= n % 64;
    return (uint32_t)std::max<uint64_t>(n, 1);
}

// ---- kernels' host entry points (pvol_march.hip, pvol_grid.hip)
#include "pvol_liargs.h"
struct GridBuildArgs {
    const float *p;      // n x 3 (upload order)
    const float *wi;     // n x 3
    const float *alpha;  // n x 30
    uint32_t n;
    float lo[3];
    float inv;
    int32_t gdim[3];
    int32_t sub;         // 1, or 4: sort by (cell, 4x4x4 sub-cell) and fill subStart
    // volume (for the Inside() test of HomogeneousVolumeDensity::p, volumes/homogeneous.h:76-79)
    int32_t volKind;
    float extLo[3], extHi[3];
    float w2v[16];
};
extern "C" hipError_t pvol_launch_li_seq(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, hipStream_t stream);
extern "C" hipError_t pvol_launch_li_slice(const LiArgs *args, size_t ldsResolve, size_t ldsReplay, int candCap, bool stats,
                                           uint32_t nWaves, hipStream_t stream, bool resolve, int groupForm, size_t ldsGroup, uint32_t nGroupWaves,
                                           uint32_t nFixWaves);
extern "C" size_t pvol_group_lds_bytes(int candCap);
extern "C" hipError_t pvol_launch_li_group(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, uint32_t nWaves, uint32_t nFixWaves,
                                           int replay, hipStream_t stream);
extern "C" hipError_t pvol_launch_spec_compose(const SpecComposeArgs *a, hipStream_t stream);
extern "C" hipError_t pvol_launch_spec_fill(pvol_ray *rays, uint32_t n, hipStream_t stream);
extern "C" hipError_t pvol_launch_li_replay(const LiArgs *args, size_t ldsReplay, int candCap, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_surface(const SurfArgs *a, uint32_t nWaves, hipStream_t stream);
extern "C" size_t pvol_tile_lds_bytes(int maxSteps, uint32_t spp, bool fused, int nTris, bool shadowRows);
extern "C" hipError_t pvol_launch_tile(const LiArgs *args, const TileArgs *tile, bool fused, size_t ldsBytes, int candCap, hipStream_t stream, int wavesPerTask,
                                       bool plain, const char **form);
extern "C" hipError_t pvol_launch_li_par(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_lphoton_points(const PointsArgs *args, int candCap, uint32_t nWaves, hipStream_t stream);
// pvol_radiance_batch* (pvol_rays_dev.h, first compilation only: none of them evaluates a density).  count: the members of every block;
// emit: the blocks, and the slice's stream table `st` rewritten onto the expanded array (`continued`: the caller's entry of the stream
// an earlier slice began, or 0); patch: in front of surface_kernel; compose: the fold, and the end_draws into the caller's table
extern "C" hipError_t pvol_launch_rays_count(const RaysArgs *a, hipStream_t stream);
extern "C" hipError_t pvol_launch_rays_emit(const RaysArgs *a, pvol_stream *st, uint32_t nStreams, const pvol_stream *continued, hipStream_t stream);
extern "C" hipError_t pvol_launch_rays_patch(const RaysArgs *a, hipStream_t stream);
extern "C" hipError_t pvol_launch_rays_compose(const RaysArgs *a, const pvol_stream *st, uint32_t nStreams, pvol_stream *caller, hipStream_t stream);
// VolumeIntegrator "single" (pvol_single.hip): the sequential form (one wave per stream; ldsBytes = BatchPlan::ldsResolve) and
// the ray-parallel one (one wave per ray, one march step per lane; chunkCounter and needSeq zeroed by the caller)
extern "C" hipError_t pvol_launch_single_seq(const LiArgs *args, size_t ldsBytes, hipStream_t stream);
extern "C" hipError_t pvol_launch_single_par(const LiArgs *args, uint32_t nWaves, hipStream_t stream);
// The launchers of one compilation of the marching kernels: VolumeGridDensity (and every medium that is no density region) or, from
// pvol_march_exp.hip, ExponentialDensity (pvol_region_exp.h).  The host asks pvol_launchers(kind) wherever a launched kernel may
// evaluate a density; launchers that never do (spec_compose, spec_fill) are called directly.
struct RegionLaunchers {
    decltype(&pvol_launch_li_seq) liSeq;
    decltype(&pvol_launch_li_slice) liSlice;
    decltype(&pvol_launch_li_group) liGroup;
    decltype(&pvol_launch_li_replay) liReplay;
    decltype(&pvol_launch_li_par) liPar;
    decltype(&pvol_launch_surface) surface;
    decltype(&pvol_launch_tile) tile;
    decltype(&pvol_launch_lphoton_points) lphotonPoints;
    decltype(&pvol_launch_single_seq) singleSeq;
    decltype(&pvol_launch_single_par) singlePar;
};
#if !PVOL_REGION_EXP   /* undefined or 0: the first compilation and the host units */
extern "C" hipError_t pvol_launch_li_seq_exp(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, hipStream_t stream);
extern "C" hipError_t pvol_launch_li_slice_exp(const LiArgs *args, size_t ldsResolve, size_t ldsReplay, int candCap, bool stats,
                                               uint32_t nWaves, hipStream_t stream, bool resolve, int groupForm, size_t ldsGroup, uint32_t nGroupWaves,
                                               uint32_t nFixWaves);
extern "C" hipError_t pvol_launch_li_group_exp(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, uint32_t nWaves, uint32_t nFixWaves,
                                               int replay, hipStream_t stream);
extern "C" hipError_t pvol_launch_li_replay_exp(const LiArgs *args, size_t ldsReplay, int candCap, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_li_par_exp(const LiArgs *args, size_t ldsBytes, int candCap, bool stats, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_surface_exp(const SurfArgs *a, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_tile_exp(const LiArgs *args, const TileArgs *tile, bool fused, size_t ldsBytes, int candCap, hipStream_t stream,
                                           int wavesPerTask, bool plain, const char **form);
extern "C" hipError_t pvol_launch_lphoton_points_exp(const PointsArgs *args, int candCap, uint32_t nWaves, hipStream_t stream);
extern "C" hipError_t pvol_launch_single_seq_exp(const LiArgs *args, size_t ldsBytes, hipStream_t stream);
extern "C" hipError_t pvol_launch_single_par_exp(const LiArgs *args, uint32_t nWaves, hipStream_t stream);
static inline const RegionLaunchers &pvol_launchers(int volKind) {
    static const RegionLaunchers base = {pvol_launch_li_seq, pvol_launch_li_slice, pvol_launch_li_group, pvol_launch_li_replay, pvol_launch_li_par,
                                         pvol_launch_surface, pvol_launch_tile, pvol_launch_lphoton_points, pvol_launch_single_seq, pvol_launch_single_par};
    static const RegionLaunchers expo = {pvol_launch_li_seq_exp, pvol_launch_li_slice_exp, pvol_launch_li_group_exp, pvol_launch_li_replay_exp,
                                         pvol_launch_li_par_exp, pvol_launch_surface_exp, pvol_launch_tile_exp, pvol_launch_lphoton_points_exp,
                                         pvol_launch_single_seq_exp, pvol_launch_single_par_exp};
    return volKind == PVOL_VOLUME_EXPONENTIAL ? expo : base;
}
#endif
extern "C" hipError_t pvol_build_grid(const GridBuildArgs *args, float4 *pos4, float4 *alpha4, float4 *wi4,
                                      uint32_t *cellStart, uint32_t *subStart, hipStream_t stream);
extern "C" hipError_t pvol_build_bvh(const float *dTri, const int32_t *dMat, const int32_t *dFlip, uint32_t n, float pad, float4 *tris,
                                     float4 *nodes, hipStream_t stream);
extern "C" hipError_t pvol_grid_occupancy(const uint32_t *cellStart, uint32_t ncells, double *sumSquares, hipStream_t stream);

#define PVOL_N_PHASES 6
enum { PVOL_PHASE_END = -1, PVOL_PHASE_TILE = 0, PVOL_PHASE_RNG = 1, PVOL_PHASE_MARCH = 2, PVOL_PHASE_SURFACE = 3, PVOL_PHASE_FILM = 4, PVOL_PHASE_OTHER = 5 };

// The context's on-demand device buffers.  pvol_reserve is the one place they are allocated: nothing to do when `want` fits, else it
// waits for `stream` (an earlier batch may still read the old buffer), frees, and allocates exactly `want` bytes.
struct PVOL_LOCAL DevBuf { DevPtr<unsigned char> p; size_t bytes = 0; };
enum {
    PVOL_BUF_RECORDS, PVOL_BUF_STATE,   // resolve/replay: per-step records of a slice, MT state of every stream
    PVOL_BUF_DEFER,                     // li_group_kernel's deferred lookups (DeferRec)
    PVOL_BUF_TAU, PVOL_BUF_SPEC_LINK,   // per sample of a render batch: the T the surface term is attenuated by (TauRec); its segments (one word)
    PVOL_BUF_SEG_RAYS, PVOL_BUF_SEG_INFO, PVOL_BUF_SEG_OUT, PVOL_BUF_SEG_RECORDS,   // segment pool of the specular recursion: rays, SegInfo, 60 floats, records,
    PVOL_BUF_SEG_COUNTER, PVOL_BUF_SEG_STREAM,   // ... its fill counter (16 bytes) and the pool seen as one pvol_stream
    PVOL_BUF_TILE_RAYS, PVOL_BUF_TILE_XY, PVOL_BUF_TILE_OUT, PVOL_BUF_TILE_STREAMS, PVOL_BUF_TILE_WINDOWS,   // render driver (pvol_render_host.hip)
    PVOL_BUF_LI_IN, PVOL_BUF_LI_OUT,    // device staging of the coalesced per-sample batches (pvol_li_coalesce.hip)
    PVOL_BUF_GROUP_STAGE,               // pvol_render_frame_group: the other contexts' films next to the root's
    PVOL_BUF_FG_DIRS, PVOL_BUF_FG_RAYS, // pvol_final_gather* (pvol_final_gather.hip): a slice's direction records and ray records
    PVOL_BUF_LP_ORDER, PVOL_BUF_LP_TEMP, // pvol_lphoton_batch* (pvol_lphoton.hip): a slice's cell keys and slots (pvol_order_points), the sort's own scratch
    // pvol_radiance_batch* (pvol_rays.hip), one slice: the expanded rays, their SegInfo, 60-float rows and draw counts; per caller ray the block
    // sizes and their scan (2 x (n + 1) words) and the primaries' stashed rows; the slice's stream table; the scan's own scratch
    PVOL_BUF_RR_RAYS, PVOL_BUF_RR_INFO, PVOL_BUF_RR_ROWS, PVOL_BUF_RR_DRAWS, PVOL_BUF_RR_COUNT, PVOL_BUF_RR_STASH, PVOL_BUF_RR_STREAMS, PVOL_BUF_RR_TEMP,
    // pvol_radiance_gather_batch* (pvol_rays.hip, pvol_rays_gather.hip), per expanded ray of a slice: its final-gather query (46 floats),
    // its copy of the owner's sample rows (2 x n_samples x 3 floats), Lg (30 floats) and the gather's draws (one word)
    PVOL_BUF_RG_QUERY, PVOL_BUF_RG_U, PVOL_BUF_RG_OUT,
    PVOL_N_BUFS
};
extern "C" bool pvol_reserve(DevBuf &b, size_t want, hipStream_t stream);

// A photon map as the kernels read it (pvol_grid.hip): the photons sorted by cell, the start of every cell and, for a clumpy volume map,
// of every 4 x 4 x 4 sub-cell.  Built by build_photon_grid (pvol_map_host.hip); the volume map and the surface integrator's caustic map are one each.
struct PVOL_LOCAL PhotonGrid {
    DevPtr<float4> pos4, alpha4, wi4;
    DevPtr<uint32_t> cellStart, subStart;   // subStart: second level of a clumpy map, else empty
    DevPtr<float> mom;                      // volume map under a scene that passes pvol_moment_gate: MOM_ROW floats per photon, else empty
    uint32_t n = 0;
    float gridLo[3] = {0.f, 0.f, 0.f}, cellSize = 0.f, invCell = 0.f;
    int32_t gdim[3] = {0, 0, 0};
    size_t cells() const { return (size_t)gdim[0] * gdim[1] * gdim[2]; }
};

// The Inside() test a photon must pass to count (pvol_grid.hip); PVOL_VOLUME_GRID with a zero extent passes every photon.
struct MapFilter { int32_t volKind; float extLo[3], extHi[3], w2v[16]; };
// One map from its raw device arrays raw = {p[n][3], wi[n][3], alpha[n][30]} (n > 0) and the host copy of the positions: cells of
// firstCell(volume of the photons' box), grown until the grid has at most 2^24 of them; every extent of the box at least minExt
// (pvol_map_host.hip).
PVOL_LOCAL int build_photon_grid(PhotonGrid &G, const float *const raw[3], const float *hostP, uint32_t n, double minExt,
                                 const std::function<double(double)> &firstCell, const MapFilter &f);

// What pvol_compute_radiance leaves (pvol_radiance.hip): the radiance photons in input order with their Lo, and the radiance map
// over them -- a PhotonGrid whose wi4 holds the normal and whose 32-float rows hold Lo.
struct PVOL_LOCAL RadianceResult {
    bool have = false;         // a compute succeeded since the last shoot (n may be 0)
    uint32_t n = 0;
    DevPtr<float> p, nrm, lo;  // [n][3], [n][3], [n][30]
    PhotonGrid map;
};

// What pvol_build_gather_map* leaves (pvol_gather.hip): the indirect map as the reference's kd-tree, node by node
// (GatherNode, pvol_gather_tree.h: two float4 a node), and the photons' Photon::wi in the store's order.
struct PVOL_LOCAL GatherMap {
    bool have = false;
    uint32_t n = 0;
    int depth = 0;             // nodes on the longest root-to-leaf path: bounds the lookup's stack
    DevPtr<float4> nodes4;     // [n][2]
    DevPtr<float> wi;          // [n][3]
};

// ---- the parts of a context
// Kernel timing: every batch records a pair of timing events on its launch stream (pvol_launch_batch, harvest_events in pvol_api.hip).
struct PVOL_LOCAL BatchTimer {
    typedef std::pair<DevEvent, DevEvent> Pair;
    std::vector<Pair> pending, pool;   // recorded and not yet folded in; free for the next batch
    double timeMs = 0.0;
    uint64_t launches = 0;
    std::mutex mu;                     // event lists only: these and the phase timer's
    // The pair taken for one batch: to `pending` once the batch is enqueued (done), back to `pool` on every other way out.
    struct Lease {
        BatchTimer &t; Pair ev; bool done = false;
        ~Lease() { std::lock_guard<std::mutex> g(t.mu); (done ? t.pending : t.pool).push_back(std::move(ev)); }
    };
};
// Phase timing of the render driver (pvol_enable_phase_timing): marks on the launch stream, a mark opens phase `id` and closes the one
// before it; PVOL_PHASE_END closes without opening.  Guarded by BatchTimer::mu.
struct PVOL_LOCAL PhaseTimer {
    bool on = false;
    std::vector<std::pair<int, DevEvent> > marks;
    std::vector<DevEvent> pool;
    double ms[PVOL_N_PHASES] = {0, 0, 0, 0, 0, 0};
};
// Coalesced per-sample calls (pvol_li_coalesce.hip): concurrent pvol_li calls queue here, one of them (the leader) runs a batch of up
// to maxBatch of them while the others wait; mu guards the queue, apiMu still guards the batch.
struct PVOL_LOCAL LiCoalescer {
    std::atomic<uint32_t> maxBatch{0};   // <= 1: every pvol_li is its own batch (pvol_li_lone)
    uint32_t maxWaitUs = 0;
    std::mutex mu;
    std::condition_variable done, more;   // a batch finished / a caller joined the queue (an idle leader may wait for it)
    std::deque<struct LiRequest *> queue;
    bool busy = false;                    // a leader is running a batch
    // calls served by coalesced batches, batches, largest batch, calls that queued behind a batch; then, for every batch of
    // pvol_li_many and the coalescer: batches redone call by call (gated backup), calls that failed on their own
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    // persistent staging of the batches (pinned host here, device in pvol_ctx::buf, grown to the largest batch) and the context's own stream
    DevStream stream;
    PinnedBuf hostIn, hostOut;
    uint32_t cap = 0;
};
// What a sliced query path keeps between calls.  bound: its *_set_scratch_bound (tests), bytes of scratch a slice may
// take, 0 = the path's PVOL_*_SCRATCH_BYTES; fence: the end of the last call's kernels, behind which the next call, on whatever stream,
// reuses their scratch.
struct PVOL_LOCAL SliceScratch { uint64_t bound = 0; ScratchFence fence; };

struct pvol_ctx {
    pvol_params params = {};
    int volInt = PVOL_VOLINT_PHOTON;   // pvol_set_volume_integrator: which Li() the batches run (PVOL_VOLINT_*)
    CtxKnobs knobs;          // the environment as pvol_create found it (pvol_env.h)
    int nCU = 256;
    // One batch at a time per context: the launches of a batch share dWords / dCounters and the scratch in `buf`.  Host entry points hold it from upload to copy-back (VolumeIntegrator::Li is called from every
    // SamplerRendererTask thread at once, samplerrenderer.cpp:247); device entry points hold it while they enqueue.
    std::recursive_mutex apiMu;
    // scene
    bool haveScene = false;
    DevScene hs = {};        // host copy
    DevPtr<DevScene> ds;     // device copy
    DevPtr<float> dDensity;
    float maxDensity = 1.f;   // largest density factor of the medium (1 for analytic volumes, max of the grid values)
    // triangle hierarchy of a scene with more than PVOL_MAX_TRIS triangles (pvol_bvh.hip), else empty
    DevPtr<float4> dBvhNodes, dBvhTris;
    std::vector<int32_t> triMatHost;   // material of every triangle of the scene (host copy, any size)
    uint32_t nSceneTris = 0;           // triangles of the scene set last
    DevPtr<float> dTriN;               // pvol_set_triangle_normals: [nSceneTris][9] in the scene's order (hs.triN), else empty
    double bvhBuildMs = 0.0;
    // photon map
    DevPtr<float> dRawP, dRawWi, dRawAlpha;  // upload order (kept for pvol_download_photons)
    PhotonGrid volMap;
    int momentTerms = 0;        // pvol_moment_scene's decision for the scene set last (0: no moment form, volMap.mom stays empty)
    // what the launches of a batch share, and what they report
    DevPtr<DevCounters> dCounters;
    DevPtr<uint32_t> dWords;   // [0] chunk counter of the ray-parallel kernels, [1] needSeq flag, [2] length of the deferred-lookup list, [3] chunk counter of a gated backup kernel
    DevBuf buf[PVOL_N_BUFS];   // scratch grown on demand (pvol_reserve), freed with the context
    bool statsOn = false;
    const char *lastKernel = "";
    const char *lastTileKernel = "";   // pvol_tile_kernel_name: set by the launch itself
    const char *lastTileForm = "";     // pvol_tile_form_name: "plain" / "general", the form of the last tile launch (pvol_tile_plain_gate)
    BatchTimer timer;
    PhaseTimer phases;
    // photon shooter
    DevShootScene hsh = {};
    DevPtr<DevShootScene> dsh;
    uint64_t shootStats[12] = {};
    double exchangeSeconds = 0.0;   // last pvol_preprocess: time in its all-gathers (part of prepSeconds[0]; 0 after pvol_preprocess_blocks)
    double prepSeconds[2] = {0.0, 0.0};   // last pvol_preprocess: shooting (all rounds + merges), search-structure build
    // surface stores of the last pvol_preprocess (kept only with params.keep_surface_photons): kind 0 caustic, 1 direct, 2 indirect
    struct PVOL_LOCAL SurfStore { DevPtr<float> p, wo, alpha; uint32_t n = 0, nPaths = 0; } surf[3];
    bool surfKept = false;   // the last pvol_preprocess ran with keep_surface_photons and left its stores here
    DevPtr<float> dRad;    // radiance photons: [n][8] = p(3) n(3) material index, pad
    uint32_t nRad = 0;
    RadianceResult rad;    // pvol_compute_radiance*: dropped by every shoot and by pvol_free_surface_stores
    GatherMap gather;      // pvol_build_gather_map*: dropped wherever `rad` is
    // the sliced query paths: pvol_final_gather* (PVOL_BUF_FG_*), pvol_lphoton_batch* (PVOL_BUF_LP_*), pvol_radiance_batch* and
    // pvol_radiance_gather_batch* (PVOL_BUF_RR_*, PVOL_BUF_RG_*)
    SliceScratch fg, lp, rr;
    // caustic map of the surface integrator (pvol_set_surface_integrator), same cell layout as the volume map
    PhotonGrid causticMap;
    // ... and its indirect map (pvol_set_surface_integrator_maps: LPhoton(indirectMap) without the final gather), built by the same builder
    PhotonGrid indirectMap;
    // specular recursion of the surface integrator (pvol_spec_dev.h): segments of the camera samples that meet glass
    bool specOn = false;            // the scene holds a specular material and the surface integrator is on
    pvol_stream hSegStream = {};    // the segment pool seen as one stream of a ray batch (host copy of PVOL_BUF_SEG_STREAM)
    LiCoalescer co;
    // pvol_render_frame_group (pvol_group.hip): the event marking this context's film done; as the root, the event after the sum
    // that last read the other films' staging (PVOL_BUF_GROUP_STAGE)
    DevEvent groupFilmEv, groupStageEv;
};

// One per-sample call of a coalesced batch: the caller's buffers, written only when rc ends PVOL_OK.
struct LiRequest {
    const pvol_ray *ray;
    uint32_t *mt;
    int32_t *mti;
    float *Lv, *T;
    int rc;
    bool done;
};
#define PVOL_LI_MAX_WAIT_US 1000u

// Every input of one batch (pvol_launch_batch).  `tile` != 0: the rays do not exist yet -- the tile kernel (pvol_tile_dev.h) generates
// them stream by stream in front of the march.  maxRaysPerStream 0: unknown, read back from the device table where a slice is sized.
struct BatchArgs {
    const pvol_ray *rays; uint32_t nRays; pvol_stream *streams; uint32_t nStreams;
    int outputKind; float *out; uint32_t *draws; const uint32_t *initState; uint32_t *finalState;
    int transOnly; uint32_t maxRaysPerStream; const TileArgs *tile; hipStream_t stream;
    TauRec *tauOut;       // render driver with the surface integrator on: the march kernels also report every sample's *T
    int32_t *status;      // coalesced per-sample batch: per ray PVOL_E_LIMIT (LiArgs::status), a limit fails only its own call
    float *specSurfOut;   // specular recursion: where the composition reports the surface term (debug), or 0
};
extern "C" int pvol_launch_batch(pvol_ctx *c, const BatchArgs &b);
template <class T> static inline T *pvol_buf(const pvol_ctx *c, int which) { return (T *)c->buf[which].p.get(); }

// ---- the plan of a batch: which kernels it takes and every size they need, a pure function of PlanIn.  LaunchKnobs
// (pvol_env.h): the environment knobs read once per launch (pvol_read_knobs).
extern "C" LaunchKnobs pvol_read_knobs();
struct PlanIn {
    int32_t nLights, volKind; float g; uint32_t nPhotons; int32_t nUsed, candCap, maxSteps, nTris;   // medium and map
    int32_t roulette, distant;   // a march step can reach the Russian roulette (roulette_possible); the first light is a distant one
    int32_t forceSeq, noGroup, noLite, statsOn, nCU, groupWavesPerCU, fixWavesPerCU, tileWaves;   // context flags, device shape
    uint32_t nRays, nStreams, maxRays; int32_t hasInit, transOnly, hasTile; uint32_t spp; int32_t specOn, hasTauOut;   // the batch
    // XYZ moments, in what was padding: the scene's gate (pvol_moment_gate: Taylor terms, 0 = keep the 30 bins; the
    // volume map then carries its moment rows), the batch's output is PVOL_OUT_XYZ, PVOL_NO_MOMENTS=1
    int16_t momentTerms; int8_t outXYZ, noMoments;
    LaunchKnobs knobs;
};
enum { PVOL_PATH_PAR, PVOL_PATH_SLICED, PVOL_PATH_SEQ };
enum { PVOL_TILE_NONE, PVOL_TILE_COUNT, PVOL_TILE_GRID_COUNT, PVOL_TILE_FUSED };
struct BatchPlan {
    int32_t rc, path, tile;
    int32_t groupForm;        // li_group_kernel's form: 0 none, 1 homogeneous (PAR: no records), 2 density region (VolumeGrid, exponential),
                              // 3 form 1 of the PAR path summing XYZ moments instead of 30 bins (GRP_FORM_MOMENTS)
    int32_t fixGroup, liteResolve;
    int32_t resolve;          // SLICED: the slice runs its own resolve pass (no FUSED pre-pass wrote the records)
    uint32_t recStride, sliceM, nSlices, nWaves, gWaves, fixWaves; int32_t tileWavesPerTask;
    uint64_t recBytes, stateBytes, deferWant, specCap, ldsSeq, ldsPar, ldsResolve, ldsGroup, ldsTile;
    const char *kernel;       // what pvol_march_kernel_name reports
};
static_assert(sizeof(PlanIn) == 152 && sizeof(BatchPlan) == 136, "tests/test_launch_plan.py mirrors both");
extern "C" size_t pvol_rec_stride(int maxSteps, bool grid);   // bytes of one record slot
extern "C" BatchPlan plan_path(const PlanIn &in);             // everything that needs no maxRays
extern "C" void plan_size(const PlanIn &in, BatchPlan &p);    // the rest, once in.maxRays is known
#define GRP_FORM_MOMENTS 3
// The gate of the tile pre-pass's PLAIN form (pvol_tile_dev.h), a pure function beside plan_path (pvol_api.hip): every input of
// the decision that PlanIn has no room for, its own struct so that PlanIn and BatchPlan keep their sizes.  1 = PLAIN exactly when the batch is
// COUNT mode (BatchPlan::tile) over a homogeneous extent, at least one light and the first one distant, no hierarchy, no spheres, at most
// PVOL_MAX_TRIS triangles (their shadow rows are then in LDS), surface integrator off, no specular link, and PVOL_TILE_GENERAL unset;
// 0 = the general form.  A black light or a black sigma_s does not enter: both forms leave tile_count_draws at the same early return.
struct TilePlainIn {
    int32_t tile;                       // BatchPlan::tile of the batch (PVOL_TILE_*)
    int32_t volKind, nLights, light0Kind;
    int32_t hasBvh, nSpheres, nTris;    // DevScene::bvhNodes != 0, nSpheres, nTris
    int32_t surfOn, specLink;           // DevScene::surf.enabled, TileArgs::specLink != 0 (TileArgs::specOn implies it)
    int32_t tileGeneral;                // PVOL_TILE_GENERAL=1
};
static_assert(sizeof(TilePlainIn) == 40, "tests/test_tile_plain_gate.py mirrors it");
extern "C" int pvol_tile_plain_gate(const TilePlainIn *in);
// The plan of a batch under VolumeIntegrator "single" (DESIGN.md 24), a pure function beside plan_path (pvol_api.hip): no HIP call, no context, no
// environment; its own input struct, as pvol_tile_plain_gate has.  It decides in this order:
//   1. the refusals (rc = PVOL_E_UNSUPPORTED): a rainbow medium; a final gather (pvol_radiance_gather_batch*); then, with a tile (the render
//      driver; pvol_radiance_batch* is held to the same limit): more than one light, a density region, a specular material under the surface integrator, R'
//   2. PVOL_SINGLE_PAR (single_par_kernel): at most one light, a homogeneous extent or no medium, no caller RNG state, PVOL_FORCE_SEQ unset
//      (and, with a tile, !R', which 1. has left)
//   3. PVOL_SINGLE_SEQ (single_seq_kernel) for everything else without a tile -- also where plan_path, fed R' as PlanIn::roulette, answers
//      SLICED, which has no kernel here; with a tile what 2. does not take is refused (PVOL_E_UNSUPPORTED)
// R' (rouletteRay): a ray can reach the roulette on the ACCUMULATED Tr.y() -- pvol_single_roulette_possible.
enum { PVOL_SINGLE_SEQ = 0, PVOL_SINGLE_PAR = 1 };
struct SinglePlanIn {
    int32_t volKind, nLights;
    int32_t rouletteRay;        // R'
    int32_t hasInit, forceSeq;  // PlanIn::hasInit, PlanIn::forceSeq
    int32_t hasTile, specOn;    // PlanIn::hasTile, PlanIn::specOn
    int32_t gather;             // the caller wants a final gather
};
struct SinglePlan { int32_t rc, form; const char *kernel; };
static_assert(sizeof(SinglePlanIn) == 32 && sizeof(SinglePlan) == 16, "tests/test_single_plan.py mirrors both");
extern "C" void pvol_single_plan(const SinglePlanIn *in, SinglePlan *out);
// R': not true exactly when diag * maxSigmaT * (1.5 maxDensity for a density region, else 1) < 6.8 -- the bound of roulette_possible
// (pvol_api.hip) over the longest segment a ray can spend inside the extent instead of one step.  No medium: never.
extern "C" int pvol_single_roulette_possible(int volKind, double diag, float maxSigmaT, float maxDensity);
// PVOL_OK, or what the render driver answers under the context's volume integrator before it launches or writes anything
extern "C" int pvol_single_render_status(const pvol_ctx *c);
// ... and pvol_radiance_batch*, which is held to the same limit (its batch has no tile, so PVOL_FORCE_SEQ does not enter)
extern "C" int pvol_single_caller_status(const pvol_ctx *c);
// The gate of the moment form, a pure function (pvol_api.hip): the number N in 1..3 of Taylor terms of exp(-delta_b L) whose truncation
// bound x^N / N! e^x, x = max_b |delta_b| pathBound, is below 2^-25, or 0 = none is (keep the 30-bin path).  sigA / sigS: 30 values;
// delta_b = sigma_t_b - the midrange of sigma_t; pathBound: a bound on the optical path length of a ray inside the medium.
extern "C" int pvol_moment_gate(const float *sigA, const float *sigS, double pathBound);
// li_group_kernel's settled class, pure: precore_bound (pvol_dev.h) for the host, and the knob's value.  The knob
// lives in the context beside PVOL_NO_MOMENTS (CtxKnobs, pvol_env.h) and not in LaunchKnobs, whose layout the plan's tests mirror.
extern "C" float pvol_precore_bound(float theta, float rho);
extern "C" float pvol_precore_kappa(const char *env);
// What the moment form reads besides the map: the gate's decision for the scene `h` (its extent's world-space diagonal bounds a ray's
// path, twice that the direct term's, which carries one order more), h.momSigBar / momEmit / momDirect, and the rows of the
// map's fill kernel (MomentWeights::w[4 n + c][b], pvol_grid.hip).  Pure; returns the terms (0: h's moment fields stay zero).
struct MomentWeights { float w[12][32]; };
extern "C" int pvol_moment_scene(DevScene &h, MomentWeights *w);
extern "C" hipError_t pvol_fill_moments(const MomentWeights *w, const float4 *alpha4, float *mom, uint32_t n, hipStream_t stream);

extern "C" {
void pvol_phase_mark(pvol_ctx *c, hipStream_t stream, int id);
// finish the volume map whose raw arrays (dRawP/dRawWi/dRawAlpha, n photons) are already on the device (pvol_map_host.hip)
int pvol_finish_map(pvol_ctx *c, uint32_t n, const float *hostPositions);
void pvol_free_photons(pvol_ctx *c);          // empties the volume map, in the context and in its host scene
void pvol_free_surface_stores(pvol_ctx *c);
void pvol_free_caustic_map(pvol_ctx *c);      // empties the caustic and the indirect map and switches the surface integrator off
int pvol_push_scene(pvol_ctx *c);
// pvol_li without the coalescer (pvol_api.hip) and through it (pvol_li_coalesce.hip); arguments already validated
int pvol_li_lone(pvol_ctx *c, const pvol_ray *ray, uint32_t *mt, int32_t *mti, float *Lv, float *T);
int pvol_li_coalesced(pvol_ctx *c, const pvol_ray *ray, uint32_t *mt, int32_t *mti, float *Lv, float *T);
int pvol_order_after_pending(pvol_ctx *c, hipStream_t stream);
// an RCCL function by name, bound at run time once per process (pvol_tile.hip); 0 when no RCCL is in reach
void *pvol_rccl_symbol(const char *name);
// plan_size(plan_path(in)) for the tests; like pvol_rccl_symbol not part of include/pvol.h
void pvol_plan_batch(const PlanIn *in, BatchPlan *out);
// every environment knob (pvol_env.h) parsed from n (name, value) pairs instead of the process environment, for the tests
void pvol_env_parse(const char *const *names, const char *const *values, uint32_t n, EnvKnobs *out);
// the gather map's kd-tree (gather_tree_build, pvol_gather_tree.h) over n host positions p[n][3], for the tests (pvol_gather.hip):
// nodes gets n GatherNode (32 bytes each), *depth the tree's depth.  No HIP call.  PVOL_E_INVALID: a NULL pointer or a non-finite
// position; PVOL_E_UNSUPPORTED: n == 0 or n > 2^24
int pvol_gather_tree_build(const float *p, uint32_t n, void *nodes, int32_t *depth);
// every status of the gather entry points in their one order (include/pvol.h), reachable without a device for the tests
// (pvol_gather.hip).  what: 0 pvol_build_gather_map, 1 pvol_build_gather_map_arrays, 2 pvol_gather_photons*, 3 pvol_gather_directions*;
// haveState: the stores are kept (0) / a map is built (2, 3); storeN: photons of the kept indirect store (0); args: the call's
// pointers as GatherCheck lists them; hostPointers: the arrays can be read
struct GatherCheck {
    const pvol_photon_array *indirect;                         // what 1
    const float *p; uint32_t count; float maxDist;             // what 2, 3
    const void *outIndex, *outD2, *outFound, *outRounds;       // what 2
    const float *frames, *wo, *uBsdf, *uPhoton; int32_t nSamples; float cosGatherAngle; const void *outBsdf, *outPhoton;   // what 3
};
int pvol_check_gather(int what, int haveCtx, int haveState, uint32_t storeN, const GatherCheck *args, int hostPointers);
// every status of pvol_final_gather* in its one order (include/pvol.h), reachable without a device for the tests
// (pvol_final_gather.hip); no HIP call.  args: the call's pointers and numbers; volKind: the scene's medium; haveGather: a gather
// map is built; haveRad / radN: a radiance result exists / its radiance photons
struct FinalGatherCheck {
    const float *p, *frames, *wo, *kd, *rayEps; uint32_t count; float maxDist; int32_t nSamples; float cosGatherAngle;
    const float *uBsdf, *uPhoton; const void *L, *draws;
};
int pvol_check_final_gather(int haveCtx, const FinalGatherCheck *args, int haveScene, int volKind, int haveGather, int haveRad, uint32_t radN);
// queries per slice of pvol_final_gather*: as many as keep a slice's scratch (64 bytes per gather ray, 2 n_samples rays per query)
// within `bound` bytes (pvol_slice_items under PVOL_FINAL_GATHER_SCRATCH_BYTES)
uint32_t pvol_final_gather_slice(int32_t nSamples, uint64_t bound);
// lowers (or, with 0, restores) the scratch bound of this context's pvol_final_gather* calls, for the tests
int pvol_final_gather_set_scratch_bound(pvol_ctx *c, uint64_t bytes);
// every status of pvol_lphoton_batch* in its one order (include/pvol.h), reachable without a device for the tests (pvol_lphoton.hip);
// no HIP call.  args: the call's pointers and numbers; g: the medium's HG parameter (0 without a scene)
struct LPhotonCheck { const float *p, *w; uint32_t n; int32_t outputKind; const void *out; };
int pvol_check_lphoton(int haveCtx, const LPhotonCheck *args, int haveScene, float g);
// points per slice of pvol_lphoton_batch*: as many as keep a slice's ordering scratch (PVOL_LPHOTON_POINT_SCRATCH bytes per point)
// within `bound` bytes (pvol_slice_items under PVOL_LPHOTON_SCRATCH_BYTES)
#define PVOL_LPHOTON_POINT_SCRATCH 16u
uint32_t pvol_lphoton_slice(uint64_t bound);
// lowers (or, with 0, restores) the scratch bound of this context's pvol_lphoton_batch* calls, for the tests
int pvol_lphoton_set_scratch_bound(pvol_ctx *c, uint64_t bytes);
// every status of pvol_radiance_batch* in its one order (include/pvol.h), reachable without a device for the tests (pvol_rays.hip); no
// HIP call.  args: the call's pointers and numbers; volKind: the scene's medium; surfOn: a surface integrator is described and on.
// (pvol_check_radiance is the radiance photons' check above; this one carries the entry point's full name.)
struct RadianceBatchCheck { const void *rays, *streams; uint32_t nRays, nStreams; int32_t outputKind; const pvol_radiance_out *out; };
int pvol_radiance_batch_check(int haveCtx, const RadianceBatchCheck *args, int haveScene, int volKind, int surfOn);
// caller rays per slice of pvol_radiance_batch*: as many as keep a slice's scratch within `bound` bytes (pvol_slice_items under
// PVOL_RADIANCE_SCRATCH_BYTES) when every ray spawns maxSegments rays -- PVOL_RADIANCE_RAY_SCRATCH bytes per expanded ray and
// PVOL_RADIANCE_CALLER_SCRATCH per caller ray (pvol_rays_plan.h).  maxSegments: pvol_radiance_max_segments for the worst case; the
// entry point asks with 0 (nobody spawns), counts, and cuts the slice back to the longest run of its rays whose blocks fit
uint32_t pvol_radiance_slice(uint32_t maxSegments, uint64_t bound);
// rays_slice_cut and rays_slice_streams (pvol_rays_plan.h) for the tests.  The second: the table of the slice [r0, r1) of a call of
// nRays rays over `streams`, from stream *s on: table (room for nStreams entries) gets the slice's entries, out3 = {s0, entries,
// continued}, *s the next slice's first stream, *maxRays what streams_partition reports.  PVOL_E_INVALID: a NULL pointer, streams
// that do not partition [0, nRays), *s > nStreams, or not r0 < r1 <= nRays
uint32_t pvol_radiance_slice_cut(const uint32_t *offset, uint32_t n, uint64_t budget);
int pvol_radiance_slice_streams(const pvol_stream *streams, uint32_t nStreams, uint32_t nRays, uint32_t r0, uint32_t r1, uint32_t *s,
                                pvol_stream *table, uint32_t *out3, uint32_t *maxRays);
// rays the specular recursion can spawn for one ray: 2 + 4 + ... + 2^(maxSpecularDepth - 1), 0 unless specOn (glass in the scene, the
// surface integrator on, maxspeculardepth > 1)
uint32_t pvol_radiance_max_segments(int specOn, int32_t maxSpecularDepth);
// lowers (or, with 0, restores) the scratch bound of this context's pvol_radiance_batch* calls, for the tests
int pvol_radiance_set_scratch_bound(pvol_ctx *c, uint64_t bytes);
// every status of pvol_radiance_gather_batch* in its one order (include/pvol.h), reachable without a device for the tests
// (pvol_rays.hip); no HIP call.  args: the call's pointers and numbers; volKind: the scene's medium; surfOn: a surface integrator is
// described and on; indirectN: photons of the indirect map it describes; haveGather: a gather map is built; haveRad / radN: a radiance
// result exists / its radiance photons
struct RadianceGatherCheck {
    const void *rays, *streams; uint32_t nRays, nStreams; int32_t outputKind; const pvol_radiance_gather_out *out; const pvol_gather_params *gather;
};
int pvol_radiance_gather_check(int haveCtx, const RadianceGatherCheck *args, int haveScene, int volKind, int surfOn, uint32_t indirectN, int haveGather,
                               int haveRad, uint32_t radN);
// caller rays per slice of pvol_radiance_gather_batch* when nobody spawns: pvol_radiance_slice(0, bound) with the gather's
// PVOL_RADIANCE_GATHER_SCRATCH(nSamples) bytes per expanded ray on top; the entry point counts and cuts as pvol_radiance_batch* does
uint32_t pvol_radiance_gather_slice(int32_t nSamples, uint64_t bound);
// the kernels of pvol_radiance_gather_batch* (pvol_rays_gather.hip), over the `total` expanded rays of a slice of n caller rays
struct RaysGatherArgs {
    const DevScene *scene;
    pvol_ray *rays;                  // [total] expanded (rays_emit_kernel's); patch adds the gather's draws to rng_skip
    const SegInfo *info;             // [total] sample = the owner, the caller ray's index in the slice
    const uint32_t *offset;          // [n + 1] where every block starts
    uint32_t total, n;
    int32_t nSamples;
    const float *uBsdf, *uPhoton;    // [n][nSamples][3] the slice's rows of the caller's arrays
    float *p, *frames, *wo, *kd, *rayEps;   // [total] x 3, 9, 3, 30, 1: the queries
    float *mUBsdf, *mUPhoton;        // [total][nSamples][3] every member's copy of its owner's rows
    float *Lg;                       // [total][30]
    uint32_t *gDraws;                // [total]
    float *rows;                     // [total][60] add: Lv += T (.) Lg
    uint32_t *gatherDraws;           // [n] the caller's output (optional)
};
extern "C" hipError_t pvol_launch_rays_gather_query(const RaysGatherArgs *a, hipStream_t stream);   // the queries and the sample rows
extern "C" hipError_t pvol_launch_rays_gather_patch(const RaysGatherArgs *a, hipStream_t stream);   // rng_skip += draws; gatherDraws
extern "C" hipError_t pvol_launch_rays_gather_add(const RaysGatherArgs *a, hipStream_t stream);     // behind surface_kernel
// the points [first, first + n) of d_p ordered by their cell of G (pvol_grid.hip)
hipError_t pvol_order_points(const PhotonGrid *G, const float *d_p, uint32_t first, uint32_t n, uint32_t *work, void *temp, size_t *tempBytes,
                             hipStream_t stream);
// the shoot's merge (ShootMerge, pvol_shoot_merge.h) replayed over recorded count tables, for the tests (pvol_shoot_host.hip)
size_t pvol_shoot_merge_replay(const uint32_t *cfg, const uint32_t *tables, uint32_t nTables, uint64_t *out, size_t cap);
// the plan of a render call (RenderPlan below) flattened for the tests (pvol_render_host.hip)
size_t pvol_render_plan_flat(const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                             const uint32_t *taskIds, uint32_t nTaskIds, const int32_t *flags, int64_t tileBatchRays, uint64_t *out, size_t cap);
// the status pvol_set_scene gives the scene on a working device, reachable without one for the tests (pvol_scene_host.hip)
int pvol_check_scene(const pvol_params *params, const pvol_scene *s);
// pvol_set_triangle_normals' argument checks against the scene `s`, reachable without a device for the tests (pvol_scene_host.hip)
int pvol_check_triangle_normals(const pvol_scene *s, const float *n, uint32_t nTriangles);
// pvol_set_scene's check of an exponential medium's arguments (PVOL_OK or PVOL_E_INVALID), reachable without a device for the tests;
// up3 (optional) gets the normalised updir
int pvol_check_exponential(const pvol_volume *v, float *up3);
// the argument checks of pvol_compute_radiance (what 0), pvol_compute_radiance_arrays (1) and pvol_radiance_lookup* (2), reachable
// without a device for the tests (pvol_radiance.hip).  haveState: the stores are kept (0) / a compute has succeeded (2); a, b: the
// radiance photons' p and n (1) or the queries' (2); hostPointers: a, b and the maps can be read (their values must be finite)
int pvol_check_radiance(int what, int haveCtx, int haveState, int32_t nLookup, float maxDist, const pvol_photon_array *const *maps, const float *a,
                        const float *b, const float *rhoR, const float *rhoT, uint32_t count, const void *outLo, const void *outFound, int hostPointers);
// every status of pvol_set_surface_integrator_maps in its one order, reachable without a device for the tests (pvol_map_host.hip).
// materials: 0 the scene's surfaces are matte, 1 glass among them, 2 a kind the surface integrator does not cover; storesKept and
// storeN / storePaths ([0] caustic, [1] indirect): what the last pvol_preprocess* kept; hostPointers: the arrays can be read
int pvol_check_surface_maps(const pvol_surface_params *sp, int haveScene, int materials, int storesKept, const uint32_t *storeN,
                            const uint32_t *storePaths, const pvol_photon_array *caustic, const pvol_photon_array *indirect, int hostPointers);
// the ray probe of the tests (pvol_probe.hip): n host rays through the device's own hit routines on the uploaded scene -- mode 0
// surf_closest, 1 lane_occluded, 2 scene_occluded (one ray per wave), 3 scene_closest (one ray per wave); per ray out gets t, rayEps, p, nn, dpdu (11 floats) and outi the
// hit flag, the primitive (triangle index in upload order, -1 - i for sphere i) and its material.  Synchronous; PVOL_E_INVALID for a
// null pointer, no scene, n == 0 or an unknown mode
int pvol_probe_hits(pvol_ctx *c, const pvol_ray *rays, uint32_t n, int mode, float *out, int32_t *outi);
// the largest density of a checked exponential medium over its extent (feeds roulette_possible like a VolumeGrid's maximum); up3: the normalised updir
float pvol_exponential_max_density(const pvol_volume *v, const float *up3);
}

// ---- the scene's device image (pvol_scene_host.hip): everything pvol_set_scene derives from its arguments, a pure
// function of them -- no HIP call, no context.  `scene` is complete but for what only a device can give: the density grid, the
// hierarchy, shootScene and the photon-map fields (all zero here).
struct PVOL_LOCAL SceneImage {
    DevScene scene;
    DevShootScene shoot;
    float maxDensity;               // largest density factor of the medium (1 for analytic volumes, max of the grid values)
    float bvhPad;                   // a scene that takes the hierarchy: what its boxes are padded by
    std::vector<int32_t> primMat;   // material of every triangle, then of every sphere
};
PVOL_LOCAL int pvol_scene_image(const pvol_params *params, const pvol_scene *s, SceneImage *out);

// writes a map (an empty one included) into the photon-map fields of the host scene (pvol_map_host.hip)
PVOL_LOCAL void pvol_map_to_scene(const PhotonGrid &G, DevScene &h);
// the volume map's moment rows under the scene h, with h's moment constants and the gate's decision (pvol_map_host.hip)
PVOL_LOCAL int pvol_map_moments(const PhotonGrid &G, DevScene &h, DevPtr<float> &mom, int *terms);

// ImageFilm's crop window behind the *_window entry points: a NULL window is the whole frame (crop 0 1 0 1), which is what the
// entry points without a window pass
static inline bool pvol_window_ok(const pvol_film *f, const pvol_film_window *w) {
    return !w || (w->x_pixel_start >= 0 && w->y_pixel_start >= 0 && w->x_pixel_count > 0 && w->y_pixel_count > 0 &&
                  w->x_pixel_count <= f->x_resolution - w->x_pixel_start && w->y_pixel_count <= f->y_resolution - w->y_pixel_start);
}
static inline pvol_film_window pvol_window_or_full(const pvol_film *f, const pvol_film_window *w) {
    if (w) return *w;
    pvol_film_window full = {0, 0, f->x_resolution, f->y_resolution};
    return full;
}
static inline bool film_ok(const pvol_film *f) {
    return f && f->x_resolution > 0 && f->y_resolution > 0 && f->filter_xwidth > 0.f && f->filter_ywidth > 0.f &&
           f->filter_xwidth <= 3.f && f->filter_ywidth <= 3.f;
}
// the splat of n samples into the film (pvol_tile.hip); window == NULL: the whole frame, through the full-frame kernel
PVOL_LOCAL int film_add(pvol_ctx *c, const pvol_film *film, const pvol_film_window *window, const float *dXY, const float *dXYZ, uint32_t stride,
                        uint64_t n, int guard, float *dPixels, hipStream_t stream);

// ---- the plan of a render call (pvol_render_host.hip): every check of pvol_render_tasks_window_device, every task's
// sub-window and sample count, and the cut of the task list into batches with all a batch reserves and uploads -- a pure function of its
// arguments: no HIP call, no context, no environment.
// One task's sub-window (Sampler::ComputeSubWindow) and its camera samples; pvol_render_sample_count sums the same
static inline uint64_t pvol_task_samples(const pvol_sampler *s, uint32_t task, int32_t win[4]) {
    pvol_compute_sub_window(s, task, win);
    return (uint64_t)(win[1] - win[0]) * (uint64_t)(win[3] - win[2]) * s->pixel_samples;
}
struct RenderBatch {
    uint32_t b0, b1;       // the batch is tasks [b0, b1) of the list; its stream table and windows are the plan's entries [b0, b1)
    uint32_t maxRays;      // samples of its largest task
    int32_t surfOn, specOn;
    uint64_t nRays;        // camera samples of the batch
    uint64_t doneRays;     // ... and of the batches in front of it: where its debug records go
    uint64_t want[7];      // bytes reserved: PVOL_BUF_TILE_RAYS .. PVOL_BUF_TILE_WINDOWS, PVOL_BUF_TAU, PVOL_BUF_SPEC_LINK
};
struct PVOL_LOCAL RenderPlan {
    int rc;
    TileArgs tile;                       // what depends on camera and sampler only; the batch adds its buffers
    uint64_t batchRays;                  // the work-buffer budget of a batch, in camera samples
    std::vector<int32_t> win;            // per task of the list: x0, x1, y0, y1
    std::vector<uint64_t> count;         // per task: camera samples
    std::vector<pvol_stream> streams;    // per task: seed = task number, first_ray = samples in front of it within its batch
    std::vector<RenderBatch> batches;
};
// surfOn: the surface integrator is on; specOn: ... and the scene holds a specular material; tileBatchRays: LaunchKnobs::tileBatchRays
PVOL_LOCAL RenderPlan pvol_render_plan(const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                                       const uint32_t *taskIds, uint32_t nTaskIds, bool havePixels, bool haveScene, bool surfOn, bool specOn,
                                       int64_t tileBatchRays);
// One rank's share of a frame: its tasks (pvol_partition_tasks) into its own film, zeroed first.  The caller has the context's device set.
PVOL_LOCAL int render_share(pvol_ctx *c, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window, const pvol_sampler *smp,
                            uint32_t rank, uint32_t nRanks, float *dPixels, hipStream_t stream);
#endif
