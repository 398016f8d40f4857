// pvol_liargs.h -- the argument block of the Li() kernels, ONE definition for the kernels (pvol_march.hip) and the host code that
// fills it (pvol_api.hip, pvol_render_host.hip through pvol_host.h)
#ifndef PVOL_LIARGS_H
#define PVOL_LIARGS_H
#include "pvol_dev.h"
// The fixed tail of the marching kernels' LDS, prevRk | paint (march_lds, pvol_march.hip), sized here for the kernels and for plan_size
#define PREV_N 256     // march steps for which the previous ray's k-th distance^2 is remembered
#define PAINT_ROW 16   // rows up to this many photons go through the painted index list
#define PAINT_CAP (64 * PAINT_ROW)
constexpr size_t PVOL_MARCH_LDS_FIXED = PREV_N * 4 + PAINT_CAP * 4;
static_assert(PVOL_MARCH_LDS_FIXED == 256 * 4 + 1024 * 4, "the LDS byte counts of the plan are pinned (tests/test_launch_plan.py)");

// One launch of a kernel template by the batch: NREG = candidate registers per lane in select_k (4 covers nused <= 64, 12 covers
// nused <= 576), STATS = the work counters.  `kernel` is written with the names NREG (and STATS) in its template arguments and is
// instantiated for exactly the values the ladder can choose.
#define PVOL_LAUNCH_NREG(candCap, kernel, grid, block, ldsBytes, stream, ...)                                                      \
    do {                                                                                                                           \
        if ((candCap) <= 4 * 64) { constexpr int NREG = 4; hipLaunchKernelGGL(kernel, grid, block, ldsBytes, stream, __VA_ARGS__); } \
        else { constexpr int NREG = 12; hipLaunchKernelGGL(kernel, grid, block, ldsBytes, stream, __VA_ARGS__); }                   \
    } while (0)
#define PVOL_LAUNCH_STATS_NREG(stats, candCap, kernel, grid, block, ldsBytes, stream, ...)                                         \
    do {                                                                                                                           \
        if (stats) { constexpr bool STATS = true; PVOL_LAUNCH_NREG(candCap, kernel, grid, block, ldsBytes, stream, __VA_ARGS__); } \
        else { constexpr bool STATS = false; PVOL_LAUNCH_NREG(candCap, kernel, grid, block, ldsBytes, stream, __VA_ARGS__); }      \
    } while (0)
struct LiArgs {
    const DevScene *scene;
    const pvol_ray *rays;
    pvol_stream *streams;
    uint32_t nStreams;
    uint32_t nRays;
    int outputKind;
    float *out;
    uint32_t *draws;
    const uint32_t *initState;  // optional: nStreams x 625 words (mt[624], mti) instead of seeding
    uint32_t *finalState;       // optional: same layout, written back
    DevCounters *counters;
    int transmittanceOnly;
    uint32_t *chunkCounter;     // li_par_kernel: next chunk of CHUNK_RAYS rays
    uint32_t *needSeq;          // li_par_kernel sets it when a ray reaches the roulette; li_seq_kernel runs only if set (gate)
    int gated;                  // li_seq_kernel: 1 = return at once unless *needSeq
    // resolve + replay (scenes where drawn values matter): rays are processed in slices, slice k of a stream =
    // its rays [k*sliceM, (k+1)*sliceM); the MT state of every stream persists in `state` between slices
    unsigned char *records;     // [nStreams * sliceM] slots of recStride bytes
    uint32_t recStride, sliceM, sliceK;
    uint32_t *state;            // [nStreams][625]
    float grpGuess;             // li_group_kernel: search radius^2 = this x the guessed k-th distance^2
    int liteResolve;            // no march step can reach the roulette: geometry pre-pass + RNG-only resolve
    DeferRec *defer;            // li_group_kernel: lookups handed to li_fixup_kernel
    uint32_t *deferCount;
    uint32_t deferCap;
    TauRec *tauOut;             // optional: per ray Li()'s *T (render driver with the surface integrator on)
    int32_t fixGroup;           // nused beyond the bucket plan: the hand-over list is padded to 64-slot runs for li_fixup_group_kernel
    float fxgWiden, fxgAim;     // li_fixup_group_kernel's radius policy (0 = the defaults 1.3 / 1.4): first radius^2 = widen x the probe's, the probe aims at aim x nused photons
    int32_t *status;            // optional: per ray PVOL_E_LIMIT where the record / LDS plan refused it (coalesced per-sample batches)
    int32_t moments;            // li_group_kernel, ray-parallel XYZ form: sum the map's moment rows (BatchPlan::groupForm 3)
    float grpPrecore;           // li_group_kernel: kappa of the settled class (theta = kappa x the smallest guessed k-th distance^2 served), 0 = off
};
// One slice of pvol_lphoton_batch* (lphoton_points_kernel, pvol_points_dev.h): LPhoton at the caller's points.  p, w, out, nFound and
// radius2 are the CALL's arrays, indexed by the point's input slot; order lists the slice's slots in the order the waves serve them.
struct PointsArgs {
    const DevScene *scene;
    const float *p, *w;         // [call's n][3]; w == 0: no direction (g == 0 reads none)
    const uint32_t *order;      // [n] input slots, sorted by grid cell (pvol_order_points); 0: first, first + 1, ...
    uint32_t first, n;          // the slice: n lookups, and where the unsorted order starts
    int32_t spectral;
    float *out;                 // 30 floats per point, or X, Y, Z, 0
    uint32_t *nFound;           // optional
    float *radius2;             // optional
};
// One slice of pvol_radiance_batch* (pvol_rays_dev.h): n caller rays and the expanded array their blocks are laid out in.
struct RaysArgs {
    const DevScene *scene;
    const pvol_ray *in;         // [n] the slice's caller rays
    uint32_t n;
    int32_t surfOn, specOn;     // the surface integrator is on; ... and a glass hit can spawn rays (pvol_ctx::specOn)
    int32_t spectral;           // L: 60 floats per ray, else X, Y, Z, T.y
    uint32_t *count;            // [n + 1] members per block, entry n zero
    const uint32_t *offset;     // [n + 1] its exclusive scan: where every block starts, entry n the expanded rays of the slice
    pvol_ray *rays;             // expanded: per block the segments in post-order, the primary last
    SegInfo *info;              // expanded; the primary's: Fs = maxt after the clip, pad[0] = 1 when Scene::Intersect hit inside [mint, maxt]
    float *rows;                // expanded: Lv[30], T[30] of the volume batch, then of surface_kernel's spectral mode
    const uint32_t *draws;      // expanded: RandomUInt calls of every member's own volume Li()
    float *stash;               // [n][60] the primaries' rows while theirs hold Ls_matte
    float *L, *surfXyz, *tHit;  // the slice's part of pvol_radiance_out; all but L optional
    uint32_t *outDraws, *surfDraws, *nSegments;
};
#endif
