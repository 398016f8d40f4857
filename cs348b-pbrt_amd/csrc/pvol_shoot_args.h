// pvol_shoot_args.h -- the argument blocks of the photon shooter's kernels, ONE definition for the kernels (pvol_shoot.hip) and the
// host driver that fills them (pvol_shoot_host.hip)
#ifndef PVOL_SHOOT_ARGS_H
#define PVOL_SHOOT_ARGS_H
#include <hip/hip_runtime.h>
#include "pvol_dev.h"

struct ShootArgs {
    const DevScene *scene;
    const DevShootScene *shoot;
    uint32_t nTasks;
    const uint32_t *stateIn;  // [nTasks][pvol_shoot_state_words()]
    uint32_t *stateOut;       // same layout; a round that has to be redone (block buffer too small) restarts from stateIn
    uint32_t *halton;         // [nTasks][48] permutation tables (bases 2,3,5,7,11,13: 41 entries)
    const uint32_t *flags;    // [nTasks] bit0 causticDone, bit1 indirectDone, bit2 volumeDone, bit3 finished
    float *localPhotons;      // [nTasks][cap][36]: p(3) wi(3) alpha(30)
    uint32_t *localCounts;    // [nTasks][8]: volume, caustic, direct, indirect deposits of this block, surface records kept, radiance photons kept
    uint32_t cap;
    // the surface stores of photonshooter.cpp:148-189, kept only on request (pvol_params.keep_surface_photons): every deposit
    // is one record Photon(p, alpha, wo) with its kind (0 caustic, 1 direct, 2 indirect), in deposit order
    float *localSurf;         // [nTasks][capS][36]: p(3) wo(3) alpha(30)
    uint32_t *localSurfKind;  // [nTasks][capS]
    uint32_t capS;
    float *localRad;          // [nTasks][capR][8]: p(3) n(3) material index, pad  (RadiancePhoton + whose rho it carries)
    uint32_t capR;
    int keepSurface;
    unsigned long long *stats;  // paths, follow_calls, no_hit, march_steps, interactions, absorbed, split_children, overflow
    int init;                 // 1: seed RNG + Halton tables instead of shooting
    uint32_t blockPaths;      // paths per task and round (4096: PhotonShootingTask::Run's block, photonshooter.cpp:247)
    int gridVolume;           // the medium is a VolumeGrid: the kernel takes GRID_KMAX x 64 more LDS words (march_grid)
    const uint32_t *taskIds;  // [nTasks] global task number of each slot (one rank's share, pvol_preprocess_ranks), or null:
                              // slot == task.  Every array above is indexed by slot; the RNG seed and Halton permutation by task
};

// merge of one task's block into the global photon arrays: alpha /= float(nshot) with the RUNNING nshot
// of that task's turn (photonshooter.cpp:333)
struct MergeArgs {
    const float *localPhotons;
    uint32_t cap;
    const uint32_t *srcTask;   // per merged segment: task, count, destination offset, nshot
    const uint32_t *count;
    const uint32_t *dstOff;
    const float *nshot;
    uint32_t nSeg;
    float *p, *wi, *alpha;     // destination raw arrays
};

// merge of one task's surface records into the per-kind arrays, in deposit order (photonshooter.cpp:303-327), and of its
// radiance photons (:341-349).  `take` has bit k set when kind k is merged at this task's turn.
struct SurfMergeArgs {
    const float *localSurf; const uint32_t *localSurfKind; uint32_t capS;
    const float *localRad; uint32_t capR;
    const uint32_t *srcTask, *nSurf, *take, *dstOff;   // dstOff: [nSeg][4] = caustic, direct, indirect, radiance
    const uint32_t *nRad;
    uint32_t nSeg;
    float *p[3], *wo[3], *alpha[3];
    float *rad;   // [n][8]
};

// Placement of the rows of a sharded shoot (pvol_preprocess_ranks).  After the last round every rank holds the all-gathered local
// arrays of all ranks: rank r's block is `rankStride` floats, field f of it (p, wi|wo, alpha; or the radiance record) `fieldOff`
// floats in, `width` floats per row, rows in that rank's append order.  A segment (src rank, local row, global row, count) is one
// task's contribution at its turn in the merge; the segments are in global order and cover [0, nRows) without gaps.
struct PlaceArgs {
    const float *recv;
    uint64_t rankStride;
    uint64_t fieldOff;
    uint32_t width;
    const uint32_t *segSrc, *segLocal, *segGlobal;
    uint32_t nSeg;
    uint64_t nRows;
    float *dst;   // [nRows][width]
};

extern "C" {
hipError_t pvol_launch_shoot(const ShootArgs *a, hipStream_t stream);
#if !PVOL_REGION_EXP   /* undefined or 0: the first compilation and the host units */
hipError_t pvol_launch_shoot_exp(const ShootArgs *a, hipStream_t stream);   // pvol_shoot_exp.hip: through an exponential medium
#endif
size_t pvol_shoot_state_words(void);
hipError_t pvol_launch_merge(const MergeArgs *m, hipStream_t stream);
hipError_t pvol_launch_merge_surface(const SurfMergeArgs *m, hipStream_t stream);
hipError_t pvol_launch_place_rows(const PlaceArgs *a, hipStream_t stream);
}
#endif
