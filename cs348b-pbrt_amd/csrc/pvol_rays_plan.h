// pvol_rays_plan.h -- the decisions of pvol_radiance_batch*'s slice walk (pvol_rays.hip) as pure functions: where a
// candidate slice is cut back, and which of the caller's streams a slice holds.  Plain C++, no HIP: pvol_rays.hip drives the device
// with what they return, tests/test_rays_plan.py reaches them (pvol_radiance_slice_cut, pvol_radiance_slice_streams) without a GPU.
#ifndef PVOL_RAYS_PLAN_H
#define PVOL_RAYS_PLAN_H
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/pvol.h"

// scratch of a slice: bytes per expanded ray (48 of ray, 32 of SegInfo, 240 of output, 4 of draw count) and per caller ray (its
// stashed row, block size and offset)
#define PVOL_RADIANCE_RAY_SCRATCH 324u
#define PVOL_RADIANCE_CALLER_SCRATCH 248u
// pvol_radiance_gather_batch* adds, per expanded ray, its final-gather query (p 12, frame 36, wo 12, kd 120, ray_eps 4), the result
// (Lg 120, draws 4) and its copy of the owner's sample rows (2 x 12 per sample)
#define PVOL_RADIANCE_GATHER_SCRATCH(nSamples) (308u + 24u * (uint32_t)(nSamples))

// perExpanded: bytes per expanded ray -- PVOL_RADIANCE_RAY_SCRATCH, plus the gather's where the call gathers
static inline bool rays_slice_fits(uint64_t expanded, uint64_t callers, uint64_t budget, uint64_t perExpanded = PVOL_RADIANCE_RAY_SCRATCH) {
    return expanded * perExpanded + callers * PVOL_RADIANCE_CALLER_SCRATCH <= budget;
}

// How many of a candidate slice's n caller rays go: all of them when their blocks fit the budget, else the longest run that does --
// whole runs of 64 where that many fit, never fewer than one ray.  offset: the exclusive scan over the n + 1 block sizes, so the
// offsets of a run do not depend on what follows it and the scan stands for the run that is kept.
static inline uint32_t rays_slice_cut(const uint32_t *offset, uint32_t n, uint64_t budget, uint64_t perExpanded = PVOL_RADIANCE_RAY_SCRATCH) {
    if (n <= 1 || rays_slice_fits(offset[n], n, budget, perExpanded)) return n;
    uint32_t lo = 1, hi = n;   // fits(lo) is taken for granted (one ray always goes), fits(hi) is false
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rays_slice_fits(offset[mid], mid, budget, perExpanded)) lo = mid; else hi = mid;
    }
    return lo >= 64 ? lo - lo % 64 : lo;
}

// The stream table of the slice [r0, r1) of a call of nRays rays: the caller's streams hs[s0 .. s0 + n) with rays in it, and the empty
// ones that stand there (at the very end: in the last slice), appended to `table` with first_ray and n_rays rebased to the slice and
// end_draw 0.  s: the first stream that may reach into the slice; left at the first one of the next slice, which is the stream the
// boundary cuts where it cuts one.  continued: the slice's first stream began in an earlier slice.
struct RaysSliceStreams { uint32_t s0, n; bool continued; };
static inline RaysSliceStreams rays_slice_streams(const pvol_stream *hs, uint32_t nStreams, uint32_t r0, uint32_t r1, uint32_t nRays, uint32_t &s,
                                                  std::vector<pvol_stream> &table) {
    const bool last = r1 == nRays;
    RaysSliceStreams out = {s, 0u, false};
    for (; s < nStreams; ++s) {
        const pvol_stream &h = hs[s];
        const uint32_t end = h.first_ray + h.n_rays;
        if (h.first_ray >= r1 && !(last && !h.n_rays)) break;
        pvol_stream t = h;
        t.first_ray = std::max(h.first_ray, r0) - r0; t.n_rays = std::min(end, r1) - std::max(h.first_ray, r0); t.end_draw = 0;
        table.push_back(t);
        ++out.n;
        if (end > r1) break;   // the boundary cuts this stream: the next slice begins with the rest of it
    }
    out.continued = out.n && hs[out.s0].first_ray < r0;
    return out;
}

// the streams partition the ray array in order (every ray belongs to exactly one stream); maxRays (optional): the longest stream, at least 1
static inline bool streams_partition(const pvol_stream *st, uint32_t nStreams, uint32_t nRays, uint32_t *maxRays) {
    uint64_t next = 0;
    uint32_t most = 1;
    for (uint32_t s = 0; s < nStreams; ++s) {
        if (st[s].first_ray != next) return false;
        next += st[s].n_rays;
        most = std::max(most, st[s].n_rays);
    }
    if (maxRays) *maxRays = most;
    return next == nRays;
}
#endif
