// pvol_points_dev.h -- lphoton_points_kernel: PhotonVolumeIntegrator::LPhoton (photonvolume.cpp:65-108) at points the caller names
// (pvol_lphoton_batch*).  Included by pvol_march.hip, where lphoton() lives; the unit's second compilation
// (pvol_region_exp.h) gives the exponential medium.
//
// One wave per lookup, in runs of 64 consecutive lookups of the SORTED order (the host sorts the points by the volume map's grid
// cell, pvol_order_points), eight consecutive runs per wave at a time as li_fixup_kernel walks its list: neighbours in the order
// are neighbours in space, so the k-th distance^2 just found is the first radius of the next lookup and the photon rows of one
// run are still in the L2 for the next.
//
// Every point is looked up TWICE.  The order in which lphoton() lists its candidates depends on the radius it searched (which rows
// of cells share a batch of 64, which of them are long enough to be read on their own, whether the sub-cell level was walked), and
// that order decides which photon of a tie at the k-th distance is kept and in which order the flux is summed.  A radius carried
// from the neighbour would therefore let a point's bytes depend on which points share the call.  So the carried radius only
// serves a first pass that stops after the selection (REPORT 2): nFound and the k-th distance^2 are exact whatever the radius was.
// The second pass searches a radius that is a function of the point alone -- PVOL_GUESS_SCALE x its own k-th distance^2, which
// holds the k nearest by construction, or the whole maxdist ball where fewer than nused lie inside -- and its list, its ties and
// its sum are the point's own.  A point with fewer than 10 photons skips it (photonvolume.cpp:83-84).
#ifndef PVOL_POINTS_DEV_H
#define PVOL_POINTS_DEV_H

// the two passes as functions of their own, so that the kernel holds each body once
template <int NREG>
__device__ __noinline__ void lphoton_select(const DevScene &S, Gather &G, V3 pt, int lane, WaveCounters &wc, float guess, float *rk, int *nFound, float *maxmd) {
    lphoton<false, NREG, true, 2>(S, G, v3(0.f, 0.f, 1.f), pt, mk4(0.f), lane, wc, guess, rk, nFound, maxmd);
}
template <int NREG>
__device__ __noinline__ f4 lphoton_own(const DevScene &S, Gather &G, V3 w, V3 pt, f4 sigS_at_p, int lane, WaveCounters &wc, float guess) {
    float rk, maxmd;
    int nFound;
    return lphoton<false, NREG, true, 1>(S, G, w, pt, sigS_at_p, lane, wc, guess, &rk, &nFound, &maxmd);
}

template <bool SPECTRAL, int NREG>
__global__ __launch_bounds__(LANES, (NREG > 4 ? PVOL_WPE_BIG : PVOL_WPE)) void lphoton_points_kernel(PointsArgs A) {
    extern __shared__ __align__(16) unsigned char lds[];
    const DevScene &S = *A.scene;
    const int lane = threadIdx.x;
    Gather G;
    G.cap = S.candCap;
    G.cd = reinterpret_cast<float *>(lds);
    G.ci = reinterpret_cast<uint32_t *>(lds + (size_t)G.cap * 4);
    G.paint = reinterpret_cast<uint32_t *>(lds + (size_t)G.cap * 8);
    const int q = lane & 7;
    const f4 sigS4 = ld4(S.sigS, q);
    const f4 X4 = ld4(S.cieX, q), Y4 = ld4(S.cieY, q), Z4 = ld4(S.cieZ, q);
    WaveCounters wc = {};
    const uint32_t nRuns = (A.n + 63u) / 64u;
    for (uint32_t runI = blockIdx.x * 8u; runI < nRuns; runI = ((runI & 7u) == 7u) ? runI + 1u + (gridDim.x - 1u) * 8u : runI + 1u) {
        const uint32_t e0 = runI * 64u;
        const bool have = e0 + (uint32_t)lane < A.n;
        // every lane fetches one point of the run and evaluates the medium there; the lookups then take them lane by lane
        uint32_t slot = 0u;
        V3 p = v3(0.f, 0.f, 0.f), w = v3(0.f, 0.f, 1.f);
        float dens = 0.f;
        if (have) {
            slot = A.order ? A.order[e0 + lane] : A.first + e0 + (uint32_t)lane;
            p = v3(A.p[3 * (size_t)slot], A.p[3 * (size_t)slot + 1], A.p[3 * (size_t)slot + 2]);
            if (A.w) w = v3(A.w[3 * (size_t)slot], A.w[3 * (size_t)slot + 1], A.w[3 * (size_t)slot + 2]);
            if (S.volKind != PVOL_VOLUME_NONE) dens = vol_density(S, p);   // sigma_s(p) = sigma_s x this: Inside() ? 1 : 0, or Density()
        }
        unsigned long long todo = __ballot(have);
        float carry = 0.f;   // a run starts from the map's mean density
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t sj = (uint32_t)lane_i((int)slot, j);
            const V3 pj = v3(lane_f(p.x, j), lane_f(p.y, j), lane_f(p.z, j)), wj = v3(lane_f(w.x, j), lane_f(w.y, j), lane_f(w.z, j));
            const float dj = lane_f(dens, j);
            float rk, maxmd;
            int nFound;
            lphoton_select<NREG>(S, G, pj, lane, wc, carry > 0.f ? carry : S.rkEstimate, &rk, &nFound, &maxmd);
            carry = rk > 0.f ? rk : S.maxDistSq;   // fewer than nused within maxdist: sparse here, the full ball is the cheap radius
            f4 L = mk4(0.f);
            if (nFound >= 10) L = lphoton_own<NREG>(S, G, wj, pj, sigS4 * dj, lane, wc, nFound == S.nUsed ? maxmd : 0.f);
            if (lane == 0) {
                if (A.nFound) A.nFound[sj] = (uint32_t)nFound;
                if (A.radius2) A.radius2[sj] = maxmd;
            }
            if (SPECTRAL) {
                if (lane < 8) {
                    float *op = A.out + (size_t)sj * 30 + 4 * q;
                    op[0] = L.x; op[1] = L.y;
                    if (q < 7) { op[2] = L.z; op[3] = L.w; }
                }
            } else {   // li_fixup_kernel's projection
                const float scale = float(700 - 400) / float(106.856895f * 30);
                const float x = group8_sum(X4.x * L.x + X4.y * L.y + X4.z * L.z + X4.w * L.w) * scale;
                const float y = group8_sum(Y4.x * L.x + Y4.y * L.y + Y4.z * L.z + Y4.w * L.w) * scale;
                const float z = group8_sum(Z4.x * L.x + Z4.y * L.y + Z4.z * L.z + Z4.w * L.w) * scale;
                if (lane == 0) *reinterpret_cast<float4 *>(A.out + (size_t)sj * 4) = make_float4(x, y, z, 0.f);
            }
        }
    }
}

// candCap: DevScene::candCap of the scene the points are looked up in; NREG by it exactly as pvol_launch_li_group chooses
extern "C" hipError_t pvol_launch_lphoton_points(const PointsArgs *args, int candCap, uint32_t nWaves, hipStream_t stream) {
    const size_t ldsBytes = (size_t)candCap * 8 + PAINT_CAP * 4;
    const bool big = candCap > 4 * LANES;
    const dim3 grid(nWaves), block(LANES);
    if (args->spectral) {
        if (big) hipLaunchKernelGGL((lphoton_points_kernel<true, 12>), grid, block, ldsBytes, stream, *args);
        else hipLaunchKernelGGL((lphoton_points_kernel<true, 4>), grid, block, ldsBytes, stream, *args);
    } else {
        if (big) hipLaunchKernelGGL((lphoton_points_kernel<false, 12>), grid, block, ldsBytes, stream, *args);
        else hipLaunchKernelGGL((lphoton_points_kernel<false, 4>), grid, block, ldsBytes, stream, *args);
    }
    return hipGetLastError();
}
#endif
