// pvol_radiance.hip -- the tail of PhotonShooter::Preprocess with `finalgather` (core/photonshooter.cpp:505-524) on the device:
// ComputeRadianceTask::Run (:359-395) gives every radiance photon its outgoing radiance Lo from three k-NN irradiance estimates
// (EPhoton, :17-35) over the direct, indirect and caustic maps, and the photons become the radiance map, which answers
// radianceMap->Lookup(p, RadiancePhotonProcess(n), INFINITY) (photonshooter.h:63-78): the nearest photon whose normal faces n.
// Kernels and their host code in one unit; the maps are PhotonGrids built by build_photon_grid (pvol_map_host.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include "pvol_math.h"
#include "pvol_gridrows_dev.h"
#include "pvol_radwalk_dev.h"
#include "pvol_host.h"

#define RAD_MAX_LOOKUP 576   // the project's nused bound

// One surface map as radiance_lo_kernel reads it
struct RadMap {
    GridView g;
    const float4 *wi4, *alpha4;
    uint32_t n;
    float nPaths;   // (float)count of EPhoton's `count * md2 * M_PI`
};
struct RadLoArgs {
    RadMap map[3];   // in the order ComputeRadianceTask adds them: direct, indirect, caustic
    const float *rpP, *rpN, *rhoR, *rhoT;
    uint32_t nRp;
    int32_t k;       // nLookup
    float maxDist, maxD2;
    float *lo;       // [nRp][30]
};
struct RadNearestArgs {
    RadWalk w;                  // the radiance map's grid and normals (pvol_radwalk_dev.h)
    const float4 *lo4;          // its 32-float rows (Lo)
    const float *qp, *qn;
    uint32_t count;
    float *lo;
    uint32_t *found;
};

// EPhoton (photonshooter.cpp:17-35) of one map for the wave's radiance photon, both sides at once: lanes 0..31 return bin
// (lane & 31) of E(n), lanes 32..63 of E(-n) -- Dot(-n, wi) > 0 exactly when Dot(n, wi) < 0.  The wave streams the photons of the
// ball's cell rows: how many have d2 < maxD2 (the visit test, kdtree.h:180); when at least k do, md2 is the k-th smallest d2
// (PhotonProcess, photonshooter.h:186-203), found by bisection over the fp32 bit pattern, one pass per step; then the members'
// flux rows are added in stream order, lane = bin (ties at the k-th distance: the first in stream order).  No atomics.
__device__ __attribute__((noinline)) float ephoton_stream(const RadMap &M, V3 P, V3 N, int k, float maxDist, float maxD2, int lane) {
    const GridRows R = grid_rows<false>(M.g, P, maxDist, 0);
    uint32_t lo = 0u, hi = __float_as_uint(maxD2), kth = 0xffffffffu;
    int nIn = 0;
    for (int pass = 0; pass < 40; ++pass) {
        const bool counting = pass == 0;
        const uint32_t mid = lo + ((hi - lo) >> 1);
        int cnt = 0;
        for (int r = 0; r < R.nrows; ++r) {
            uint32_t start, rlen;
            grid_row_range<false>(M.g, R, r, P, maxD2, &start, &rlen);
            for (uint32_t b = 0; b < rlen; b += LANES) {
                const uint32_t i = b + (uint32_t)lane;
                bool in = false;
                if (i < rlen) {
                    const float4 q = M.g.pos4[start + i];
                    const float dx = q.x - P.x, dy = q.y - P.y, dz = q.z - P.z;
                    const float d2 = dx * dx + dy * dy + dz * dz;
                    in = counting ? d2 < maxD2 : __float_as_uint(d2) <= mid;
                }
                cnt += __popcll(__ballot(in));
            }
        }
        if (counting) { nIn = cnt; if (nIn < k) break; continue; }
        if (cnt >= k) hi = mid; else lo = mid + 1u;
        if (!(lo < hi)) { kth = lo; break; }
    }
    if (nIn == 0) return 0.f;   // `if (proc.nFound == 0) return Spectrum(0.f)`
    float md2 = maxD2;
    int tieQuota = 0;
    if (kth != 0xffffffffu) {
        md2 = __uint_as_float(kth);
        int less = 0;
        for (int r = 0; r < R.nrows; ++r) {
            uint32_t start, rlen;
            grid_row_range<false>(M.g, R, r, P, maxD2, &start, &rlen);
            for (uint32_t b = 0; b < rlen; b += LANES) {
                const uint32_t i = b + (uint32_t)lane;
                bool lt = false;
                if (i < rlen) {
                    const float4 q = M.g.pos4[start + i];
                    const float dx = q.x - P.x, dy = q.y - P.y, dz = q.z - P.z;
                    lt = __float_as_uint(dx * dx + dy * dy + dz * dz) < kth;
                }
                less += __popcll(__ballot(lt));
            }
        }
        tieQuota = k - less;
    }
    const int bin = lane & 31, mySide = lane < 32 ? 1 : 2;
    const float *rows = (const float *)M.alpha4;
    float sum = 0.f;
    int tiesSeen = 0;
    for (int r = 0; r < R.nrows; ++r) {
        uint32_t start, rlen;
        grid_row_range<false>(M.g, R, r, P, maxD2, &start, &rlen);
        for (uint32_t b = 0; b < rlen; b += LANES) {
            const uint32_t i = b + (uint32_t)lane;
            bool mem = false, tie = false;
            if (i < rlen) {
                const float4 q = M.g.pos4[start + i];
                const float dx = q.x - P.x, dy = q.y - P.y, dz = q.z - P.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (kth == 0xffffffffu) mem = d2 < maxD2;
                else { const uint32_t bits = __float_as_uint(d2); mem = bits < kth; tie = bits == kth; }
            }
            const unsigned long long tb = __ballot(tie);
            if (tie) mem = tiesSeen + __popcll(tb & ((1ull << lane) - 1ull)) < tieQuota;
            tiesSeen += __popcll(tb);
            int side = 0;   // 1: Dot(n, wi) > 0, 2: Dot(-n, wi) > 0, 0: neither
            if (mem) {
                const float4 w = M.wi4[start + i];
                const float d = N.x * w.x + N.y * w.y + N.z * w.z;
                side = d > 0.f ? 1 : (d < 0.f ? 2 : 0);
            }
            unsigned long long mb = __ballot(side != 0);
            while (mb) {   // wave-uniform: one member at a time, its 128-B row read by the whole wave
                const int j = __ffsll((long long)mb) - 1;
                mb &= mb - 1ull;
                const uint32_t idx = start + b + (uint32_t)j;
                const int sj = __shfl(side, j);
                const float v = rows[(size_t)idx * 32 + bin];
                if (sj == mySide) sum += v;
            }
        }
    }
    return sum / ((M.nPaths * md2) * K_PI);
}

// ComputeRadianceTask::Run (photonshooter.cpp:359-395): one wave per radiance photon
__global__ __launch_bounds__(256) void radiance_lo_kernel(const RadLoArgs *__restrict__ args) {
    const RadLoArgs &A = *args;   // in device memory: the maps are indexed, and a by-value argument indexed so would move to scratch
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= A.nRp) return;
    const V3 P = v3(A.rpP[3 * (size_t)w], A.rpP[3 * (size_t)w + 1], A.rpP[3 * (size_t)w + 2]);
    const V3 N = v3(A.rpN[3 * (size_t)w], A.rpN[3 * (size_t)w + 1], A.rpN[3 * (size_t)w + 2]);
    float rr = 0.f, rt = 0.f;
    if (lane < 30) { rr = A.rhoR[30 * (size_t)w + lane]; rt = A.rhoT[30 * (size_t)w + lane]; }
    const bool doR = __ballot(rr != 0.f) != 0ull, doT = __ballot(rt != 0.f) != 0ull;   // !rho.IsBlack()
    float E = 0.f;
    if (doR || doT) {
        for (int m = 0; m < 3; ++m)
            if (A.map[m].n) E = E + ephoton_stream(A.map[m], P, N, A.k, A.maxDist, A.maxD2, lane);
    }
    const float Et = __shfl(E, (lane & 31) + 32);
    if (lane < 30) {
        float Lo = 0.f;
        if (doR) Lo += (rr * K_INV_PI) * E;
        if (doT) Lo += (rt * K_INV_PI) * Et;
        A.lo[30 * (size_t)w + lane] = Lo;
    }
}

// radianceMap->Lookup(p, RadiancePhotonProcess(n), INFINITY): one query per lane; the walk itself is radiance_nearest
// (pvol_radwalk_dev.h), shared with the final gather.
__global__ __launch_bounds__(256) void radiance_nearest_kernel(RadNearestArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.count) return;
    const float q[3] = {A.qp[3 * (size_t)i], A.qp[3 * (size_t)i + 1], A.qp[3 * (size_t)i + 2]};
    const int64_t bestIdx = radiance_nearest(A.w, q, A.qn[3 * (size_t)i], A.qn[3 * (size_t)i + 1], A.qn[3 * (size_t)i + 2]);
    A.found[i] = bestIdx >= 0 ? 1u : 0u;
    const float *row = bestIdx >= 0 ? (const float *)A.lo4 + (size_t)bestIdx * 32 : 0;
    for (int b = 0; b < 30; ++b) A.lo[30 * (size_t)i + b] = row ? row[b] : 0.f;
}

// ------------------------------------------------------------------------------------------ host

static bool all_finite(const float *v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

static RadMap rad_map(const PhotonGrid &G, uint32_t nPaths) {
    RadMap m;
    memset(&m, 0, sizeof(m));
    m.g.cellSize = G.cellSize; m.g.invCell = G.invCell;
    for (int a = 0; a < 3; ++a) { m.g.gridLo[a] = G.gridLo[a]; m.g.gdim[a] = G.gdim[a]; }
    m.g.cellStart = G.cellStart.get(); m.g.subStart = 0; m.g.pos4 = G.pos4.get();
    m.wi4 = G.wi4.get(); m.alpha4 = G.alpha4.get(); m.n = G.n; m.nPaths = (float)(int32_t)nPaths;
    return m;
}

// One surface map where the device can read it: raw = {p, wi, alpha}, the host copy of p for the grid's box
struct MapSource { const float *raw[3]; const float *hostP; uint32_t n, nPaths; };

// The radiance photons (host arrays) against the three maps (kind order: caustic, direct, indirect): Lo, then the radiance map.
// Builds everything aside and hands it to the context only when all of it succeeded.
static int compute_radiance(pvol_ctx *c, int32_t k, float maxDist, const MapSource src[3], const float *rpP, const float *rpN, const float *rhoR,
                            const float *rhoT, uint32_t nRp) {
    RadianceResult out;
    out.have = true; out.n = nRp;
    if (nRp) {
        MapFilter all;   // no Inside() filter: surface photons count wherever they lie
        memset(&all, 0, sizeof(all));
        all.volKind = PVOL_VOLUME_GRID;
        RadLoArgs A;
        memset(&A, 0, sizeof(A));
        PhotonGrid G[3];
        const int order[3] = {1, 2, 0};   // direct + indirect + caustic (photonshooter.cpp:374-379)
        const double first = 0.5 * maxDist;
        for (int m = 0; m < 3; ++m) {
            const MapSource &s = src[order[m]];
            if (!s.n) continue;
            int rc = build_photon_grid(G[m], s.raw, s.hostP, s.n, 1e-3 * maxDist, [first](double) { return first; }, all);
            if (rc != PVOL_OK) return rc;
            A.map[m] = rad_map(G[m], s.nPaths);
        }
        DevPtr<float> dRhoR, dRhoT;
        DevPtr<RadLoArgs> dArgs;
        if (!dArgs.alloc(1)) return PVOL_E_NO_MEMORY;
        if (!out.p.alloc(3 * (size_t)nRp) || !out.nrm.alloc(3 * (size_t)nRp) || !out.lo.alloc(30 * (size_t)nRp) || !dRhoR.alloc(30 * (size_t)nRp) ||
            !dRhoT.alloc(30 * (size_t)nRp))
            return PVOL_E_NO_MEMORY;
        if (!ok(hipMemcpy(out.p.get(), rpP, sizeof(float) * 3 * (size_t)nRp, hipMemcpyHostToDevice)) ||
            !ok(hipMemcpy(out.nrm.get(), rpN, sizeof(float) * 3 * (size_t)nRp, hipMemcpyHostToDevice)) ||
            !ok(hipMemcpy(dRhoR.get(), rhoR, sizeof(float) * 30 * (size_t)nRp, hipMemcpyHostToDevice)) ||
            !ok(hipMemcpy(dRhoT.get(), rhoT, sizeof(float) * 30 * (size_t)nRp, hipMemcpyHostToDevice)))
            return PVOL_E_NO_DEVICE;
        A.rpP = out.p.get(); A.rpN = out.nrm.get(); A.rhoR = dRhoR.get(); A.rhoT = dRhoT.get();
        A.nRp = nRp; A.k = k; A.maxDist = maxDist; A.maxD2 = maxDist * maxDist; A.lo = out.lo.get();
        if (!ok(hipMemcpy(dArgs.get(), &A, sizeof(A), hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
        hipLaunchKernelGGL(radiance_lo_kernel, dim3((nRp + 3) / 4), dim3(256), 0, 0, (const RadLoArgs *)dArgs.get());
        if (!ok(hipGetLastError()) || !ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;
        // the radiance map: photons lie on surfaces, so a grid of cell edge e over a box of surface area S has about S / e^2
        // occupied cells; e = sqrt(2 S / n) aims at two photons in each
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = 0; i < nRp; ++i)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], rpP[3 * (size_t)i + a]); hi[a] = std::max(hi[a], rpP[3 * (size_t)i + a]); }
        double ext[3], diag = 0;
        for (int a = 0; a < 3; ++a) { ext[a] = (double)hi[a] - lo[a]; diag = std::max(diag, ext[a]); }
        const double minExt = diag > 0 ? 1e-3 * diag : 1e-3;
        for (int a = 0; a < 3; ++a) ext[a] = std::max(ext[a], minExt);
        const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
        const double cell = sqrt(2.0 * area / nRp);
        const float *const raw[3] = {out.p.get(), out.nrm.get(), out.lo.get()};
        int rc = build_photon_grid(out.map, raw, rpP, nRp, minExt, [cell](double) { return cell; }, all);
        if (rc != PVOL_OK) return rc;
    }
    c->rad = std::move(out);
    return PVOL_OK;
}

RadWalk pvol_radiance_walk(const pvol_ctx *c) {
    const PhotonGrid &G = c->rad.map;
    RadWalk w;
    memset(&w, 0, sizeof(w));
    w.g = rad_map(G, 1).g;
    w.nrm4 = G.wi4.get(); w.n = c->rad.n ? G.n : 0u;
    // photons are put into cells by floor((x - lo) * inv) in fp32: a shell's bound gives way by 1e-4 cell plus the rounding of the
    // largest cell index
    w.eps = G.cellSize * (1e-4f + 1e-6f * (float)std::max(G.gdim[0], std::max(G.gdim[1], G.gdim[2])));
    return w;
}

static hipError_t launch_nearest(const pvol_ctx *c, const float *dP, const float *dN, uint32_t count, float *dLo, uint32_t *dFound, hipStream_t stream) {
    RadNearestArgs A;
    memset(&A, 0, sizeof(A));
    A.w = pvol_radiance_walk(c);
    A.lo4 = c->rad.map.alpha4.get();
    A.qp = dP; A.qn = dN; A.count = count; A.lo = dLo; A.found = dFound;
    hipLaunchKernelGGL(radiance_nearest_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, A);
    return hipGetLastError();
}

extern "C" {

int pvol_check_radiance(int what, int haveCtx, int haveState, int32_t nLookup, float maxDist, const pvol_photon_array *const *maps, const float *a,
                        const float *b, const float *rhoR, const float *rhoT, uint32_t count, const void *outLo, const void *outFound, int hostPointers) {
    if (!haveCtx || what < 0 || what > 2) return PVOL_E_INVALID;
    if (what == 2) {   // a lookup
        if (!haveState) return PVOL_E_INVALID;   // before any compute
        if (count && (!a || !b || !outLo || !outFound)) return PVOL_E_INVALID;
        if (hostPointers && count && (!all_finite(a, 3 * (size_t)count) || !all_finite(b, 3 * (size_t)count))) return PVOL_E_INVALID;
        return PVOL_OK;
    }
    if (nLookup < 1 || !(maxDist > 0.f) || !std::isfinite(maxDist)) return PVOL_E_INVALID;
    if (what == 0) {
        if (!haveState) return PVOL_E_INVALID;   // no kept stores
    } else {
        if (!maps) return PVOL_E_INVALID;
        if (count && (!a || !b || !rhoR || !rhoT)) return PVOL_E_INVALID;
        for (int m = 0; m < 3; ++m) {
            const pvol_photon_array *M = maps[m];
            if (!M || !M->n) continue;
            if (!M->p || !M->wi || !M->alpha || !M->n_paths) return PVOL_E_INVALID;
            if (hostPointers && (!all_finite(M->p, 3 * (size_t)M->n) || !all_finite(M->wi, 3 * (size_t)M->n) || !all_finite(M->alpha, 30 * (size_t)M->n)))
                return PVOL_E_INVALID;
        }
        if (hostPointers && count &&
            (!all_finite(a, 3 * (size_t)count) || !all_finite(b, 3 * (size_t)count) || !all_finite(rhoR, 30 * (size_t)count) ||
             !all_finite(rhoT, 30 * (size_t)count)))
            return PVOL_E_INVALID;
    }
    if (nLookup > RAD_MAX_LOOKUP) return PVOL_E_UNSUPPORTED;
    return PVOL_OK;
}

int pvol_compute_radiance(pvol_ctx *c, int32_t nLookup, float maxDist) {
    int rc = pvol_check_radiance(0, c != 0, c && c->surfKept, nLookup, maxDist, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->surfKept) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    // the stores stay on the device; their positions come back once for the grids' boxes (as pvol_set_surface_integrator does)
    std::vector<float> hp[3];
    MapSource src[3];
    for (int kind = 0; kind < 3; ++kind) {
        const pvol_ctx::SurfStore &st = c->surf[kind];
        hp[kind].resize(3 * (size_t)st.n);
        if (st.n && !ok(hipMemcpy(hp[kind].data(), st.p.get(), sizeof(float) * 3 * (size_t)st.n, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
        if (st.n && !st.nPaths) return PVOL_E_INVALID;
        src[kind] = MapSource{{st.p.get(), st.wo.get(), st.alpha.get()}, hp[kind].data(), st.n, st.nPaths};
    }
    const uint32_t n = c->nRad;
    std::vector<float> p(3 * (size_t)n), nrm(3 * (size_t)n), rhoR(30 * (size_t)n), rhoT(30 * (size_t)n);
    if (n && (rc = pvol_download_radiance_photons(c, p.data(), nrm.data(), rhoR.data(), rhoT.data(), n)) != PVOL_OK) return rc;
    return compute_radiance(c, nLookup, maxDist, src, p.data(), nrm.data(), rhoR.data(), rhoT.data(), n);
}

int pvol_compute_radiance_arrays(pvol_ctx *c, int32_t nLookup, float maxDist, const pvol_photon_array *const maps[3], const float *rpP, const float *rpN,
                                 const float *rhoR, const float *rhoT, uint32_t nRp) {
    int rc = pvol_check_radiance(1, c != 0, 0, nLookup, maxDist, maps, rpP, rpN, rhoR, rhoT, nRp, 0, 0, 1);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    DevPtr<float> up[3][3];
    MapSource src[3];
    const size_t width[3] = {3, 3, 30};
    for (int kind = 0; kind < 3; ++kind) {
        src[kind] = MapSource{{0, 0, 0}, 0, 0, 0};
        const pvol_photon_array *M = maps[kind];
        if (!M || !M->n || !nRp) continue;
        const float *h[3] = {M->p, M->wi, M->alpha};
        for (int i = 0; i < 3; ++i) {
            if (!up[kind][i].alloc(width[i] * (size_t)M->n)) return PVOL_E_NO_MEMORY;
            if (!ok(hipMemcpy(up[kind][i].get(), h[i], sizeof(float) * width[i] * (size_t)M->n, hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
            src[kind].raw[i] = up[kind][i].get();
        }
        src[kind].hostP = M->p; src[kind].n = M->n; src[kind].nPaths = M->n_paths;
    }
    return compute_radiance(c, nLookup, maxDist, src, rpP, rpN, rhoR, rhoT, nRp);
}

int pvol_radiance_lo_count(pvol_ctx *c, uint32_t *n) {
    if (!c || !n) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // a concurrent compute moves its result into c->rad under it
    *n = c->rad.have ? c->rad.n : 0u;
    return PVOL_OK;
}

int pvol_download_radiance_lo(pvol_ctx *c, float *p, float *nrm, float *lo, uint32_t capacity) {
    if (!c || !p || !nrm || !lo) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    const uint32_t n = std::min(capacity, c->rad.have ? c->rad.n : 0u);
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const bool good = ok(hipMemcpy(p, c->rad.p.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                      ok(hipMemcpy(nrm, c->rad.nrm.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                      ok(hipMemcpy(lo, c->rad.lo.get(), sizeof(float) * 30 * (size_t)n, hipMemcpyDeviceToHost));
    return good ? PVOL_OK : PVOL_E_NO_DEVICE;
}

int pvol_radiance_lookup(pvol_ctx *c, const float *p, const float *n, uint32_t count, float *lo, uint32_t *found) {
    int rc = pvol_check_radiance(2, c != 0, c && c->rad.have, 0, 0.f, 0, p, n, 0, 0, count, lo, found, 1);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->rad.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    HostStage st;
    const float *dP = st.in(p, 3 * (size_t)count), *dN = st.in(n, 3 * (size_t)count);
    float *dLo = st.out(lo, 30 * (size_t)count);
    uint32_t *dFound = st.out(found, count);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    if (!ok(launch_nearest(c, dP, dN, count, dLo, dFound, 0))) return PVOL_E_NO_DEVICE;
    return st.download();   // the copy-back on the null stream waits for the kernel
}

int pvol_radiance_lookup_device(pvol_ctx *c, const float *dP, const float *dN, uint32_t count, float *dLo, uint32_t *dFound, void *hipStream) {
    int rc = pvol_check_radiance(2, c != 0, c && c->rad.have, 0, 0.f, 0, dP, dN, 0, 0, count, dLo, dFound, 0);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->rad.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    return ok(launch_nearest(c, dP, dN, count, dLo, dFound, (hipStream_t)hipStream)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

}  // extern "C"
