// pvol_lphoton.hip -- the host side of pvol_lphoton_batch*: PhotonVolumeIntegrator::LPhoton (integrators/photonvolume.cpp:65-108)
// on the current volume map at points the caller names.  The lookups are lphoton_points_kernel's (pvol_points_dev.h,
// compiled in pvol_march.hip and, for the exponential medium, pvol_march_exp.hip); this unit checks the call, walks the points in
// slices, orders every slice by the map's grid cell (pvol_order_points, pvol_grid.hip) and launches.  No atomics anywhere: two runs
// agree byte for byte, and a point's bytes do not depend on which other points share the call, on the slicing or on the ordering.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>

#include "pvol_host.h"

extern "C" {

int pvol_check_lphoton(int haveCtx, const LPhotonCheck *a, int haveScene, float g) {
    if (!haveCtx || !a) return PVOL_E_INVALID;
    if (a->outputKind != PVOL_OUT_SPECTRAL && a->outputKind != PVOL_OUT_XYZ) return PVOL_E_INVALID;
    if (a->n && (!a->p || !a->out)) return PVOL_E_INVALID;
    if (a->n && !a->w && haveScene && g != 0.f) return PVOL_E_INVALID;   // the phase function reads the direction
    if (!haveScene) return PVOL_E_NO_SCENE;
    return PVOL_OK;
}

uint32_t pvol_lphoton_slice(uint64_t bound) {
    // the header's bound is the largest: a slice then holds at most 2^22 points, well inside the sort's int count
    return pvol_slice_items(bound, PVOL_LPHOTON_SCRATCH_BYTES, PVOL_LPHOTON_POINT_SCRATCH);
}

int pvol_lphoton_set_scratch_bound(pvol_ctx *c, uint64_t bytes) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    c->lp.bound = std::min<uint64_t>(bytes, PVOL_LPHOTON_SCRATCH_BYTES);   // the hook only lowers the bound
    return PVOL_OK;
}

static int check_ctx(const pvol_ctx *c, const LPhotonCheck *a) {
    return pvol_check_lphoton(c != 0, a, c && c->haveScene, c && c->haveScene ? c->hs.g : 0.f);
}

int pvol_lphoton_batch_device(pvol_ctx *c, const float *dP, const float *dW, uint32_t n, int outputKind, float *dOut, uint32_t *dNFound,
                              float *dRadius2, void *hipStream) {
    const LPhotonCheck a = {dP, dW, n, outputKind, dOut};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);   // the context's state is read under the lock only
    const int rc0 = check_ctx(c, &a);
    if (rc0 != PVOL_OK) return rc0;
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipStream_t stream = (hipStream_t)hipStream;
    const bool spectral = outputKind == PVOL_OUT_SPECTRAL;
    const PhotonGrid &G = c->volMap;
    if (!G.n) {   // no map, or an empty one: LPhoton finds nothing anywhere
        if (!ok(hipMemsetAsync(dOut, 0, sizeof(float) * (spectral ? 30 : 4) * (size_t)n, stream)) ||
            (dNFound && !ok(hipMemsetAsync(dNFound, 0, sizeof(uint32_t) * (size_t)n, stream))) ||
            (dRadius2 && !ok(hipMemsetAsync(dRadius2, 0, sizeof(float) * (size_t)n, stream))))
            return PVOL_E_NO_DEVICE;
        return PVOL_OK;
    }
    // an earlier call's kernels, on whatever stream, may still read the ordering scratch
    if (!c->lp.fence.wait(stream)) return PVOL_E_NO_DEVICE;
    const uint32_t slice = std::min(n, pvol_lphoton_slice(c->lp.bound));
    const bool sort = !c->knobs.lpNoSort;
    size_t tempBytes = 0;
    uint32_t *work = 0;
    if (sort) {
        if (!pvol_reserve(c->buf[PVOL_BUF_LP_ORDER], (size_t)PVOL_LPHOTON_POINT_SCRATCH * slice, stream)) return PVOL_E_NO_MEMORY;
        work = pvol_buf<uint32_t>(c, PVOL_BUF_LP_ORDER);
        if (!ok(pvol_order_points(&G, dP, 0, slice, work, 0, &tempBytes, stream))) return PVOL_E_NO_DEVICE;   // the first slice is the largest
        if (!pvol_reserve(c->buf[PVOL_BUF_LP_TEMP], std::max<size_t>(tempBytes, 16), stream)) return PVOL_E_NO_MEMORY;
    }
    PointsArgs A;
    memset(&A, 0, sizeof(A));
    A.scene = c->ds.get();
    A.p = dP; A.w = dW;
    A.spectral = spectral;
    A.out = dOut; A.nFound = dNFound; A.radius2 = dRadius2;
    const RegionLaunchers &launch = pvol_launchers(c->hs.volKind);
    const uint32_t maxWaves = (uint32_t)std::max(1, c->nCU * c->knobs.fixWavesPerCU);
    // the slices follow one another on the stream, so each may reuse the scratch of the one before
    for (uint32_t q0 = 0; q0 < n; q0 += slice) {
        const uint32_t m = std::min(slice, n - q0);
        A.first = q0; A.n = m;
        if (sort) {
            size_t tb = c->buf[PVOL_BUF_LP_TEMP].bytes;
            if (!ok(pvol_order_points(&G, dP, q0, m, work, pvol_buf<unsigned char>(c, PVOL_BUF_LP_TEMP), &tb, stream))) return PVOL_E_NO_DEVICE;
            A.order = work + 3 * (size_t)m;
        }
        const uint32_t nRuns = (m + 63u) / 64u;
        const uint32_t nWaves = std::min(maxWaves, (nRuns + 7u) / 8u);
        if (!ok(launch.lphotonPoints(&A, c->hs.candCap, nWaves, stream))) return PVOL_E_NO_DEVICE;
    }
    return c->lp.fence.record(stream) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

int pvol_lphoton_batch(pvol_ctx *c, const float *p, const float *w, uint32_t n, int outputKind, float *out, uint32_t *nFound, float *radius2) {
    const LPhotonCheck a = {p, w, n, outputKind, out};
    if (!c) return check_ctx(0, &a);
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    int rc = check_ctx(c, &a);
    if (rc != PVOL_OK) return rc;
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    HostStage st;
    const float *dP = st.in(p, 3 * (size_t)n), *dW = st.in(w, 3 * (size_t)n);
    float *dOut = st.out(out, (size_t)(outputKind == PVOL_OUT_SPECTRAL ? 30 : 4) * n);
    uint32_t *dNF = st.out(nFound, n);
    float *dR2 = st.out(radius2, n);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = pvol_lphoton_batch_device(c, dP, dW, n, outputKind, dOut, dNF, dR2, 0);
    if (rc != PVOL_OK) return rc;
    if (!ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;   // nothing is written unless all of it ran
    return st.download();
}

}  // extern "C"
