// pvol_gather.hip -- the sampling half of the final gather (integrators/photonmap.cpp:183-219, :248-265 and the weights of
// :233-243, :280-291): the 50 nearest indirect photons in the order PhotonProcess leaves its heap in, and the two loops that turn
// them and the sampler's draws into gather-ray directions with their MIS weights.  The rays are not traced here and Lindir is not
// looked up.  The heap's layout depends on the kd-tree's visiting order, so the map is the reference's kd-tree
// itself, built on the host (pvol_gather_tree.h), and the lookup restates privateLookup (core/kdtree.h:157-183) and
// PhotonProcess::operator() (core/photonshooter.h:186-203) step by step, one query per lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "pvol_math.h"
#include "pvol_bsdf_dev.h"
#include "pvol_host.h"
#include "pvol_gather_tree.h"

#define GATHER_K 50                           // nIndirSamplePhotons (photonmap.cpp:190)
#define GATHER_STACK PVOL_GATHER_MAX_DEPTH    // one frame per node of the path from the root
#define GATHER_MAX_ROUNDS 300u                // from the smallest positive fp32 to +inf are 277 doublings: never reached
#define GATHER_NONE 0xffffffffu

struct GatherArgs {
    const float4 *nodes4;   // GatherNode as two float4: {p, splitPos}, {splitAxis, hasLeftChild, rightChild, index} (bit patterns)
    const float *wi;        // [n][3] Photon::wi in the store's order
    uint32_t n;
    const float *p;         // [count][3]
    uint32_t count;
    float maxDist;
    uint32_t *index;        // [count][50] store indices in heap order; 0: not wanted
    float *d2;              // [count][50]
    uint32_t *found, *rounds;
    // the two sampling loops
    const float *frames;    // [count][9] nn, dpdu, ng
    const float *wo;        // [count][3]
    const float *uBsdf, *uPhoton;   // [count][nSamples][3] uComponent, uDir[0], uDir[1]
    int32_t nSamples;
    float cosGather;
    pvol_gather_sample *outBsdf, *outPhoton;   // [count][nSamples]
};

typedef float HeapKeys[LANES];
typedef uint32_t HeapIds[LANES];

// ClosePhoton::operator< (photonshooter.h:44-47): by distance, a tie by the photon's address in nodeData, i.e. its node number
__device__ __forceinline__ bool close_less(float da, uint32_t na, float db, uint32_t nb) { return da == db ? na < nb : da < db; }

// libstdc++'s __push_heap: the value climbs from `hole` while its parent is smaller, not above `top`
__device__ __forceinline__ void heap_push(HeapKeys *hk, HeapIds *hn, int lane, int hole, int top, float vd, uint32_t vn) {
    int parent = (hole - 1) / 2;
    while (hole > top && close_less(hk[parent][lane], hn[parent][lane], vd, vn)) {
        hk[hole][lane] = hk[parent][lane]; hn[hole][lane] = hn[parent][lane];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    hk[hole][lane] = vd; hn[hole][lane] = vn;
}

// libstdc++'s __adjust_heap: the hole sinks along the larger child down to a leaf (an even length has one node with a lone left
// child), then the value is pushed back up from there
__device__ __forceinline__ void heap_adjust(HeapKeys *hk, HeapIds *hn, int lane, int hole, int len, float vd, uint32_t vn) {
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (close_less(hk[child][lane], hn[child][lane], hk[child - 1][lane], hn[child - 1][lane])) --child;
        hk[hole][lane] = hk[child][lane]; hn[hole][lane] = hn[child][lane];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        hk[hole][lane] = hk[child - 1][lane]; hn[hole][lane] = hn[child - 1][lane];
        hole = child - 1;
    }
    heap_push(hk, hn, lane, hole, top, vd, vn);
}

__device__ __forceinline__ float power_heuristic(int nf, float fPdf, int ng, float gPdf) {   // core/montecarlo.h:262-265
    const float f = nf * fPdf, g = ng * gPdf;
    return (f * f) / (f * f + g * g);
}

__device__ __forceinline__ void put_sample(pvol_gather_sample *o, V3 wi, float weight, float bsdfPdf, float photonPdf, uint32_t index, bool valid) {
    float4 *o4 = reinterpret_cast<float4 *>(o);
    if (!valid) { wi = v3(0.f, 0.f, 0.f); weight = bsdfPdf = photonPdf = 0.f; }
    o4[0] = make_float4(wi.x, wi.y, wi.z, weight);
    o4[1] = make_float4(bsdfPdf, photonPdf, __uint_as_float(index), __uint_as_float(valid ? 1u : 0u));
}

// One query per lane, one wave per block.  The lane's heap is a column of LDS: entry e of lane l at [e][l], so whatever entries
// the lanes of a wave touch, they touch 64 different banks.  The traversal's stack of (node, state) frames lies next to it.
template <bool DIRS> __global__ __launch_bounds__(LANES) void gather_lookup_kernel(GatherArgs A) {
    __shared__ float hk[GATHER_K][LANES];
    __shared__ uint32_t hn[GATHER_K][LANES];
    __shared__ uint32_t stk[GATHER_STACK][LANES];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * LANES + (uint32_t)lane;
    if (i >= A.count) return;
    const float q[3] = {A.p[3 * (size_t)i], A.p[3 * (size_t)i + 1], A.p[3 * (size_t)i + 2]};
    // photonmap.cpp:193-199: the ball doubles (in d^2) until it holds 50 photons
    float searchDist2 = A.maxDist * A.maxDist;
    uint32_t rounds = 0;
    int nFound = 0;
    for (;;) {
        const float roundMd2 = searchDist2;
        float md2 = roundMd2;
        nFound = 0;
        // privateLookup (kdtree.h:157-183) with its recursion as a stack: state 0 = entered, 1 = the near child has returned,
        // 2 = both children have
        int sp = 1;
        stk[0][lane] = 0u;
        while (sp > 0) {
            const uint32_t frame = stk[sp - 1][lane];
            const uint32_t node = frame & 0xffffffu, state = frame >> 24;
            const float4 nb = A.nodes4[2 * (size_t)node + 1];
            const uint32_t axis = __float_as_uint(nb.x);
            if (axis != 3u && state < 2u) {
                const float split = A.nodes4[2 * (size_t)node].w;
                const float pa = axis == 0u ? q[0] : (axis == 1u ? q[1] : q[2]);
                const uint32_t left = __float_as_uint(nb.y) && node + 1u < A.n ? node + 1u : GATHER_NONE;
                const uint32_t right = __float_as_uint(nb.z) < A.n ? __float_as_uint(nb.z) : GATHER_NONE;
                const bool leftNear = pa <= split;
                uint32_t next;
                if (state == 0u) {
                    next = leftNear ? left : right;
                } else {   // the far side, judged by the maxDistSquared the near side left behind
                    const float dist2 = (pa - split) * (pa - split);
                    next = leftNear ? right : left;
                    if (!(dist2 < md2)) next = GATHER_NONE;
                }
                stk[sp - 1][lane] = node | ((state + 1u) << 24);
                if (next != GATHER_NONE && sp < GATHER_STACK) { stk[sp][lane] = next; ++sp; }   // sp < depth <= GATHER_STACK by construction
                continue;
            }
            --sp;
            const float4 na = A.nodes4[2 * (size_t)node];
            const float dx = na.x - q[0], dy = na.y - q[1], dz = na.z - q[2];
            const float dist2 = dx * dx + dy * dy + dz * dz;   // DistanceSquared, contraction off
            if (!(dist2 < md2)) continue;
            // PhotonProcess::operator() (photonshooter.h:186-203)
            if (nFound < GATHER_K) {
                hk[nFound][lane] = dist2; hn[nFound][lane] = node;
                if (++nFound == GATHER_K) {
                    for (int parent = (GATHER_K - 2) / 2; parent >= 0; --parent)   // std::make_heap
                        heap_adjust(hk, hn, lane, parent, GATHER_K, hk[parent][lane], hn[parent][lane]);
                    md2 = hk[0][lane];
                }
            } else {
                // std::pop_heap moves the root to the last place, which the new photon then overwrites: only the re-insertion
                // of the former last element matters; then std::push_heap of the new one
                heap_adjust(hk, hn, lane, 0, GATHER_K - 1, hk[GATHER_K - 1][lane], hn[GATHER_K - 1][lane]);
                heap_push(hk, hn, lane, GATHER_K - 1, 0, dist2, node);
                md2 = hk[0][lane];
            }
        }
        searchDist2 *= 2.f;
        ++rounds;
        // `while (proc.nFound < nIndirSamplePhotons)`; a round over the whole tree (md2 = +inf) that still holds fewer -- a
        // non-finite query, a d^2 that overflows -- ends the query where the reference would not return
        if (nFound == GATHER_K || !(roundMd2 < INFINITY) || rounds >= GATHER_MAX_ROUNDS) break;
    }
    // node numbers become store indices; the tail of a short result is zero
    for (int e = 0; e < GATHER_K; ++e) {
        if (e < nFound) hn[e][lane] = __float_as_uint(A.nodes4[2 * (size_t)hn[e][lane] + 1].w);
        else { hn[e][lane] = 0u; hk[e][lane] = 0.f; }
    }
    if (A.index) {
        for (int e = 0; e < GATHER_K; ++e) {
            A.index[GATHER_K * (size_t)i + e] = hn[e][lane];
            A.d2[GATHER_K * (size_t)i + e] = hk[e][lane];
        }
        A.found[i] = (uint32_t)nFound;
        A.rounds[i] = rounds;
    }
    if (!DIRS) return;

    const int nS = A.nSamples;
    pvol_gather_sample *oB = A.outBsdf + (size_t)i * nS, *oP = A.outPhoton + (size_t)i * nS;
    if (nFound < GATHER_K) {
        for (int s = 0; s < nS; ++s) {
            put_sample(oB + s, v3(0.f, 0.f, 0.f), 0.f, 0.f, 0.f, GATHER_NONE, false);
            put_sample(oP + s, v3(0.f, 0.f, 0.f), 0.f, 0.f, 0.f, GATHER_NONE, false);
        }
        return;
    }
    // the BSDF's frame (BSDF::BSDF, core/reflection.cpp:619-627)
    const float *fr = A.frames + 9 * (size_t)i;
    const V3 nn = v3(fr[0], fr[1], fr[2]), ng = v3(fr[6], fr[7], fr[8]);
    const BsdfFrame F = bsdf_frame(nn, v3(fr[3], fr[4], fr[5]));
    const V3 woW = v3(A.wo[3 * (size_t)i], A.wo[3 * (size_t)i + 1], A.wo[3 * (size_t)i + 2]);
    const float woZ = dot(woW, nn), woNg = dot(woW, ng);
    const float cosG = A.cosGather, thresh = .999f * cosG;
    const float conePdf = 1.f / (2.f * K_PI * (1.f - cosG));   // UniformConePdf, montecarlo.cpp:400-402
    for (int loop = 0; loop < 2; ++loop)
        for (int s = 0; s < nS; ++s) {
            const float *u = (loop ? A.uPhoton : A.uBsdf) + 3 * ((size_t)i * nS + s);
            V3 wi = v3(0.f, 0.f, 0.f);
            float bsdfPdf = 0.f;
            uint32_t chosen = GATHER_NONE;
            bool valid;
            if (loop == 0) {
                // BSDF::Sample_f over one Lambertian lobe (reflection.cpp:534-598; BxDF::Sample_f, :323-330)
                float dx, dy;
                concentric_disk<true>(u[1], u[2], &dx, &dy);
                V3 l = v3(dx, dy, sqrtf(fmaxf(0.f, 1.f - dx * dx - dy * dy)));
                if (woZ < 0.f) l.z *= -1.f;
                bsdfPdf = woZ * l.z > 0.f ? fabsf(l.z) * K_INV_PI : 0.f;
                valid = bsdfPdf != 0.f;
                wi = to_world(F, l);
            } else {
                // photonmap.cpp:253-260; a uComponent outside [0, 1) is clamped to a photon that exists
                const int photonNum = min(GATHER_K - 1, max(0, (int)floorf(fminf(fmaxf(u[0], 0.f), 1.f) * (float)GATHER_K)));
                chosen = hn[photonNum][lane];
                const V3 z = v3(A.wi[3 * (size_t)chosen], A.wi[3 * (size_t)chosen + 1], A.wi[3 * (size_t)chosen + 2]);
                V3 vx;
                if (fabsf(z.x) > fabsf(z.y)) {   // CoordinateSystem written out: coordinate_system() here moves gather_lookup_kernel<true> from 82 to 80 VGPRs
                    const float invLen = 1.f / sqrtf(z.x * z.x + z.z * z.z);
                    vx = v3(-z.z * invLen, 0.f, z.x * invLen);
                } else {
                    const float invLen = 1.f / sqrtf(z.y * z.y + z.z * z.z);
                    vx = v3(0.f, z.z * invLen, -z.y * invLen);
                }
                const V3 vy = cross(z, vx);
                // UniformSampleCone, the basis form (montecarlo.cpp:413-420)
                const float costheta = (1.f - u[1]) * cosG + u[1] * 1.f;
                const float sintheta = sqrtf(1.f - costheta * costheta);
                const float phi = u[2] * 2.f * K_PI;
                wi = (vx * (cos_rounded(phi) * sintheta) + vy * (sin_rounded(phi) * sintheta)) + z * costheta;
                const float wiZ = dot(wi, nn);   // BSDF::Pdf (reflection.cpp:601-616)
                bsdfPdf = woZ * wiZ > 0.f ? fabsf(wiZ) * K_INV_PI : 0.f;
                valid = true;
            }
            // f is black unless wi and wo lie on one side of the GEOMETRIC normal (reflection.cpp:585-591, :634-641)
            if (valid) valid = dot(wi, ng) * woNg > 0.f;
            float photonPdf = 0.f, weight = 0.f;
            if (valid) {
                for (int j = 0; j < GATHER_K; ++j) {   // photonmap.cpp:236-241 / :281-286
                    const size_t k = hn[j][lane];
                    if (A.wi[3 * k] * wi.x + A.wi[3 * k + 1] * wi.y + A.wi[3 * k + 2] * wi.z > thresh) photonPdf += conePdf;
                }
                photonPdf /= (float)GATHER_K;
                const float absDot = fabsf(dot(wi, nn));
                weight = loop ? absDot * power_heuristic(nS, photonPdf, nS, bsdfPdf) / photonPdf
                              : absDot * power_heuristic(nS, bsdfPdf, nS, photonPdf) / bsdfPdf;
            }
            put_sample((loop ? oP : oB) + s, wi, weight, bsdfPdf, photonPdf, chosen, valid);
        }
}

// ------------------------------------------------------------------------------------------ host

static bool all_finite(const float *v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// The tree over hostP on the host, then it and the photons' wi (dWi / hWi: [n][3] on the device or the host) into a GatherMap;
// built aside and handed to the context only when all of it succeeded.
static int build_gather(pvol_ctx *c, const float *hostP, const float *dWi, const float *hWi, uint32_t n) {
    std::vector<GatherNode> nodes(n);
    GatherMap out;
    out.have = true; out.n = n;
    out.depth = gather_tree_build(hostP, n, nodes.data());
    if (out.depth > GATHER_STACK) return PVOL_E_UNSUPPORTED;   // cannot happen for n <= 2^24
    static_assert(sizeof(GatherNode) == 2 * sizeof(float4), "the kernel reads a node as two float4");
    if (!out.nodes4.alloc(2 * (size_t)n) || !out.wi.alloc(3 * (size_t)n)) return PVOL_E_NO_MEMORY;
    if (!ok(hipMemcpy(out.nodes4.get(), nodes.data(), sizeof(GatherNode) * (size_t)n, hipMemcpyHostToDevice)) ||
        !ok(hipMemcpy(out.wi.get(), dWi ? dWi : hWi, sizeof(float) * 3 * (size_t)n, dWi ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)))
        return PVOL_E_NO_DEVICE;
    c->gather = std::move(out);
    return PVOL_OK;
}

static hipError_t launch_gather(const pvol_ctx *c, GatherArgs A, bool dirs, hipStream_t stream) {
    A.nodes4 = c->gather.nodes4.get(); A.wi = c->gather.wi.get(); A.n = c->gather.n;
    const dim3 grid((A.count + LANES - 1) / LANES), block(LANES);
    if (dirs) hipLaunchKernelGGL(gather_lookup_kernel<true>, grid, block, 0, stream, A);
    else hipLaunchKernelGGL(gather_lookup_kernel<false>, grid, block, 0, stream, A);
    return hipGetLastError();
}

extern "C" {

int pvol_gather_tree_build(const float *p, uint32_t n, void *nodes, int32_t *depth) {
    if (!depth || (n && (!p || !nodes))) return PVOL_E_INVALID;
    if (n && !all_finite(p, 3 * (size_t)n)) return PVOL_E_INVALID;
    if (n < 1 || n > PVOL_GATHER_MAX_PHOTONS) return PVOL_E_UNSUPPORTED;
    *depth = gather_tree_build(p, n, (GatherNode *)nodes);
    return PVOL_OK;
}

int pvol_check_gather(int what, int haveCtx, int haveState, uint32_t storeN, const GatherCheck *a, int hostPointers) {
    if (!haveCtx || what < 0 || what > 3 || (what != 0 && !a)) return PVOL_E_INVALID;
    if (what <= 1) {   // a build
        uint32_t n = storeN;
        if (what == 0) {
            if (!haveState) return PVOL_E_INVALID;   // no kept stores
        } else {
            const pvol_photon_array *M = a->indirect;
            if (!M) return PVOL_E_INVALID;
            n = M->n;
            if (n && (!M->p || !M->wi)) return PVOL_E_INVALID;
            if (hostPointers && n && (!all_finite(M->p, 3 * (size_t)n) || !all_finite(M->wi, 3 * (size_t)n))) return PVOL_E_INVALID;
        }
        if (n < GATHER_K || n > PVOL_GATHER_MAX_PHOTONS) return PVOL_E_UNSUPPORTED;
        return PVOL_OK;
    }
    // a lookup.  max_dist^2 must not underflow to zero either: `searchDist2 *= 2.f` would never leave it
    if (!(a->maxDist > 0.f) || !std::isfinite(a->maxDist) || !(a->maxDist * a->maxDist > 0.f)) return PVOL_E_INVALID;
    if (what == 2) {
        if (a->count && (!a->p || !a->outIndex || !a->outD2 || !a->outFound || !a->outRounds)) return PVOL_E_INVALID;
    } else {
        if (a->nSamples < 1 || a->nSamples > 256) return PVOL_E_INVALID;
        if (!(a->cosGatherAngle > -1.f && a->cosGatherAngle < 1.f)) return PVOL_E_INVALID;
        if (a->count && (!a->p || !a->frames || !a->wo || !a->uBsdf || !a->uPhoton || !a->outBsdf || !a->outPhoton)) return PVOL_E_INVALID;
    }
    if (!haveState) return PVOL_E_INVALID;   // before any build
    return PVOL_OK;
}

int pvol_build_gather_map(pvol_ctx *c) {
    int rc = pvol_check_gather(0, c != 0, c && c->surfKept, c ? c->surf[2].n : 0u, 0, 0);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    rc = pvol_check_gather(0, 1, c->surfKept, c->surf[2].n, 0, 0);   // again under the lock: a shoot may have run in between
    if (rc != PVOL_OK) return rc;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    const pvol_ctx::SurfStore &st = c->surf[2];
    std::vector<float> hp(3 * (size_t)st.n);
    if (!ok(hipMemcpy(hp.data(), st.p.get(), sizeof(float) * 3 * (size_t)st.n, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
    if (!all_finite(hp.data(), hp.size())) return PVOL_E_INVALID;
    return build_gather(c, hp.data(), st.wo.get(), 0, st.n);
}

int pvol_build_gather_map_arrays(pvol_ctx *c, const pvol_photon_array *indirect) {
    GatherCheck a;
    memset(&a, 0, sizeof(a));
    a.indirect = indirect;
    int rc = pvol_check_gather(1, c != 0, 0, 0, &a, 1);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    return build_gather(c, indirect->p, 0, indirect->wi, indirect->n);
}

int pvol_gather_map_count(pvol_ctx *c, uint32_t *n) {
    if (!c || !n) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    *n = c->gather.have ? c->gather.n : 0u;
    return PVOL_OK;
}

int pvol_gather_photons_device(pvol_ctx *c, const float *dP, uint32_t count, float maxDist, uint32_t *dIndex, float *dD2, uint32_t *dFound,
                               uint32_t *dRounds, void *hipStream) {
    GatherCheck a;
    memset(&a, 0, sizeof(a));
    a.p = dP; a.count = count; a.maxDist = maxDist; a.outIndex = dIndex; a.outD2 = dD2; a.outFound = dFound; a.outRounds = dRounds;
    int rc = pvol_check_gather(2, c != 0, c && c->gather.have, 0, &a, 0);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->gather.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    GatherArgs A;
    memset(&A, 0, sizeof(A));
    A.p = dP; A.count = count; A.maxDist = maxDist; A.index = dIndex; A.d2 = dD2; A.found = dFound; A.rounds = dRounds;
    return ok(launch_gather(c, A, false, (hipStream_t)hipStream)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

int pvol_gather_photons(pvol_ctx *c, const float *p, uint32_t count, float maxDist, uint32_t *index, float *d2, uint32_t *found, uint32_t *rounds) {
    GatherCheck a;
    memset(&a, 0, sizeof(a));
    a.p = p; a.count = count; a.maxDist = maxDist; a.outIndex = index; a.outD2 = d2; a.outFound = found; a.outRounds = rounds;
    int rc = pvol_check_gather(2, c != 0, c && c->gather.have, 0, &a, 1);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->gather.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    HostStage st;
    const float *dP = st.in(p, 3 * (size_t)count);
    uint32_t *dIndex = st.out(index, GATHER_K * (size_t)count);
    float *dD2 = st.out(d2, GATHER_K * (size_t)count);
    uint32_t *dFound = st.out(found, count), *dRounds = st.out(rounds, count);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = pvol_gather_photons_device(c, dP, count, maxDist, dIndex, dD2, dFound, dRounds, 0);
    return rc != PVOL_OK ? rc : st.download();   // the copy-back on the null stream waits for the kernel
}

int pvol_gather_directions_device(pvol_ctx *c, const float *dP, const float *dFrames, const float *dWo, uint32_t count, float maxDist, int32_t nSamples,
                                  float cosGatherAngle, const float *dUBsdf, const float *dUPhoton, pvol_gather_sample *dOutBsdf,
                                  pvol_gather_sample *dOutPhoton, void *hipStream) {
    GatherCheck a;
    memset(&a, 0, sizeof(a));
    a.p = dP; a.count = count; a.maxDist = maxDist; a.frames = dFrames; a.wo = dWo; a.uBsdf = dUBsdf; a.uPhoton = dUPhoton;
    a.nSamples = nSamples; a.cosGatherAngle = cosGatherAngle; a.outBsdf = dOutBsdf; a.outPhoton = dOutPhoton;
    int rc = pvol_check_gather(3, c != 0, c && c->gather.have, 0, &a, 0);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->gather.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    GatherArgs A;
    memset(&A, 0, sizeof(A));
    A.p = dP; A.count = count; A.maxDist = maxDist; A.frames = dFrames; A.wo = dWo; A.uBsdf = dUBsdf; A.uPhoton = dUPhoton;
    A.nSamples = nSamples; A.cosGather = cosGatherAngle; A.outBsdf = dOutBsdf; A.outPhoton = dOutPhoton;
    return ok(launch_gather(c, A, true, (hipStream_t)hipStream)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

int pvol_gather_directions(pvol_ctx *c, const float *p, const float *frames, const float *wo, uint32_t count, float maxDist, int32_t nSamples,
                           float cosGatherAngle, const float *uBsdf, const float *uPhoton, pvol_gather_sample *outBsdf, pvol_gather_sample *outPhoton) {
    GatherCheck a;
    memset(&a, 0, sizeof(a));
    a.p = p; a.count = count; a.maxDist = maxDist; a.frames = frames; a.wo = wo; a.uBsdf = uBsdf; a.uPhoton = uPhoton;
    a.nSamples = nSamples; a.cosGatherAngle = cosGatherAngle; a.outBsdf = outBsdf; a.outPhoton = outPhoton;
    int rc = pvol_check_gather(3, c != 0, c && c->gather.have, 0, &a, 1);
    if (rc != PVOL_OK) return rc;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!c->gather.have) return PVOL_E_INVALID;
    if (!count) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const size_t nU = 3 * (size_t)count * nSamples, nO = (size_t)count * nSamples;
    HostStage st;
    const float *dP = st.in(p, 3 * (size_t)count), *dFrames = st.in(frames, 9 * (size_t)count), *dWo = st.in(wo, 3 * (size_t)count);
    const float *dUB = st.in(uBsdf, nU), *dUP = st.in(uPhoton, nU);
    pvol_gather_sample *dOB = st.out(outBsdf, nO), *dOP = st.out(outPhoton, nO);
    if ((rc = st.upload()) != PVOL_OK) return rc;
    rc = pvol_gather_directions_device(c, dP, dFrames, dWo, count, maxDist, nSamples, cosGatherAngle, dUB, dUP, dOB, dOP, 0);
    return rc != PVOL_OK ? rc : st.download();   // the copy-back on the null stream waits for the kernel
}

}  // extern "C"
