// pvol_single.hip -- VolumeIntegrator "single": SingleScatteringIntegrator::Li (integrators/single.cpp:66-139) for gfx950.
// The march of photonvolume.cpp:112-222 with three statements changed: Tr is ACCUMULATED over the steps (single.cpp:101), every step
// adds Tr * Lve + Tr * sigma_s * p * Ld * nLights / pdf (:114, :131) and the sum is scaled by the step length once (:138).  No photon
// map is read.  The RNG traffic is the photon integrator's: 4 + 6n for the three LD arrays, one draw per step, one per roulette test,
// one per unoccluded light sample.
//   single_seq_kernel  one wave per MT19937 stream, the state in LDS, every branch of the reference: the lightNum shuffle for several
//                      lights, drawn tau() offsets for a density region, the roulette on the accumulated Tr.
//   single_par_kernel  one wave per ray, ONE MARCH STEP PER LANE.  Legal where no drawn value reaches the result (at most one light,
//                      a homogeneous extent): with no gather nothing per step is serial, and the accumulated transmittance of a
//                      homogeneous extent is exp(-sigma_t * prefix length) -- one prefix sum over the wave.  A ray whose accumulated
//                      Tr.y() comes near the roulette raises the batch's needSeq flag (single_seq_kernel then redoes the batch).
// Its own unit, compiled a second time over an exponential medium (pvol_single_exp.hip), so that every other code object is what it
// was.  The small helpers it shares with pvol_march.hip's kernels by text (stream_of, the two tau() lengths) stand here a second time
// for the same reason.
#include "pvol_math.h"

#include "pvol_liargs.h"
#include "pvol_rng_dev.h"
#include "pvol_light_dev.h"
#include "pvol_closest_dev.h"   // scene_occluded, lane_occluded

#define SINGLE_CHUNK_RAYS 64

// tau() length of a homogeneous extent along a general segment (homogeneous.h:80-84): Distance(ray(t0), ray(t1))
__device__ __forceinline__ float single_tau_length(const DevScene &S, V3 o, V3 d, float mint, float maxt) {
    RayD r;
    r.o = o; r.d = d; r.mint = mint; r.maxt = maxt;
    float t0, t1;
    if (!vol_intersect(S, r, &t0, &t1)) return 0.f;
    V3 a = o + d * t0, b = o + d * t1;
    return len(a - b);
}
// ... and along a ray that STARTS INSIDE it (mint == 0): BBox::IntersectP (core/geometry.cpp:68-86) leaves t0 == 0 exactly, so only the
// far slab distances remain.  pv = WorldToVolume(o), dvInv = 1 / WorldToVolume(d) per axis.
__device__ __forceinline__ float single_exit_length(const DevScene &S, V3 o, V3 d, V3 pv, V3 dvInv, float maxt) {
    float t1 = maxt;
    const float pp[3] = {pv.x, pv.y, pv.z}, ii[3] = {dvInv.x, dvInv.y, dvInv.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float tn = (S.extLo[i] - pp[i]) * ii[i];
        float tf = (S.extHi[i] - pp[i]) * ii[i];
        if (tn > tf) tf = tn;
        t1 = tf < t1 ? tf : t1;
    }
    V3 a = o + d * 0.f, b = o + d * t1;
    return len(a - b);
}

// stream of ray `ri`: streams are sorted by first_ray and cover disjoint ranges
__device__ __forceinline__ uint32_t single_stream_of(const pvol_stream *st, uint32_t n, uint32_t ri) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (st[mid].first_ray <= ri) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void single_stream_begin_kernel(pvol_stream *st, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st[i].end_draw = st[i].start_draw;
}

// ------------------------------------------------------------------------------------------ sequential form
// One call of SingleScatteringIntegrator::Li on the wave's live stream.  Spectra in the "8 lanes x float4" layout of the march kernels.
// `lightNum`: LDS, S.maxSteps floats (read with more than one light only).  tauRec: *T as {summed tau() length inside the extent,
// product of the roulette factors} -- T = scale * exp(-sigma_t * len) for an analytic medium.
__device__ void single_march_seq(const DevScene &S, const LiArgs &A, const pvol_ray &pr, Rng &rng, float *lightNum, int lane,
                                 unsigned long long &steps, f4 *LvOut, f4 *TrOut, TauRec *tauRec, size_t ri) {
    const int q = lane & 7;
    const f4 sigA = ld4(S.sigA, q), sigS = ld4(S.sigS, q);
    const f4 sigT = sigA + sigS;
    const f4 Y = ld4(S.cieY, q), le = ld4(S.le, q);
    const int nLights = S.nLights;
    const bool analytic = !is_region(S.volKind);
    RayD ray;
    ray.o = v3(pr.o[0], pr.o[1], pr.o[2]);
    ray.d = v3(pr.d[0], pr.d[1], pr.d[2]);
    ray.mint = pr.mint;
    ray.maxt = pr.maxt;
    f4 Lv = mk4(0.f), Tr = mk4(1.f);
    float tLen = 0.f, tScale = 1.f;
    float t0, t1;
    bool hit = S.volKind != PVOL_VOLUME_NONE && vol_intersect(S, ray, &t0, &t1) && (t1 - t0) != 0.f;
    int nSamples = hit ? (int)ceilf((t1 - t0) / S.stepSize) : 0;
    if (hit && nSamples > S.maxSteps && nLights > 1) {   // the LDS plan cannot hold this ray's lightNum: report, never guess
        if (lane == 0) {
            if (A.status) A.status[ri] = PVOL_E_LIMIT;
            else atomicAdd(&A.counters->nErrors, 1ull);
        }
        hit = false;
    }
    if (hit) {
        const float step = (t1 - t0) / nSamples;
        V3 p = ray.o + ray.d * t0, pPrev;
        const V3 w = -ray.d;
        t0 += pr.scatter_u * step;
        // LDShuffleScrambled1D(1,n,lightNum) + (1,n,lightComp) + 2D(1,n,lightPos): 4+6n draws (single.cpp:87-92).  The three delta
        // lights ignore lightComp/lightPos, and lightNum only matters with more than one light: what is never read is only counted.
        if (nLights > 1) {
            const uint32_t scramble = rng_uint<true>(rng, lane);
            for (int i = lane; i < nSamples; i += LANES) lightNum[i] = van_der_corput((uint32_t)i, scramble);
            rng_skip<true>(rng, (unsigned long long)nSamples, lane);   // n one-element shuffles (montecarlo.h:308-309)
            __syncthreads();
            for (int base = 0; base < nSamples; base += LANES) {       // Shuffle(samples, n, 1), montecarlo.h:174-181: the draws and their
                const int cnt = min(LANES, nSamples - base);            // remainders 64 at a time, the swaps serial
                const uint32_t y = rng_bulk(rng, cnt, lane);
                const int iMine = base + lane;
                const uint32_t oth = lane < cnt ? (uint32_t)iMine + (y % (uint32_t)(nSamples - iMine)) : 0u;
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)oth, j);
                    if (lane == 0) {
                        const float a = lightNum[base + j], b = lightNum[other];
                        lightNum[base + j] = b;
                        lightNum[other] = a;
                    }
                }
            }
            __syncthreads();
            rng_skip<true>(rng, 3ull + 4ull * (unsigned long long)nSamples, lane);
        } else {
            rng_skip<true>(rng, 4ull + 6ull * (unsigned long long)nSamples, lane);
        }
        for (int i = 0; i < nSamples; ++i, t0 += step) {
            ++steps;
            pPrev = p;
            p = ray.o + ray.d * t0;
            const V3 pv = xform_point(S.w2v, p);
            const bool inP = analytic && box_inside(S.extLo, S.extHi, pv);
            RayD tauRay;
            tauRay.o = pPrev; tauRay.d = p - pPrev; tauRay.mint = 0.f; tauRay.maxt = 1.f;
            const f4 stepTau = vol_tau(S, tauRay, .5f * S.stepSize, rng_float<true>(rng, lane), sigT);
            if (A.tauOut && analytic) tLen += single_tau_length(S, pPrev, tauRay.d, 0.f, 1.f);   // vol_tau's own length
            Tr = Tr * exp4(neg4(stepTau));   // accumulated, in fp32 step by step (single.cpp:101): the roulette below sees this product
            if (spec_y(Tr, Y) < 1e-3) {
                const float continueProb = .5f;
                if (rng_float<true>(rng, lane) > continueProb) {
                    Tr = mk4(0.f);
                    tScale = 0.f;
                    break;
                }
                Tr = Tr / continueProb;
                tScale *= 2.f;
            }
            const float dens = analytic ? (inP ? 1.f : 0.f) : region_density(S, pv);   // homogeneous.h:64-75 / volume.h:81-92
            const f4 ss = sigS * dens;
            Lv = Lv + Tr * (le * dens);   // single.cpp:114: not multiplied by sigma_a
            if (!spec_is_black(ss) && nLights > 0) {
                int ln = 0;
                if (nLights > 1) ln = min((int)floorf(lightNum[i] * nLights), nLights - 1);
                const DevLight &light = S.lights[ln];
                const LightSample ls = light_sample(light, p, 0.f);
                f4 L = ld4(light.intensity, q);
                if (!ls.distant) L = L * ls.fall / ls.d2;
                if (!spec_is_black(L) && !scene_occluded(S, ls.vis, lane)) {
                    // vis.Transmittance(..., NULL, rng, ...): one draw, 4 * stepSize (single.cpp:48-63)
                    const f4 Ttr = exp4(neg4(vol_tau(S, ls.vis, 4.f * S.stepSize, rng_float<true>(rng, lane), sigT)));
                    const f4 Ld = L * Ttr;
                    // vr->p(p, w, -wo): homogeneous.h:76-79 (0 outside the extent), DensityRegion::p otherwise
                    const float ph = (analytic && !inP) ? 0.f : phase_hg(w, -ls.wo, S.g);
                    Lv = Lv + Tr * ss * ph * Ld * float(nLights) / 1.f;
                }
            }
        }
        Lv = Lv * step;
    }
    *LvOut = Lv;
    *TrOut = Tr;
    *tauRec = TauRec{tLen, tScale};
}

__device__ __forceinline__ void single_write_f4(const DevScene &S, const LiArgs &A, size_t ri, f4 Lv, f4 Tr, int lane) {
    const int q = lane & 7;
    if (A.outputKind == PVOL_OUT_SPECTRAL) {
        if (lane < 8) {
            float *o = A.out + ri * 60;
            const float lv[4] = {Lv.x, Lv.y, Lv.z, Lv.w}, tr[4] = {Tr.x, Tr.y, Tr.z, Tr.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int bin = 4 * q + c;
                if (bin < 30) { o[bin] = lv[c]; o[30 + bin] = tr[c]; }
            }
        }
    } else {
        const f4 X4 = ld4(S.cieX, q), Y = ld4(S.cieY, q), Z4 = ld4(S.cieZ, q);
        const float scale = float(700 - 400) / float(106.856895f * 30);   // core/spectrum.h:427-428
        const float x = group8_sum(X4.x * Lv.x + X4.y * Lv.y + X4.z * Lv.z + X4.w * Lv.w) * scale;
        const float y = group8_sum(Y.x * Lv.x + Y.y * Lv.y + Y.z * Lv.z + Y.w * Lv.w) * scale;
        const float z = group8_sum(Z4.x * Lv.x + Z4.y * Lv.y + Z4.z * Lv.z + Z4.w * Lv.w) * scale;
        const float ty = spec_y(Tr, Y);
        if (lane == 0) *reinterpret_cast<f4 *>(A.out + ri * 4) = make_float4(x, y, z, ty);
    }
}

// LDS: MT19937 state MT_N * 4 | lightNum maxSteps * 4 (BatchPlan::ldsResolve)
__global__ __launch_bounds__(LANES, 2) void single_seq_kernel(LiArgs A) {
    extern __shared__ __align__(16) unsigned char lds[];
    const DevScene &S = *A.scene;
    const int lane = threadIdx.x;
    const uint32_t sidx = blockIdx.x;
    if (sidx >= A.nStreams) return;
    if (A.gated && *A.needSeq == 0u) return;
    uint32_t *mt = reinterpret_cast<uint32_t *>(lds);
    float *lightNum = reinterpret_cast<float *>(lds + MT_N * 4);
    const pvol_stream st = A.streams[sidx];
    Rng rng;
    rng.mt = mt;
    rng.draws = 0;
    if (A.initState) {
        const uint32_t *src = A.initState + (size_t)sidx * (MT_N + 1);
        for (int i = lane; i < MT_N; i += LANES) mt[i] = src[i];
        rng.mti = (int)src[MT_N];
        rng.draws = st.start_draw;
        __syncthreads();
    } else {
        mt_seed(mt, st.seed, lane);
        rng.mti = MT_N;
        rng_skip<true>(rng, st.start_draw, lane);
    }
    unsigned long long steps = 0;
    for (uint32_t k = 0; k < st.n_rays; ++k) {
        const size_t ri = (size_t)st.first_ray + k;
        const pvol_ray pr = A.rays[ri];
        rng_skip<true>(rng, pr.rng_skip, lane);
        const unsigned long long d0 = rng.draws;
        f4 Lv, Tr;
        TauRec tr;
        single_march_seq(S, A, pr, rng, lightNum, lane, steps, &Lv, &Tr, &tr, ri);
        single_write_f4(S, A, ri, Lv, Tr, lane);
        if (A.tauOut && lane == 0) A.tauOut[ri] = tr;
        if (A.draws && lane == 0) A.draws[ri] = (uint32_t)(rng.draws - d0);
    }
    if (lane == 0) A.streams[sidx].end_draw = rng.draws;
    if (A.finalState) {
        uint32_t *dst = A.finalState + (size_t)sidx * (MT_N + 1);
        __syncthreads();
        for (int i = lane; i < MT_N; i += LANES) dst[i] = mt[i];
        if (lane == 0) dst[MT_N] = (uint32_t)rng.mti;
    }
    if (lane == 0) {
        if (st.n_rays) atomicAdd(&A.counters->nRays, (unsigned long long)st.n_rays);
        if (steps) atomicAdd(&A.counters->nSteps, steps);
    }
}

// ------------------------------------------------------------------------------------------ ray-parallel form
// inclusive sum over the wave's lanes with DPP adds (no LDS round trips): row_shr 1, 2, 4, 8 scan each row of 16 lanes,
// row_bcast15 / row_bcast31 carry the row totals across the rows
__device__ __forceinline__ float single_scan(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false));
    return v;
}

// The roulette's test value with a margin.  The sequential form multiplies Tr step by step in fp32, this form takes
// exp(-sigma_t * prefix length): after i steps the two differ by at most ~4e-7 i relative (per step one rounded product, 6e-8, and one
// fast exponential, ~2 ulp, against the scan's own sum, ~6e-8 log2(64) per trip).  A ray whose Tr.y() at step i is within
// 0.1 % + 4e-7 i above the threshold is handed to the sequential form, which decides on the reference's own product: the guard grows
// with the step count, so a march of 10^4 steps (the plan's limit is 12 000) is covered as one of 100 is.
__device__ __forceinline__ float single_roulette_guard(int stepsDone) { return 1e-3f * (1.001f + 4e-7f * (float)stepsDone); }

// LDS: one float4 per spectral bin {sigma_t, Le, sigma_s * I of the one light, CIE Y}, 480 bytes, read as wave-wide broadcasts (every
// lane the same address).  As scalar loads the 120 values did not fit the scalar registers (101 of them spilled).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): at 3 waves per SIMD 168 VGPRs with 62 spilled and 36 spilled SGPRs
// (li_par_kernel: 168, 150 and 93); at 2 waves 233 VGPRs and no VGPR spill (measured slower); at 4 waves 128 with 110 spilled.
__global__ __launch_bounds__(LANES, 3) void single_par_kernel(LiArgs A) {
    __shared__ f4 bins[PVOL_NBINS];
    const DevScene &S = *A.scene;
    const int lane = threadIdx.x;
    const int nLights = S.nLights;
    if (lane < PVOL_NBINS)
        bins[lane] = make_float4(S.sigA[lane] + S.sigS[lane], S.le[lane], nLights > 0 ? S.sigS[lane] * S.lights[0].intensity[lane] : 0.f, S.cieY[lane]);
    __syncthreads();
    // wave-uniform facts of the medium and its one light
    const int binL = min(lane, PVOL_NBINS - 1);
    const float sigTmax = wave_max(bins[binL].x);
    const bool blackS = !wave_any(S.sigS[binL] != 0.f), blackLe = !wave_any(bins[binL].y != 0.f);
    const bool blackI = nLights > 0 ? !wave_any(S.lights[0].intensity[binL] != 0.f) : true;
    const bool medium = S.volKind != PVOL_VOLUME_NONE;
    unsigned long long nRaysDone = 0, nStepsDone = 0;
    for (;;) {
        uint32_t chunk = 0;
        if (lane == 0) chunk = atomicAdd(A.chunkCounter, 1u);
        chunk = (uint32_t)lane_i((int)chunk, 0);
        const unsigned long long r0 = (unsigned long long)chunk * SINGLE_CHUNK_RAYS;
        if (r0 >= A.nRays) break;
        const uint32_t r1 = (uint32_t)min((unsigned long long)A.nRays, r0 + SINGLE_CHUNK_RAYS);
        uint32_t sidx = single_stream_of(A.streams, A.nStreams, (uint32_t)r0);
        uint32_t sEnd = A.streams[sidx].first_ray + A.streams[sidx].n_rays;
        unsigned long long acc = 0;   // draws of the current stream seen by this wave
        for (uint32_t ri = (uint32_t)r0; ri < r1; ++ri) {
            while (ri >= sEnd && sidx + 1 < A.nStreams) {   // chunk crosses into the next stream
                if (lane == 0 && acc) atomicAdd((unsigned long long *)&A.streams[sidx].end_draw, acc);
                acc = 0;
                ++sidx;
                sEnd = A.streams[sidx].first_ray + A.streams[sidx].n_rays;
            }
            const pvol_ray pr = A.rays[ri];
            RayD ray;
            ray.o = v3(pr.o[0], pr.o[1], pr.o[2]);
            ray.d = v3(pr.d[0], pr.d[1], pr.d[2]);
            ray.mint = pr.mint;
            ray.maxt = pr.maxt;
            float t0, t1;
            const bool hit = medium && vol_intersect(S, ray, &t0, &t1) && (t1 - t0) != 0.f;
            const int nSamples = hit ? (int)ceilf((t1 - t0) / S.stepSize) : 0;
            ++nRaysDone;
            float lvMine = 0.f;       // lane b < 30: bin b of Lv / step, summed over the trips
            float lenTotal = 0.f;     // tau() length of the steps so far (wave-uniform)
            unsigned long long draws = 0;
            bool redo = false;
            if (hit) {
                const float step = (t1 - t0) / nSamples;
                const V3 pEntry = ray.o + ray.d * t0;
                const V3 w = -ray.d;
                float tcur = t0 + pr.scatter_u * step;
                draws = 4ull + 6ull * (unsigned long long)nSamples;
                V3 pCarry = pEntry;   // p of the step before the trip
                bool inCarry = box_inside(S.extLo, S.extHi, xform_point(S.w2v, pEntry));
                for (int base = 0; base < nSamples && !redo; base += LANES) {
                    const int cnt = min(LANES, nSamples - base);
                    // t0 is ACCUMULATED in the reference (`t0 += step` per iteration): replay the same additions
                    float tMine = 0.f;
                    for (int j = 0; j < cnt; ++j) {
                        if (lane == j) tMine = tcur;
                        tcur += step;
                    }
                    const bool on = lane < cnt;
                    const V3 p = ray.o + ray.d * tMine;
                    const V3 pv = xform_point(S.w2v, p);
                    const bool inP = on && box_inside(S.extLo, S.extHi, pv);
                    // pPrev / inPrev of lane j = p / inP of lane j - 1 (the carry for lane 0)
                    V3 pPrev;
                    pPrev.x = __shfl_up(p.x, 1); pPrev.y = __shfl_up(p.y, 1); pPrev.z = __shfl_up(p.z, 1);
                    int inPrevI = __shfl_up(inP ? 1 : 0, 1);
                    if (lane == 0) { pPrev = pCarry; inPrevI = inCarry ? 1 : 0; }
                    float lenStep = 0.f;
                    if (on) {
                        const V3 dseg = p - pPrev;
                        // both ends inside: the slab clip of the [0,1] segment is taken as the identity.  For a point ON the extent's
                        // boundary the reference's fp32 clip can return t1 = 1 - ulp: the length (and tauOut, which feeds the surface
                        // composition) is then the reference's within an ulp, not bit for bit -- inside the 1e-4 bar, as in li_par_kernel
                        if (inPrevI && inP) {
                            const V3 a = pPrev + dseg * 0.f, b = pPrev + dseg * 1.f;
                            lenStep = len(a - b);
                        } else {
                            lenStep = single_tau_length(S, pPrev, dseg, 0.f, 1.f);
                        }
                    }
                    pCarry.x = lane_f(p.x, cnt - 1); pCarry.y = lane_f(p.y, cnt - 1); pCarry.z = lane_f(p.z, cnt - 1);
                    inCarry = lane_i(inP ? 1 : 0, cnt - 1) != 0;
                    // accumulated transmittance of step i: exp(-sigma_t * (length of steps 0..i))
                    const float prefix = lenTotal + single_scan(lenStep);
                    lenTotal = lane_f(prefix, LANES - 1);
                    // Tr.y() >= Y(1) exp(-prefix sigTmax): no roulette while prefix sigTmax < 6.8 (the bound of roulette_possible)
                    bool near = false;
                    if (on && !(prefix * sigTmax < 6.8f)) {
                        float yv = 0.f;
                        for (int b = 0; b < PVOL_NBINS; ++b) yv += bins[b].w * __expf(-bins[b].x * prefix);
                        near = yv * 300.f / (106.856895f * 30) < single_roulette_guard(base + lane + 1);
                    }
                    if (wave_any(near)) { redo = true; break; }
                    // this lane's light sample: Sample_L, the black test, the shadow ray, its way out of the extent
                    bool lit = false;
                    float exitLen = 0.f, gain = 0.f;   // gain: p(p, w, -wo) * fall / d2 * nLights
                    if (inP && !blackS && nLights > 0) {   // sigma_s is black outside the extent
                        const LightSample ls = light_sample(S.lights[0], p, 0.f);
                        if (!(ls.fall == 0.f || blackI) && !lane_occluded(S, ls.vis)) {
                            lit = true;
                            const V3 dv = xform_vector(S.w2v, ls.vis.d);
                            exitLen = single_exit_length(S, ls.vis.o, ls.vis.d, pv, v3(1.f / dv.x, 1.f / dv.y, 1.f / dv.z), ls.vis.maxt);
                            gain = phase_hg(w, -ls.wo, S.g) * (ls.distant ? 1.f : ls.fall / ls.d2) * float(nLights);
                        }
                    }
                    draws += (unsigned long long)cnt + (unsigned long long)__popcll(__ballot(lit));
                    nStepsDone += (unsigned long long)cnt;
                    // Every lane's step adds to all 30 bins.  Thirty partial sums per lane across the trips, reduced once per ray, cost
                    // 200 spilled VGPRs at three waves per SIMD (the unrolled loop also hoists the 120 table values); one wave sum per
                    // bin and trip instead is ~12 instructions a bin for 64 steps and keeps the loop rolled.
                    if (wave_any(inP && (lit || !blackLe))) {
#pragma nounroll
                        for (int b = 0; b < PVOL_NBINS; ++b) {
                            const f4 c = bins[b];
                            float v = 0.f;
                            if (inP && !blackLe) v = __expf(-c.x * prefix) * c.y;
                            // Tr * sigma_s * p * (L * exp(-tau(shadow ray))) * nLights: the two exponentials as one
                            if (lit) v += __expf(-c.x * (prefix + exitLen)) * (c.z * gain);
                            const float s = wave_sum(v);
                            if (lane == b) lvMine += s;
                        }
                    }
                }
                lvMine *= step;   // single.cpp:138
            }
            if (redo) {   // the roulette compares a drawn value: the batch is redone sequentially
                if (lane == 0) atomicOr(A.needSeq, 1u);
                continue;
            }
            // bin `lane` of Lv (above) and of T = exp(-sigma_t * length) in lanes 0..29
            const int bin = binL;
            const float trMine = __expf(-bins[bin].x * lenTotal);
            if (A.outputKind == PVOL_OUT_SPECTRAL) {
                if (lane < PVOL_NBINS) { A.out[(size_t)ri * 60 + lane] = lvMine; A.out[(size_t)ri * 60 + 30 + lane] = trMine; }
            } else {
                const bool bOn = lane < PVOL_NBINS;
                const float scale = float(700 - 400) / float(106.856895f * 30);   // core/spectrum.h:427-428
                const float x = wave_sum(bOn ? S.cieX[bin] * lvMine : 0.f) * scale, y = wave_sum(bOn ? S.cieY[bin] * lvMine : 0.f) * scale;
                const float z = wave_sum(bOn ? S.cieZ[bin] * lvMine : 0.f) * scale, ty = wave_sum(bOn ? S.cieY[bin] * trMine : 0.f) * scale;
                if (lane == 0) *reinterpret_cast<f4 *>(A.out + (size_t)ri * 4) = make_float4(x, y, z, ty);
            }
            if (A.tauOut && lane == 0) A.tauOut[ri] = TauRec{lenTotal, 1.f};
            if (A.draws && lane == 0) A.draws[ri] = (uint32_t)draws;
            acc += draws + pr.rng_skip;
        }
        if (lane == 0 && acc) atomicAdd((unsigned long long *)&A.streams[sidx].end_draw, acc);
    }
    if (lane == 0) {
        if (nRaysDone) atomicAdd(&A.counters->nRays, nRaysDone);
        if (nStepsDone) atomicAdd(&A.counters->nSteps, nStepsDone);
    }
}

extern "C" hipError_t pvol_launch_single_seq(const LiArgs *args, size_t ldsBytes, hipStream_t stream) {
    hipLaunchKernelGGL(single_seq_kernel, dim3(args->nStreams), dim3(LANES), ldsBytes, stream, *args);
    return hipGetLastError();
}

// the caller has zeroed chunkCounter and needSeq (LiArgs)
extern "C" hipError_t pvol_launch_single_par(const LiArgs *args, uint32_t nWaves, hipStream_t stream) {
    hipLaunchKernelGGL(single_stream_begin_kernel, dim3((args->nStreams + 255) / 256), dim3(256), 0, stream, args->streams, args->nStreams);
    hipLaunchKernelGGL(single_par_kernel, dim3(nWaves), dim3(LANES), 0, stream, *args);
    return hipGetLastError();
}
