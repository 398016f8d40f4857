// pvol_rays_dev.h -- included by pvol_march.hip after pvol_tile_dev.h (first compilation only: nothing here reads a density).
//
// The pre-pass and the fold of pvol_radiance_batch* (DESIGN.md 22): SamplerRenderer::Li (renderers/samplerrenderer.cpp:228-251,
// :95-97) for rays the CALLER generated.  What the tile kernel does for its camera rays -- Scene::Intersect clips the ray, the
// surface integrator's draws are counted in front of the ray's volume Li(), the spawned rays of a glass hit are laid out in the
// stream's order (pvol_spec_dev.h) -- is done here for one caller ray per lane, and the result is an ordinary ray batch:
//
//   expanded array, per caller ray i the block [offset[i], offset[i + 1]):   seg 0, seg 1, ..., seg nSeg-1, primary
//
// in post-order, i.e. in the order the reference's one RNG stream meets them.  Every member is a pvol_ray with rng_skip = the draws
// made since the previous member's volume Li() (the block's first member also carries the caller's own rng_skip: its sampler drew
// before Li() was called, samplerrenderer.cpp:83-97), so the march kernels walk the block like any other rays of the stream and nobody
// counts a segment's volume draws ahead of time.  Two passes over spec_surface<0> with a scan between them: the sizes are known
// before anything is written, so there is no pool, no atomic and nothing that can overflow.
//
// After the volume batch (60-float rows) and surface_kernel in its spectral mode, rays_compose_kernel folds every block as
// spec_compose_kernel folds a camera sample's segments, with the primary as the depth-0 node:
//     value(seg) = Lv(seg) + T(seg) (.) sum over its children ((Fs K) / awz) g value(child)      (rows already hold T (.) Ls_matte in Lv)
//     L = Lv(primary) + T(primary) (.) [ Ls_matte(primary hit) + sum over the primary hit's lobes ... ]
// The primary's own row is moved to a stash before surface_kernel runs and replaced by Lv = 0, T = 1, so that the kernel leaves
// Ls_matte itself there: the surface term is reported BEFORE its multiplication by T, and a T of zero (a roulette kill) loses nothing.
#ifndef PVOL_RAYS_DEV_H
#define PVOL_RAYS_DEV_H

// Scene::Intersect over [mint, maxt] (samplerrenderer.cpp:236): surf_closest knows no upper bound, the caller's maxt is applied here
__device__ __forceinline__ bool rays_clip(const DevScene &S, const pvol_ray &r, V3 *o, V3 *d, Hit *h) {
    *o = v3(r.o[0], r.o[1], r.o[2]); *d = v3(r.d[0], r.d[1], r.d[2]);
    h->tri = 0; h->mat = 0; h->t = 0.f; h->rayEps = 0.f; h->p = h->nn = h->dpdu = v3(0.f, 0.f, 0.f);
    return surf_closest(S, *o, *d, r.mint, h) && h->t <= r.maxt;
}

// SpecEmitPol for a block whose end is known: a segment beyond it (the two passes disagreeing) is dropped, never written
struct RaysEmitPol {
    pvol_ray *rays; SegInfo *info; uint32_t base, end, sample, own; float su, time;
    __device__ void visit(SpecCtx &X, int D, int lobe, int mat, float Fs, float awz, float g, V3 o, V3 d, float mint, float maxt) {
        const uint32_t idx = base + X.nSeg;
        if (idx < end) {
            pvol_ray r;
            r.o[0] = o.x; r.o[1] = o.y; r.o[2] = o.z; r.mint = mint;
            r.d[0] = d.x; r.d[1] = d.y; r.d[2] = d.z; r.maxt = maxt;
            // the caller's own draws (its sampler's) come before Li() is called at all: they are skipped in front of the block's first member
            r.time = time; r.scatter_u = su; r.rng_skip = X.pending + (X.nSeg == 0u ? own : 0u); r.flags = 0u;
            rays[idx] = r;
            SegInfo si;
            si.sample = sample; si.depthLobeMat = (uint32_t)D | ((uint32_t)lobe << 8) | ((uint32_t)mat << 16);
            si.Fs = Fs; si.awz = awz; si.g = g; si.pad[0] = si.pad[1] = si.pad[2] = 0u;
            info[idx] = si;
        }
        X.pending = 0u;
    }
};

// count[i] = members of caller ray i's block (its segments + itself); count[n] = 0, so that the scan's entry n is the total
__global__ __launch_bounds__(LANES) void rays_count_kernel(RaysArgs A) {
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (i > A.n) return;
    uint32_t cnt = i < A.n ? 1u : 0u;
    if (i < A.n && A.specOn) {   // only a glass hit spawns anything: a matte hit's draws are the emit pass's business
        const DevScene &S = *A.scene;
        V3 o, d;
        Hit h;
        if (rays_clip(S, A.in[i], &o, &d, &h) && S.shootScene->mats[h.mat].kind != PVOL_MATERIAL_MATTE) {
            SpecCtx X;
            X.blackMask = 0u; X.pending = 0u; X.nSeg = 0u;
            SpecNullPol np;
            spec_surface<0>(S, X, np, d, h);
            cnt += X.nSeg;
        }
    }
    A.count[i] = cnt;
}

__global__ __launch_bounds__(LANES) void rays_emit_kernel(RaysArgs A) {
    const DevScene &S = *A.scene;
    const int lane = threadIdx.x;
    unsigned blackMask = 0u;   // all 64 lanes are still here: the test is a wave's (eight lanes hold a spectrum)
    { const int q = lane & 7; for (int l = 0; l < S.nLights; ++l) if (spec_is_black(ld4(S.lights[l].intensity, q))) blackMask |= 1u << l; }
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t base = A.offset[i], e = A.offset[i + 1] - 1u;
    pvol_ray r = A.in[i];
    V3 o, d;
    Hit h;
    const bool hit = rays_clip(S, r, &o, &d, &h);
    uint32_t pending = 0u;
    if (hit) {
        r.maxt = h.t;
        if (A.surfOn) {   // PhotonIntegrator::Li at the hit: its draws, and the rays it spawns in front of this ray's volume Li()
            SpecCtx X;
            X.blackMask = blackMask; X.pending = 0u; X.nSeg = 0u;
            RaysEmitPol ep;
            ep.rays = A.rays; ep.info = A.info; ep.base = base; ep.end = e; ep.sample = i; ep.own = r.rng_skip; ep.su = r.scatter_u; ep.time = r.time;
            spec_surface<0>(S, X, ep, d, h);
            pending = X.pending;
        }
    }
    r.rng_skip = pending + (e > base ? 0u : r.rng_skip); r.flags = 0u;   // a block of its own: the caller's draws, then the surface integrator's
    A.rays[e] = r;
    SegInfo si;
    si.sample = i; si.depthLobeMat = 0u; si.Fs = r.maxt; si.awz = 1.f; si.g = 0.f;   // the primary: Fs carries maxt after the clip
    si.pad[0] = hit ? 1u : 0u; si.pad[1] = si.pad[2] = 0u;
    A.info[e] = si;
}

// the slice's stream table, uploaded with first_ray / n_rays in caller rays, onto the expanded array; a stream that an earlier
// slice began goes on from the end_draw that slice left in the caller's table
__global__ void rays_streams_kernel(pvol_stream *st, uint32_t nStreams, const uint32_t *offset, const pvol_stream *continued) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nStreams) return;
    pvol_stream s = st[j];
    const uint32_t a = offset[s.first_ray], b = offset[s.first_ray + s.n_rays];
    s.first_ray = a; s.n_rays = b - a;
    if (j == 0u && continued) s.start_draw = continued->end_draw;
    st[j] = s;
}
__global__ void rays_end_kernel(const pvol_stream *st, uint32_t nStreams, pvol_stream *caller) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < nStreams) caller[j].end_draw = st[j].end_draw;
}

// Between the volume batch and surface_kernel, 64 threads per caller ray: a primary with a hit hands its row (Lv, T) to the stash
// and becomes (0, 1); one without becomes the ray that meets nothing (spec_fill_kernel's), since surface_kernel repeats surf_closest
// without an upper bound.  Its rng_skip stays: the fold reads it.
__global__ __launch_bounds__(256) void rays_patch_kernel(RaysArgs A) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), k = threadIdx.x & 63u;
    if (i >= A.n) return;
    const uint32_t e = A.offset[i + 1] - 1u;
    if (A.info[e].pad[0]) {
        if (k < 60u) {
            float *row = A.rows + (size_t)e * 60;
            A.stash[(size_t)i * 60 + k] = row[k];
            row[k] = k < 30u ? 0.f : 1.f;
        }
    } else if (k == 0u) {
        A.rays[e].mint = 1.f; A.rays[e].maxt = 0.f;
    }
}

// One caller ray per lane, bin by bin: spec_compose_kernel's post-order fold over the block, the primary as its depth-0 node
__global__ __launch_bounds__(256) void rays_compose_kernel(RaysArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const DevScene &S = *A.scene;
    const uint32_t base = A.offset[i], e = A.offset[i + 1] - 1u, n = e - base;
    const SegInfo pi = A.info[e];
    const bool stashed = A.surfOn && pi.pad[0];
    const float *prow = stashed ? A.stash + (size_t)i * 60 : A.rows + (size_t)e * 60;   // the primary's Lv, T
    const float *lsrow = A.rows + (size_t)e * 60;                                       // stashed: Ls_matte of the primary's hit
    float x = 0.f, y = 0.f, z = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, ty = 0.f;
    for (int b = 0; b < 30; ++b) {
        float acc[SPEC_MAX_DEPTH + 1];   // acc[D]: what the children of the pending depth-(D-1) ray have brought in so far
#pragma unroll
        for (int dd = 0; dd <= SPEC_MAX_DEPTH; ++dd) acc[dd] = 0.f;
        for (uint32_t s = 0; s < n; ++s) {   // post-order: a ray's children come before it
            const SegInfo si = A.info[base + s];
            const int D = (int)(si.depthLobeMat & 0xffu), lobe = (int)((si.depthLobeMat >> 8) & 0xffu), mat = (int)(si.depthLobeMat >> 16);
            const float *o = A.rows + (size_t)(base + s) * 60;
            float below = 0.f;
#pragma unroll
            for (int dd = 1; dd <= SPEC_MAX_DEPTH; ++dd) if (dd == D + 1) { below = acc[dd]; acc[dd] = 0.f; }
            const float val = o[b] + o[30 + b] * below;
            const DevMaterial &m = S.shootScene->mats[mat];
            const float K = lobe == 1 ? m.kr[b] : m.kt[b];
            const float add = ((si.Fs * K) / si.awz) * val * si.g;   // f * Li * (AbsDot(wi, n) / pdf), integrator.cpp:196,240
#pragma unroll
            for (int dd = 1; dd <= SPEC_MAX_DEPTH; ++dd) if (dd == D) acc[dd] += add;
        }
        const float Ls = acc[1] + (stashed ? lsrow[b] : 0.f);
        const float Tb = prow[30 + b];
        const float Lb = prow[b] + Tb * Ls;   // T * Ls + Lvi, samplerrenderer.cpp:95-97
        if (A.spectral) { A.L[(size_t)i * 60 + b] = Lb; A.L[(size_t)i * 60 + 30 + b] = Tb; }
        x += S.cieX[b] * Lb; y += S.cieY[b] * Lb; z += S.cieZ[b] * Lb;
        sx += S.cieX[b] * Ls; sy += S.cieY[b] * Ls; sz += S.cieZ[b] * Ls;
        ty += S.cieY[b] * Tb;
    }
    const float scale = float(700 - 400) / float(106.856895f * 30);
    if (!A.spectral) { float *op = A.L + (size_t)i * 4; op[0] = x * scale; op[1] = y * scale; op[2] = z * scale; op[3] = ty * 300.f / (106.856895f * 30); }
    if (A.surfXyz) { A.surfXyz[3 * (size_t)i] = sx * scale; A.surfXyz[3 * (size_t)i + 1] = sy * scale; A.surfXyz[3 * (size_t)i + 2] = sz * scale; }
    if (A.tHit) A.tHit[i] = pi.Fs;
    if (A.outDraws) A.outDraws[i] = A.draws[e];
    if (A.surfDraws) {   // everything the stream saw for this ray in front of its own volume Li(), the caller's rng_skip excluded
        uint32_t sd = A.rays[e].rng_skip;
        for (uint32_t s = 0; s < n; ++s) sd += A.rays[base + s].rng_skip + A.draws[base + s];
        A.surfDraws[i] = sd - A.in[i].rng_skip;   // the caller's draws sit in the block's first member
    }
    if (A.nSegments) A.nSegments[i] = n;
}

extern "C" hipError_t pvol_launch_rays_count(const RaysArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(rays_count_kernel, dim3(a->n / LANES + 1u), dim3(LANES), 0, stream, *a);   // n + 1 entries
    return hipGetLastError();
}
extern "C" hipError_t pvol_launch_rays_emit(const RaysArgs *a, pvol_stream *st, uint32_t nStreams, const pvol_stream *continued, hipStream_t stream) {
    hipLaunchKernelGGL(rays_emit_kernel, dim3((a->n + LANES - 1) / LANES), dim3(LANES), 0, stream, *a);
    hipLaunchKernelGGL(rays_streams_kernel, dim3((nStreams + 255u) / 256u), dim3(256), 0, stream, st, nStreams, a->offset, continued);
    return hipGetLastError();
}
extern "C" hipError_t pvol_launch_rays_patch(const RaysArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(rays_patch_kernel, dim3((a->n + 3u) / 4u), dim3(256), 0, stream, *a);
    return hipGetLastError();
}
extern "C" hipError_t pvol_launch_rays_compose(const RaysArgs *a, const pvol_stream *st, uint32_t nStreams, pvol_stream *caller, hipStream_t stream) {
    hipLaunchKernelGGL(rays_compose_kernel, dim3((a->n + 255u) / 256u), dim3(256), 0, stream, *a);
    hipLaunchKernelGGL(rays_end_kernel, dim3((nStreams + 255u) / 256u), dim3(256), 0, stream, st, nStreams, caller);
    return hipGetLastError();
}
#endif
