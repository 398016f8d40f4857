// pvol_api.hip -- the C ABI of include/pvol.h: context lifetime, the plan of a batch, kernel launches, the host batches and the
// statistics (the scene is in pvol_scene_host.hip, the photon maps in pvol_map_host.hip).  There is NO CPU fallback: every entry
// point that needs the GPU returns PVOL_E_NO_DEVICE when HIP is unusable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "pvol_dev.h"

#include "pvol_host.h"

const char *pvol_env_get(const char *name) { return getenv(name); }   // what every read point of pvol_env.h is given

extern "C" {

int pvol_abi_version(void) { return PVOL_ABI_VERSION; }

const char *pvol_strerror(int s) {
    switch (s) {
    case PVOL_OK: return "ok";
    case PVOL_E_INVALID: return "invalid argument";
    case PVOL_E_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
    case PVOL_E_NO_SCENE: return "no scene set";
    case PVOL_E_NO_MEMORY: return "out of memory";
    case PVOL_E_UNSUPPORTED: return "unsupported volume/light/material kind or size";
    case PVOL_E_LIMIT: return "a ray needs more march steps than the kernel's LDS plan";
    case PVOL_E_SHOOT_FAILED: return "unable to store enough photons";
    default: return "unknown status";
    }
}

int pvol_device_count(void) {
    int n = 0;
    if (!ok(hipGetDeviceCount(&n))) return 0;
    return n;
}

void pvol_default_params(pvol_params *p) {
    memset(p, 0, sizeof(*p));
    p->step_size = 1.f;          // photonvolume.cpp:225
    p->n_used = 250;             // photonvolume.cpp:226
    p->max_dist = 0.1f;          // photonvolume.cpp:227
    p->n_volume_photons = 0;     // photonshooter.cpp:532
    p->shooter_step_size = 0.1f; // photonshooter.cpp:533
    p->max_photon_depth = 5;     // photonshooter.cpp:539
    p->n_caustic_photons = 20000;
    p->n_indirect_photons = 10000;
    p->final_gather = 1;
    p->device = 0;
    p->grid_cell_scale = 0.f;
    p->keep_surface_photons = 0;
}

int pvol_create(const pvol_params *params, pvol_ctx **out) {
    if (!params || !out) return PVOL_E_INVALID;
    *out = 0;
    if (params->n_used < 1 || !(params->step_size > 0.f) || !(params->max_dist > 0.f)) return PVOL_E_INVALID;
    if (params->n_used > 576) return PVOL_E_UNSUPPORTED;   // select_k holds the candidate list in 12 registers per lane
    int n = 0;
    if (!ok(hipGetDeviceCount(&n)) || n <= 0 || params->device < 0 || params->device >= n) return PVOL_E_NO_DEVICE;
    if (!ok(hipSetDevice(params->device))) return PVOL_E_NO_DEVICE;
    pvol_ctx *c = new (std::nothrow) pvol_ctx();
    if (!c) return PVOL_E_NO_MEMORY;
    c->params = *params;
    c->knobs = pvol_env_context(pvol_env_get);
    c->co.maxBatch = pvol_env_li_coalesce(pvol_env_get);
    { hipDeviceProp_t prop; if (ok(hipGetDeviceProperties(&prop, params->device))) c->nCU = prop.multiProcessorCount; }
    if (!c->ds.alloc(1) || !c->dCounters.alloc(1) || !c->dWords.alloc(4) || !c->dsh.alloc(1) ||
        !ok(hipMemset(c->dCounters.get(), 0, sizeof(DevCounters)))) {
        delete c;
        return PVOL_E_NO_DEVICE;
    }
    *out = c;
    return PVOL_OK;
}

// Every allocation, event and stream of the context is held by an owner (pvol_host.h): deleting the context frees them.  The order
// of the members does not matter: after the device-wide synchronise nothing of the context is in flight.
void pvol_destroy(pvol_ctx *c) {
    if (!c) return;
    hipSetDevice(c->params.device);
    hipDeviceSynchronize();
    delete c;
}

int pvol_get_accel_info(pvol_ctx *c, double *out2) {
    if (!c || !out2) return PVOL_E_INVALID;
    out2[0] = (double)c->hs.nBvhTris; out2[1] = c->bvhBuildMs;
    return PVOL_OK;
}

int pvol_push_scene(pvol_ctx *c) {
    return ok(hipMemcpy(c->ds.get(), &c->hs, sizeof(DevScene), hipMemcpyHostToDevice)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

// ---- the plan of a batch (pvol_host.h): no HIP call, no context, no environment up to pvol_plan_batch
// bytes of one record slot: header, one byte per march step, and for a VolumeGrid the drawn offsets of every step
size_t pvol_rec_stride(int maxSteps, bool grid) {
    const size_t stride = 16 + (size_t)((maxSteps + 15) & ~15) + (grid ? 8 * (size_t)maxSteps : 0);
    return (stride + 15) & ~(size_t)15;
}

BatchPlan plan_path(const PlanIn &in) {
    BatchPlan p = {};
    const bool tile = in.hasTile, grid = is_density_region(in.volKind), homog = in.volKind == PVOL_VOLUME_HOMOGENEOUS;   // grid: a DensityRegion
    // Drawn VALUES cannot reach Li()'s result with at most one light and an analytic tau(): such scenes take the
    // ray-parallel kernel, backed by the sequential one if a ray reaches the roulette.
    const bool parOk = in.nLights <= 1 && !grid && !in.hasInit;
    // the tile pre-pass can COUNT Li()'s draws (instead of drawing them) under the same conditions, provided no march step can
    // reach the roulette
    const bool tileCount = tile && parOk && !in.roulette;
    // a VolumeGrid with at most one light: the draw COUNT is still geometry only (4 + 6n + n + u; the drawn offsets change values,
    // not counts), so the tile pre-pass counts and the values come from the RNG-only resolve pass of each slice
    const bool tileGridCount = tile && in.nLights <= 1 && grid && !in.hasInit && !in.roulette && !in.forceSeq && !in.noLite;
    const bool par = parOk && !in.forceSeq && (!tile || tileCount);
    // scenes where drawn values matter: sequential RESOLVE pre-pass + ray-parallel REPLAY, slice by slice
    const bool sliced = !par && !in.forceSeq && !in.transOnly && (in.volKind != PVOL_VOLUME_NONE || tile);
    p.kernel = "li_seq_kernel";
    p.path = par ? PVOL_PATH_PAR : sliced ? PVOL_PATH_SLICED : PVOL_PATH_SEQ;
    p.tile = !tile ? PVOL_TILE_NONE : !sliced ? PVOL_TILE_COUNT : tileGridCount ? PVOL_TILE_GRID_COUNT : PVOL_TILE_FUSED;
    if (p.tile == PVOL_TILE_COUNT && !tileCount) p.rc = PVOL_E_UNSUPPORTED;
    // *T of a VolumeGrid is a product of stepped taus with drawn offsets: not a TauRec (the surface term is refused there)
    if (in.hasTauOut && grid) p.rc = PVOL_E_UNSUPPORTED;
    // li_group_kernel (one ray per lane, gathers of 64 rays share a photon bucket): an isotropic medium with a photon map
    const bool bucket = !in.noGroup && in.g == 0.f && in.nPhotons > 0 && in.nUsed >= 10;
    if (par) {   // homogeneous and k <= 64; li_par_kernel (one wave per ray) otherwise
        p.groupForm = bucket && homog && in.nUsed <= 64 && in.candCap <= 4 * 64;
        // an XYZ result of a nearly grey medium: the flux is summed as moments.  The stats launch keeps the 30 bins
        // (a -DGRP_PHASE_DIAG build, timing only, times the form the plain launch takes)
#ifdef GRP_PHASE_DIAG
        const bool momStats = true;
#else
        const bool momStats = !in.statsOn;
#endif
        if (p.groupForm && in.momentTerms > 0 && in.outXYZ && !in.noMoments && momStats) p.groupForm = GRP_FORM_MOMENTS;
        p.kernel = p.groupForm ? "li_group_kernel" : "li_par_kernel";
    } else if (sliced) {
        // with a tile pre-pass in FUSED mode (several lights) the flag selects the pre-pass's own geometry + RNG-only form
        p.liteResolve = !in.noLite && !in.roulette;
        p.resolve = p.tile == PVOL_TILE_NONE || p.tile == PVOL_TILE_GRID_COUNT;
        // the replay form where no march step can reach the roulette; li_replay_kernel (one wave per ray) otherwise, and as the gated backup
        if (bucket && !in.statsOn && !in.roulette && (homog || grid)) p.groupForm = grid ? 2 : 1;
        p.fixGroup = p.groupForm && in.nUsed > 100 && !in.knobs.fixExact;   // GRP_PLAN_KMAX: see pvol_fixgrp_dev.h
        p.kernel = p.groupForm ? "li_group_kernel" : "li_replay_kernel";
        // the FUSED pre-pass walks the segments of the specular recursion (geo_ray + lite_ray)
        if (in.specOn && !(p.tile == PVOL_TILE_FUSED && p.liteResolve)) p.rc = PVOL_E_UNSUPPORTED;
    }
    return p;
}

// The form of the COUNT-mode tile pre-pass (pvol_host.h): PLAIN where every run-time test of the general kernels is decided by the scene.
// No light at all keeps the general form (its early return needs no rows); a black light is still a distant light and takes PLAIN.
int pvol_tile_plain_gate(const TilePlainIn *in) {
    const bool extent = in->volKind == PVOL_VOLUME_HOMOGENEOUS || in->volKind == PVOL_VOLUME_RAINBOW;   // Inside() of a box: no density region, no "none"
    return in->tile == PVOL_TILE_COUNT && !in->tileGeneral && extent && in->nLights > 0 &&
           in->light0Kind == PVOL_LIGHT_DISTANT && !in->hasBvh && in->nSpheres == 0 && in->nTris >= 0 && in->nTris <= PVOL_MAX_TRIS &&
           !in->surfOn && !in->specLink;
}

// Waves per render task of the COUNT-mode tile pre-pass.  A task is a serial chain (one MT19937 stream); with many tasks per CU
// the chip is kept busy by running them side by side (one wave each), with few -- one rank's share of a multi-GPU frame -- the
// draw count of every pixel is spread over several waves instead (tile_mw_kernel).  PVOL_TILE_WAVES overrides.
static int tile_waves_per_task(const PlanIn &in) {
    if (in.tileWaves > 0) return in.tileWaves;
    // measured on the C2 frame (tools/cmp_mt.sh, profiles/r03_tile_waves.txt): 16 tasks per CU 231 ms with one wave against 345 with two, 8 per CU
    // 210 with one, 210 with two, 270 with eight; 4 per CU 198 with one, 132 with two, 144 with eight; 2 per CU 194 against 86 with eight
    const double perCU = (double)in.nStreams / (double)std::max(1, in.nCU);
    // (second pass, with the multi-wave kernels held to two waves per SIMD -- 256 VGPRs, so that the workgroups of ALL a CU's tasks are resident:
    // 4 per CU 77 ms with two waves (134 before), 99 with four; 2 per CU 56.5 ms with four waves, 80.8 with eight at 128 VGPRs, 85.9 at 256)
    // 8 per CU: 131.5 ms with two waves, 146.9 with one; 16 per CU: 174.7 with one, 190.7 with two
    return perCU >= 12.0 ? 1 : (perCU >= 3.0 ? 2 : 4);
}
// The same for the PLAIN form (pvol_tile_plain_gate), whose two- and four-wave kernels take 152 VGPRs and spill nothing: three waves per SIMD
// instead of two, so six two-wave tasks of a CU are resident instead of four.  Measured on the C2 frame (bench.py --emulate-ranks 2,4,8 by
// PVOL_TILE_WAVES, profiles/tile_plain_emulate.txt), tile pre-pass in ms with one / two / four waves: 16 tasks per CU 158-163 / 139-141 / 194,
// 8 per CU 137 / 87-88 / 119, 4 per CU 125-131 / 78-85 / 65, 2 per CU 121 / 74-76 / 55.  More than 16 per CU is not measured and keeps one wave.
static int tile_waves_per_task_plain(uint32_t nStreams, int nCU, int tileWaves) {
    if (tileWaves > 0) return tileWaves;
    const double perCU = (double)nStreams / (double)std::max(1, nCU);
    return perCU > 16.0 ? 1 : (perCU >= 6.0 ? 2 : 4);
}

void plan_size(const PlanIn &in, BatchPlan &p) {
    typedef unsigned long long ull;
    const bool slicedPath = p.path == PVOL_PATH_SLICED;
    // LDS plans of the kernels (march_lds, pvol_march.hip)
    p.ldsPar = (size_t)in.candCap * 8 + PVOL_MARCH_LDS_FIXED; p.ldsResolve = 624 * 4 + (size_t)in.maxSteps * 4;
    p.ldsSeq = p.ldsResolve + p.ldsPar; p.ldsGroup = pvol_group_lds_bytes(in.candCap);
    if (p.tile == PVOL_TILE_FUSED) { p.ldsTile = pvol_tile_lds_bytes(in.maxSteps, in.spp, true, in.nTris, false); p.tileWavesPerTask = 1; }
    else if (p.tile != PVOL_TILE_NONE) { p.ldsTile = pvol_tile_lds_bytes(0, in.spp, false, in.nTris, in.distant != 0); p.tileWavesPerTask = tile_waves_per_task(in); }
    if (slicedPath) {
        const size_t stride = pvol_rec_stride(in.maxSteps, is_density_region(in.volKind));
        size_t m = ((size_t)4 << 30) / (stride * (size_t)in.nStreams);   // the record budget
        // nused beyond the bucket plan hands every dense lookup of a slice to the exact pass: keep that list within 8 GB
        if (in.nUsed > 100) m = std::min<size_t>(m, std::max<size_t>(64, (((size_t)8 << 30) / sizeof(DeferRec) / 64) / (size_t)in.nStreams));
        if (in.specOn) m = std::min<size_t>(m, std::max<size_t>(64, ((size_t)8 << 20) / (size_t)in.nStreams));   // keeps a slice's segment pool within its 16 M slots
        m = std::max<size_t>(64, std::min<size_t>(m, ((size_t)in.maxRays + 63) & ~(size_t)63));
        m &= ~(size_t)63;
        if (in.knobs.sliceRays >= 64) m = (size_t)in.knobs.sliceRays & ~(size_t)63;   // testing: force many slices
        if (in.hasTile) {   // a slice holds whole pixels (both powers of two)
            const size_t unit = std::max<size_t>(64, in.spp);
            m = std::max(unit, m / unit * unit);
        }
        p.recStride = (uint32_t)stride; p.sliceM = (uint32_t)m;
        p.nSlices = in.maxRays ? (in.maxRays + p.sliceM - 1) / p.sliceM : 1;
        p.recBytes = stride * (size_t)in.nStreams * p.sliceM; p.stateBytes = sizeof(uint32_t) * 625 * (size_t)in.nStreams;
    }
    // rays one launch marches: the batch, or one slice of every stream
    const ull chunks = slicedPath ? (ull)((p.sliceM + 63) / 64) * in.nStreams : ((ull)in.nRays + 63ull) / 64ull;
    const ull gchunks = slicedPath ? (ull)((p.sliceM + 511) / 512) * in.nStreams : ((ull)in.nRays + 511ull) / 512ull;   // GRP_CH rays per chunk
    const size_t inFlight = slicedPath ? (size_t)p.sliceM * in.nStreams : (size_t)in.nRays;
    if (p.path != PVOL_PATH_SEQ) p.nWaves = (uint32_t)std::min<ull>(chunks, (ull)in.nCU * 16ull);
    p.fixWaves = (uint32_t)(in.nCU * in.fixWavesPerCU);
    if (p.groupForm) {
        p.gWaves = (uint32_t)std::min<ull>(gchunks, (ull)in.nCU * (ull)in.groupWavesPerCU);
        // room for the lookups the bucket plan hands over (a fraction of a percent of ~40 per ray on C2); a list that overflows raises needSeq and
        // the batch is redone, never truncated.  nused beyond the bucket plan sends every dense lookup to the exact pass (C3: ~14 per ray)
        if (!slicedPath) p.deferWant = inFlight / 2 + 65536;
        else p.deferWant = std::min<size_t>((in.nUsed > 100 ? inFlight * 64 : inFlight) + 65536, ((size_t)8 << 30) / sizeof(DeferRec));
    }
    if (in.specOn) {   // segments of one batch / slice: twice its camera samples, 64 k .. 16 M (the link holds 25 bits)
        const size_t cap = in.knobs.specPool > 0 ? (size_t)in.knobs.specPool : std::max<size_t>(65536, 2 * inFlight);
        p.specCap = std::min<size_t>(cap, (size_t)1 << 24);
    }
}

void pvol_plan_batch(const PlanIn *in, BatchPlan *out) {
    *out = plan_path(*in);
    if (out->rc == PVOL_OK) plan_size(*in, *out);
}

// ---- the moment form's gate and constants (pvol_host.h): pure, no HIP call, no context, no environment
// sigma_t's midrange as the float the kernels multiply by, and the largest |sigma_t_b - it|
static float moment_sig_bar(const float *sigA, const float *sigS, double *maxDelta) {
    float lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < PVOL_NBINS; ++b) { const float t = sigA[b] + sigS[b]; lo = std::min(lo, t); hi = std::max(hi, t); }
    const float bar = (float)(0.5 * ((double)lo + (double)hi));
    *maxDelta = std::max((double)hi - (double)bar, (double)bar - (double)lo);
    return bar;
}
// smallest N in 1..maxN with x^N / N! e^x < 2^-25, x = max|delta| pathBound; 0 = none
static int moment_terms(const float *sigA, const float *sigS, double pathBound, int maxN) {
    double maxDelta = 0.0;
    const float bar = moment_sig_bar(sigA, sigS, &maxDelta);
    if (!std::isfinite(bar) || !std::isfinite(pathBound) || !(pathBound >= 0.0)) return 0;
    const double x = maxDelta * pathBound;
    double term = exp(x);   // x^N / N! e^x
    for (int n = 1; n <= maxN; ++n) {
        term *= x / n;
        if (term < ldexp(1.0, -25)) return n;
    }
    return 0;
}
int pvol_moment_gate(const float *sigA, const float *sigS, double pathBound) {
    if (!sigA || !sigS) return 0;
    return moment_terms(sigA, sigS, pathBound, MOM_ORDERS);
}

float pvol_precore_bound(float theta, float rho) { return precore_bound(theta, rho); }
float pvol_precore_kappa(const char *env) { return env_precore_kappa(env); }

// The longest main diagonal of the medium's extent in world space (the inverse of w2v's linear part applied to the box's edges): no
// segment inside the medium is longer.  INFINITY where w2v is projective or singular.
static double extent_world_diagonal(const DevScene &h) {
    const float *w = h.w2v;
    if (w[12] != 0.f || w[13] != 0.f || w[14] != 0.f || w[15] != 1.f) return INFINITY;
    const double m[3][3] = {{w[0], w[1], w[2]}, {w[4], w[5], w[6]}, {w[8], w[9], w[10]}};
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (!std::isfinite(det) || det == 0.0) return INFINITY;
    double inv[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {   // cofactor of (j, i) over det
            const int a = (j + 1) % 3, b = (j + 2) % 3, c = (i + 1) % 3, d = (i + 2) % 3;
            inv[i][j] = (m[a][c] * m[b][d] - m[a][d] * m[b][c]) / det;
        }
    const double e[3] = {(double)h.extHi[0] - h.extLo[0], (double)h.extHi[1] - h.extLo[1], (double)h.extHi[2] - h.extLo[2]};
    double best = 0.0;
    for (int s = 0; s < 4; ++s) {
        const double v[3] = {e[0], (s & 1) ? -e[1] : e[1], (s & 2) ? -e[2] : e[2]};
        double l2 = 0.0;
        for (int i = 0; i < 3; ++i) { const double u = inv[i][0] * v[0] + inv[i][1] * v[1] + inv[i][2] * v[2]; l2 += u * u; }
        best = std::max(best, sqrt(l2));
    }
    return best * (1.0 + 1e-6);   // the kernels measure lengths in fp32
}

int pvol_moment_scene(DevScene &h, MomentWeights *wts) {
    h.momSigBar = 0.f;
    memset(h.momEmit, 0, sizeof(h.momEmit)); memset(h.momDirect, 0, sizeof(h.momDirect));
    if (wts) memset(wts, 0, sizeof(*wts));
    if (h.volKind != PVOL_VOLUME_HOMOGENEOUS) return 0;
    const double diag = extent_world_diagonal(h);
    // flux and emission are attenuated over the view ray's rest (<= diag): MOM_ORDERS terms; the direct term over that plus the
    // shadow ray's way out (<= 2 diag): one term more
    const int terms = moment_terms(h.sigA, h.sigS, diag, MOM_ORDERS);
    if (terms < 1 || moment_terms(h.sigA, h.sigS, 2.0 * diag, MOM_ORDERS + 1) < 1) return 0;
    double maxDelta = 0.0;
    h.momSigBar = moment_sig_bar(h.sigA, h.sigS, &maxDelta);
    const float *cie[3] = {h.cieX, h.cieY, h.cieZ};
    double emit[9] = {0}, direct[PVOL_MAX_LIGHTS][12] = {{0}};
    for (int b = 0; b < PVOL_NBINS; ++b) {
        const float sigT = h.sigA[b] + h.sigS[b];
        const double d = 0.6931471805599453 * ((double)sigT - (double)h.momSigBar);
        const double albedo = sigT != 0.f ? (double)h.sigS[b] / (double)sigT : 0.0;
        double pw = 1.0;   // (ln2 delta_b)^n / n!
        for (int n = 0; n <= MOM_ORDERS; ++n) {
            for (int c = 0; c < 3; ++c) {
                if (n < MOM_ORDERS) {
                    if (wts) wts->w[4 * n + c][b] = (float)(cie[c][b] * albedo * pw);
                    emit[3 * n + c] += (double)cie[c][b] * ((double)h.sigA[b] * (double)h.le[b]) * pw;
                }
                for (int l = 0; l < h.nLights && l < PVOL_MAX_LIGHTS; ++l)
                    direct[l][3 * n + c] += (double)cie[c][b] * ((double)h.sigS[b] * (double)h.lights[l].intensity[b]) * pw;
            }
            pw *= d / (n + 1);
        }
    }
    for (int i = 0; i < 9; ++i) h.momEmit[i] = (float)emit[i];
    for (int l = 0; l < PVOL_MAX_LIGHTS; ++l) for (int i = 0; i < 12; ++i) h.momDirect[l][i] = (float)direct[l][i];
    return terms;
}

LaunchKnobs pvol_read_knobs() { return pvol_env_launch(pvol_env_get); }
// every read point of pvol_env.h over the caller's table (a name that is not in it is unset) instead of the process environment
void pvol_env_parse(const char *const *names, const char *const *values, uint32_t n, EnvKnobs *out) {
    *out = pvol_env_all([&](const char *name) -> const char * {
        for (uint32_t i = 0; i < n; ++i) if (!strcmp(names[i], name)) return values[i];
        return 0;
    });
}

// Whether a single march step can reach the Russian roulette (Tr.y() < 1e-3, photonvolume.cpp:156-161): Tr is
// ASSIGNED per step, a step is at most stepSize long, so exp(-stepSize * max sigma_t) bounds it from below.
static bool roulette_possible(const pvol_ctx *c) {
    float m = 0.f;
    for (int i = 0; i < PVOL_NBINS; ++i) m = std::max(m, c->hs.sigA[i] + c->hs.sigS[i]);
    // VolumeGrid: trilinear interpolation never exceeds the grid maximum (exponential: the maximum over the extent's corners), and
    // the stepped tau() of a segment (samples every stepSize/2, DensityRegion::tau) can overshoot the segment by one sample:
    // 1.5 x stepSize bounds it
    const float dens = is_density_region(c->hs.volKind) ? 1.5f * c->maxDensity : 1.f;
    return !(c->hs.stepSize * m * dens < 6.8f);
}

// ---- VolumeIntegrator "single" (pvol_host.h): pure up to single_plan_input
int pvol_single_roulette_possible(int volKind, double diag, float maxSigmaT, float maxDensity) {
    if (volKind == PVOL_VOLUME_NONE) return 0;
    const double dens = is_density_region(volKind) ? 1.5 * (double)maxDensity : 1.0;
    return !(diag * (double)maxSigmaT * dens < 6.8);
}

void pvol_single_plan(const SinglePlanIn *in, SinglePlan *out) {
    SinglePlan p = {PVOL_OK, PVOL_SINGLE_SEQ, "single_seq_kernel"};
    const bool extent = in->volKind == PVOL_VOLUME_HOMOGENEOUS || in->volKind == PVOL_VOLUME_NONE;
    const bool par = in->nLights <= 1 && extent && !in->hasInit && !in->forceSeq;
    if (in->volKind == PVOL_VOLUME_RAINBOW) p.rc = PVOL_E_UNSUPPORTED;   // rainbowReflection is the photon integrator's own
    else if (in->gather) p.rc = PVOL_E_UNSUPPORTED;
    else if (in->hasTile && (in->nLights > 1 || is_density_region(in->volKind) || in->specOn || in->rouletteRay)) p.rc = PVOL_E_UNSUPPORTED;
    else if (par) { p.form = PVOL_SINGLE_PAR; p.kernel = "single_par_kernel"; }
    else if (in->hasTile) p.rc = PVOL_E_UNSUPPORTED;
    *out = p;
}

static SinglePlanIn single_plan_input(const pvol_ctx *c, bool hasInit, bool hasTile, bool specOn) {
    const DevScene &h = c->hs;
    float m = 0.f;
    for (int i = 0; i < PVOL_NBINS; ++i) m = std::max(m, h.sigA[i] + h.sigS[i]);
    SinglePlanIn in = {};
    in.volKind = h.volKind; in.nLights = h.nLights;
    in.rouletteRay = pvol_single_roulette_possible(h.volKind, h.volKind == PVOL_VOLUME_NONE ? 0.0 : extent_world_diagonal(h), m, c->maxDensity);
    in.hasInit = hasInit; in.forceSeq = c->knobs.forceSeq; in.hasTile = hasTile; in.specOn = specOn;
    return in;
}

static int single_limit_status(const pvol_ctx *c, bool forceSeqCounts) {
    if (!c || c->volInt != PVOL_VOLINT_SINGLE || !c->haveScene) return PVOL_OK;
    SinglePlanIn in = single_plan_input(c, false, true, c->hs.surf.enabled != 0 && c->specOn);
    if (!forceSeqCounts) in.forceSeq = 0;
    SinglePlan p;
    pvol_single_plan(&in, &p);
    return p.rc;
}
int pvol_single_render_status(const pvol_ctx *c) { return single_limit_status(c, true); }
int pvol_single_caller_status(const pvol_ctx *c) { return single_limit_status(c, false); }

static PlanIn plan_input(const pvol_ctx *c, const BatchArgs &b) {
    const DevScene &h = c->hs;
    PlanIn in = {};
    in.nLights = h.nLights; in.volKind = h.volKind; in.g = h.g; in.nPhotons = h.nPhotons; in.nUsed = h.nUsed; in.candCap = h.candCap;
    in.maxSteps = h.maxSteps; in.nTris = h.nTris; in.roulette = roulette_possible(c); in.distant = h.nLights > 0 && h.lights[0].kind == PVOL_LIGHT_DISTANT;
    const CtxKnobs &k = c->knobs;
    in.forceSeq = k.forceSeq; in.noGroup = k.noGroup; in.noLite = k.noLite; in.statsOn = c->statsOn;
    in.nCU = c->nCU; in.groupWavesPerCU = k.groupWavesPerCU; in.fixWavesPerCU = k.fixWavesPerCU; in.tileWaves = k.tileWaves;
    in.nRays = b.nRays; in.nStreams = b.nStreams; in.maxRays = b.maxRaysPerStream; in.hasInit = b.initState != 0; in.transOnly = b.transOnly != 0; in.hasTile = b.tile != 0;
    in.spp = b.tile ? b.tile->spp : 0; in.specOn = b.tile && b.tile->specOn; in.hasTauOut = b.tauOut != 0;
    in.momentTerms = (int16_t)(h.mom ? c->momentTerms : 0); in.outXYZ = b.outputKind == PVOL_OUT_XYZ; in.noMoments = k.noMoments;
    in.knobs = pvol_read_knobs();
    return in;
}

bool pvol_reserve(DevBuf &b, size_t want, hipStream_t stream) {
    if (want <= b.bytes) return true;
    hipStreamSynchronize(stream);   // an earlier batch may still read the old buffer
    b.bytes = 0;
    if (!b.p.alloc(want)) return false;
    b.bytes = want;
    return true;
}

// Timing events: every batch records a pair on its launch stream.  Finished pairs are folded into the running sum and
// recycled here, at the next launch and in pvol_kernel_time_ms, so the list stays short however many batches a caller
// issues without ever asking for the time (the per-sample shim issues one per camera sample).  Caller holds t.mu.
static bool harvest_events(BatchTimer &t, bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < t.pending.size(); ++i) {
        BatchTimer::Pair &p = t.pending[i];
        // more than 64 batches in flight: wait for the oldest instead of growing
        const bool block = wait || t.pending.size() - i > 64;
        hipError_t q = block ? hipEventSynchronize(p.second.get()) : hipEventQuery(p.second.get());
        if (q == hipSuccess) {
            float ms = 0.f;
            if (ok(hipEventElapsedTime(&ms, p.first.get(), p.second.get()))) { t.timeMs += ms; t.launches += 1; }
            t.pool.push_back(std::move(p));
        } else if (q == hipErrorNotReady) {
            t.pending[keep++] = std::move(p);
        } else {
            (void)hipGetLastError();
            t.pool.push_back(std::move(p));
            if (wait) { t.pending.erase(t.pending.begin(), t.pending.begin() + (i + 1 - keep)); return false; }
        }
    }
    t.pending.resize(keep);
    return true;
}

// Orders `stream` behind every batch of this context still running on another stream (their end events): the device entry
// points return with their kernels in flight, and those kernels use the context's scratch (dWords and `buf`).
int pvol_order_after_pending(pvol_ctx *c, hipStream_t stream) {
    std::lock_guard<std::mutex> g(c->timer.mu);
    harvest_events(c->timer, false);
    for (const auto &p : c->timer.pending)
        if (!ok(hipStreamWaitEvent(stream, p.second.get(), 0))) return PVOL_E_NO_DEVICE;
    return PVOL_OK;
}

// Phase timing (off by default: two events per kernel group otherwise).  A mark is an event on the launch stream; a mark whose
// event cannot be created is dropped.
void pvol_phase_mark(pvol_ctx *c, hipStream_t stream, int id) {
    PhaseTimer &ph = c->phases;
    if (!ph.on) return;
    std::lock_guard<std::mutex> g(c->timer.mu);
    DevEvent e;
    if (!ph.pool.empty()) { e = std::move(ph.pool.back()); ph.pool.pop_back(); }
    else if (!e.create(true)) return;
    hipEventRecord(e.get(), stream);
    ph.marks.emplace_back(id, std::move(e));
}

// ---- specular recursion (pvol_spec_dev.h): the pool of segment rays of one batch (COUNT mode) or one slice (FUSED mode).
// Emptied in front of every tile pre-pass that fills it, and handed to that pre-pass through its TileArgs.
static int spec_pool_reset(pvol_ctx *c, TileArgs *t, size_t cap, hipStream_t stream) {
    memset(&c->hSegStream, 0, sizeof(pvol_stream)); c->hSegStream.n_rays = (uint32_t)cap;
    pvol_ray *segRays = pvol_buf<pvol_ray>(c, PVOL_BUF_SEG_RAYS);
    uint32_t *segCounter = pvol_buf<uint32_t>(c, PVOL_BUF_SEG_COUNTER);
    if (!ok(hipMemsetAsync(segCounter, 0, 16, stream)) || !ok(hipMemcpyAsync(pvol_buf<pvol_stream>(c, PVOL_BUF_SEG_STREAM), &c->hSegStream, sizeof(pvol_stream), hipMemcpyHostToDevice, stream)) ||
        !ok(pvol_launch_spec_fill(segRays, (uint32_t)cap, stream)) || !ok(hipMemsetAsync(pvol_buf<float>(c, PVOL_BUF_SEG_OUT), 0, sizeof(float) * 60 * cap, stream)))
        return PVOL_E_NO_DEVICE;
    t->specOn = 1; t->segRays = segRays; t->segInfo = pvol_buf<SegInfo>(c, PVOL_BUF_SEG_INFO); t->segCounter = segCounter; t->segCap = (uint32_t)cap;
    t->segRecords = pvol_buf<unsigned char>(c, PVOL_BUF_SEG_RECORDS);
    return PVOL_OK;
}
// The segments' own volume Li() (spectral), the surface term at their matte hits, and the fold into the camera samples.
// `replay`: the pool's records were written by the FUSED tile pre-pass (li_replay_kernel); else no drawn value matters (li_par_kernel).
static int spec_finish(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, const LiArgs &a, bool replay) {
    const size_t cap = p.specCap;
    pvol_ray *segRays = pvol_buf<pvol_ray>(c, PVOL_BUF_SEG_RAYS);
    float *segOut = pvol_buf<float>(c, PVOL_BUF_SEG_OUT);
    LiArgs sa = a;
    sa.rays = segRays; sa.nRays = (uint32_t)cap; sa.streams = pvol_buf<pvol_stream>(c, PVOL_BUF_SEG_STREAM); sa.nStreams = 1; sa.outputKind = PVOL_OUT_SPECTRAL;
    sa.out = segOut; sa.draws = 0; sa.initState = 0; sa.finalState = 0; sa.tauOut = 0; sa.defer = 0; sa.deferCount = 0; sa.deferCap = 0; sa.gated = 0;
    sa.records = pvol_buf<unsigned char>(c, PVOL_BUF_SEG_RECORDS); sa.sliceM = (uint32_t)cap; sa.sliceK = 0; sa.state = 0; sa.status = 0;
    const uint32_t nWaves = (uint32_t)std::min<unsigned long long>((cap + 63) / 64, (unsigned long long)c->nCU * 16ull);
    if (!ok(hipMemsetAsync(c->dWords.get(), 0, 4 * sizeof(uint32_t), b.stream))) return PVOL_E_NO_DEVICE;
    const RegionLaunchers &K = pvol_launchers(c->hs.volKind);
    hipError_t e = replay ? K.liReplay(&sa, p.ldsPar, c->hs.candCap, nWaves, b.stream)
                          : K.liPar(&sa, p.ldsPar, c->hs.candCap, false, nWaves, b.stream);
    if (!ok(e)) return PVOL_E_NO_DEVICE;
    SurfArgs su = {};
    su.scene = c->ds.get(); su.rays = segRays; su.nRays = (uint32_t)cap; su.out = segOut; su.tau = 0; su.surfOut = 0; su.counters = c->dCounters.get(); su.link = 0; su.spectral = 1;
    if (!ok(K.surface(&su, (uint32_t)std::min<unsigned long long>((cap + 63) / 64, (unsigned long long)c->nCU * 24ull), b.stream))) return PVOL_E_NO_DEVICE;
    SpecComposeArgs ca = {};
    ca.scene = c->ds.get(); ca.link = pvol_buf<uint32_t>(c, PVOL_BUF_SPEC_LINK); ca.info = pvol_buf<SegInfo>(c, PVOL_BUF_SEG_INFO); ca.segOut = segOut; ca.tau = a.tauOut;
    ca.out = b.out; ca.surfOut = b.specSurfOut; ca.first = 0; ca.nRays = b.nRays;
    return ok(pvol_launch_spec_compose(&ca, b.stream)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

// ---- the three paths of a batch: each fills what is left of LiArgs and launches, in stream order
// sampler + camera pre-pass that COUNTs Li()'s draws for the whole batch, once (`t`: the batch as one slice)
static int run_tile_count(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, const LiArgs &t, const TileArgs *tile) {
    pvol_phase_mark(c, b.stream, PVOL_PHASE_TILE);
    const DevScene &h = c->hs;
    TilePlainIn g = {};
    g.tile = p.tile; g.volKind = h.volKind; g.nLights = h.nLights; g.light0Kind = h.nLights > 0 ? h.lights[0].kind : -1;
    g.hasBvh = h.bvhNodes != 0; g.nSpheres = h.nSpheres; g.nTris = h.nTris; g.surfOn = h.surf.enabled != 0;
    g.specLink = tile->specOn || tile->specLink != 0; g.tileGeneral = c->knobs.tileGeneral;
    const bool plain = pvol_tile_plain_gate(&g) != 0;
    c->lastTileForm = plain ? "plain" : "general";
    // the plan's wave count is the general form's; PLAIN has its own optimum (the LDS plan, p.ldsTile, is the same for every wave count)
    const int waves = plain ? tile_waves_per_task_plain(b.nStreams, c->nCU, c->knobs.tileWaves) : p.tileWavesPerTask;
    return ok(pvol_launchers(h.volKind).tile(&t, tile, false, p.ldsTile, h.candCap, b.stream, waves, plain, &c->lastTileKernel)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}
static int run_par(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, LiArgs &a) {
    const RegionLaunchers &K = pvol_launchers(c->hs.volKind);
    hipError_t e = p.groupForm ? K.liGroup(&a, p.ldsGroup, c->hs.candCap, c->statsOn, p.gWaves, p.fixWaves, 0, b.stream)
                               : K.liPar(&a, p.ldsPar, c->hs.candCap, c->statsOn, p.nWaves, b.stream);
    if (ok(e)) {   // runs only if a ray raised needSeq (gate read on the device: no host sync here)
        a.gated = 1;
        e = K.liSeq(&a, p.ldsSeq, c->hs.candCap, c->statsOn, b.stream);
        a.gated = 0;
    }
    if (!ok(e)) return PVOL_E_NO_DEVICE;
    return p.specCap ? spec_finish(c, b, p, a, false) : PVOL_OK;
}

static int run_sliced(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, LiArgs &a, TileArgs *tile) {
    a.records = pvol_buf<unsigned char>(c, PVOL_BUF_RECORDS); a.recStride = p.recStride; a.sliceM = p.sliceM; a.state = pvol_buf<uint32_t>(c, PVOL_BUF_STATE);
    a.liteResolve = p.liteResolve; a.fixGroup = p.fixGroup;
    if (p.tile == PVOL_TILE_GRID_COUNT) {
        LiArgs t = a;
        t.sliceK = 0; t.sliceM = 0xffffffc0u; t.state = 0;
        if (run_tile_count(c, b, p, t, tile) != PVOL_OK) return PVOL_E_NO_DEVICE;
    }
    const RegionLaunchers &K = pvol_launchers(c->hs.volKind);
    for (uint32_t k = 0; k < p.nSlices; ++k) {
        a.sliceK = k;
        hipMemsetAsync(c->dWords.get(), 0, 4 * sizeof(uint32_t), b.stream);
        if (p.specCap && spec_pool_reset(c, tile, p.specCap, b.stream) != PVOL_OK) return PVOL_E_NO_DEVICE;
        if (p.tile == PVOL_TILE_FUSED) {
            pvol_phase_mark(c, b.stream, PVOL_PHASE_TILE);
            c->lastTileForm = "general";
            if (!ok(K.tile(&a, tile, true, p.ldsTile, c->hs.candCap, b.stream, p.tileWavesPerTask, false, &c->lastTileKernel))) return PVOL_E_NO_DEVICE;
        }
        pvol_phase_mark(c, b.stream, PVOL_PHASE_MARCH);   // incl. the RNG-only resolve pass of a slice where there is one
        if (!ok(K.liSlice(&a, p.ldsResolve, p.ldsPar, c->hs.candCap, c->statsOn, p.nWaves, b.stream, p.resolve != 0, p.groupForm, p.ldsGroup,
                                     p.gWaves, p.fixWaves))) return PVOL_E_NO_DEVICE;
        // this slice's segments: their Li() from the records the pre-pass left, then the fold into the slice's camera samples
        if (p.specCap && spec_finish(c, b, p, a, true) != PVOL_OK) return PVOL_E_NO_DEVICE;
    }
    return PVOL_OK;
}

// VolumeIntegrator "single": the ray-parallel form backed by the sequential one behind the needSeq gate, or the sequential form alone
static int run_single(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, LiArgs &a, int form) {
    const RegionLaunchers &K = pvol_launchers(c->hs.volKind);
    hipError_t e = hipSuccess;
    if (form == PVOL_SINGLE_PAR) {
        e = K.singlePar(&a, p.nWaves, b.stream);
        a.gated = 1;
    } else if (!ok(hipMemsetAsync(c->dWords.get(), 0, 4 * sizeof(uint32_t), b.stream))) {   // the gate word a coalesced batch reads back
        return PVOL_E_NO_DEVICE;
    }
    if (ok(e)) e = K.singleSeq(&a, p.ldsResolve, b.stream);
    a.gated = 0;
    return ok(e) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

static int run_seq(pvol_ctx *c, const BatchArgs &b, const BatchPlan &p, LiArgs &a) {
    return ok(pvol_launchers(c->hs.volKind).liSeq(&a, p.ldsSeq, c->hs.candCap, c->statsOn, b.stream)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

// Scratch of the plan's sizes, all of it before the first enqueue of the batch.
static int reserve_scratch(pvol_ctx *c, const BatchPlan &p, hipStream_t stream) {
    const size_t cap = p.specCap;
    if (!pvol_reserve(c->buf[PVOL_BUF_RECORDS], p.recBytes, stream) || !pvol_reserve(c->buf[PVOL_BUF_STATE], p.stateBytes, stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_DEFER], p.deferWant * sizeof(DeferRec), stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_SEG_RAYS], sizeof(pvol_ray) * cap, stream) || !pvol_reserve(c->buf[PVOL_BUF_SEG_INFO], sizeof(SegInfo) * cap, stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_SEG_OUT], sizeof(float) * 60 * cap, stream) || !pvol_reserve(c->buf[PVOL_BUF_SEG_RECORDS], p.recStride * cap, stream) ||
        !pvol_reserve(c->buf[PVOL_BUF_SEG_COUNTER], cap ? 16 : 0, stream) || !pvol_reserve(c->buf[PVOL_BUF_SEG_STREAM], cap ? sizeof(pvol_stream) : 0, stream))
        return PVOL_E_NO_MEMORY;
    return PVOL_OK;
}

int pvol_launch_batch(pvol_ctx *c, const BatchArgs &b) {
    PlanIn in = plan_input(c, b);
    // Transmittance() is the same function under both integrators (single.cpp:48-63 is photonvolume.cpp:15-30)
    const bool single = c->volInt == PVOL_VOLINT_SINGLE && !b.transOnly;
    SinglePlan sp = {};
    if (single) {
        const SinglePlanIn si = single_plan_input(c, in.hasInit != 0, in.hasTile != 0, in.specOn != 0);
        pvol_single_plan(&si, &sp);
        if (sp.rc != PVOL_OK) return sp.rc;
        in.roulette = si.rouletteRay;   // the COUNT pre-pass's 4 + 6n + n + u is exact where the ACCUMULATED Tr.y() stays above 1e-3
    }
    BatchPlan p = plan_path(in);
    if (p.rc != PVOL_OK) return p.rc;
    if (single) {   // no map is read: no bucket form, no records; a SLICED answer takes the sequential form (never with a tile)
        p.path = sp.form == PVOL_SINGLE_PAR ? PVOL_PATH_PAR : PVOL_PATH_SEQ;
        p.groupForm = 0; p.fixGroup = 0; p.liteResolve = 0; p.resolve = 0; p.kernel = sp.kernel;
    }
    const hipStream_t stream = b.stream;
    BatchTimer &timer = c->timer;
    BatchTimer::Pair taken;
    {
        std::lock_guard<std::mutex> g(timer.mu);
        harvest_events(timer, false);
        if (!timer.pool.empty()) { taken = std::move(timer.pool.back()); timer.pool.pop_back(); }
        else if (!taken.first.create(true) || !taken.second.create(true)) return PVOL_E_NO_DEVICE;
    }
    BatchTimer::Lease lease{timer, std::move(taken)};   // back to the pool on every early return below
    const BatchTimer::Pair &ev = lease.ev;
    if (p.path == PVOL_PATH_SLICED && in.maxRays == 0) {   // device entry point: the stream table lives on the device
        std::vector<pvol_stream> hs(b.nStreams);   // read on the caller's stream: ordered behind whatever produced the table
        if (!ok(hipMemcpyAsync(hs.data(), b.streams, sizeof(pvol_stream) * (size_t)b.nStreams, hipMemcpyDeviceToHost, stream)) ||
            !ok(hipStreamSynchronize(stream))) return PVOL_E_NO_DEVICE;
        for (uint32_t i = 0; i < b.nStreams; ++i) in.maxRays = std::max(in.maxRays, hs[i].n_rays);
    }
    plan_size(in, p);
    int rc = reserve_scratch(c, p, stream);
    if (rc != PVOL_OK) return rc;
    c->lastKernel = p.kernel;
    TileArgs tile;   // the tile driver's arguments, completed here with the segment pool of the specular recursion
    if (b.tile) tile = *b.tile;
    LiArgs a = {};
    a.scene = c->ds.get(); a.rays = b.rays; a.streams = b.streams; a.nStreams = b.nStreams; a.nRays = b.nRays; a.outputKind = b.outputKind;
    a.out = b.out; a.draws = b.draws; a.initState = b.initState; a.finalState = b.finalState; a.counters = c->dCounters.get();
    a.transmittanceOnly = b.transOnly; a.chunkCounter = c->dWords.get(); a.needSeq = c->dWords.get() + 1; a.gated = 0;
    a.tauOut = b.tauOut; a.status = b.status; a.grpGuess = in.knobs.groupGuess; a.moments = p.groupForm == GRP_FORM_MOMENTS;
    a.grpPrecore = c->knobs.groupPrecore;
    if (p.groupForm) {
        a.defer = pvol_buf<DeferRec>(c, PVOL_BUF_DEFER); a.deferCount = c->dWords.get() + 2;
        a.deferCap = (uint32_t)std::min<size_t>(c->buf[PVOL_BUF_DEFER].bytes / sizeof(DeferRec), 0xffffffffu);
        if (p.path == PVOL_PATH_SLICED) { a.fxgWiden = in.knobs.fxgWiden; a.fxgAim = in.knobs.fxgAim; }
    }
    if (p.path == PVOL_PATH_PAR) hipMemsetAsync(c->dWords.get(), 0, 3 * sizeof(uint32_t), stream);
    if (p.tile == PVOL_TILE_COUNT) {   // outside the timed region of the march kernel; the march keeps the pre-pass's slice fields
        a.sliceK = 0; a.sliceM = 0xffffffc0u; a.state = 0;
        if (p.specCap) rc = spec_pool_reset(c, &tile, p.specCap, stream);
        if (rc == PVOL_OK) rc = run_tile_count(c, b, p, a, &tile);
        if (rc != PVOL_OK) return rc;
    }
    hipEventRecord(ev.first.get(), stream);
    pvol_phase_mark(c, stream, PVOL_PHASE_MARCH);
    rc = single ? run_single(c, b, p, a, sp.form)
                : p.path == PVOL_PATH_PAR ? run_par(c, b, p, a) : p.path == PVOL_PATH_SLICED ? run_sliced(c, b, p, a, &tile) : run_seq(c, b, p, a);
    if (rc != PVOL_OK) return rc;
    hipEventRecord(ev.second.get(), stream);
    pvol_phase_mark(c, stream, PVOL_PHASE_END);
    lease.done = true;   // to `pending`
    return PVOL_OK;
}

static int check_errors(pvol_ctx *c) {
    DevCounters h;
    if (!ok(hipMemcpy(&h, c->dCounters.get(), sizeof(h), hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
    if (h.nErrors) {
        unsigned long long zero = 0;
        hipMemcpy(&c->dCounters.get()->nErrors, &zero, sizeof(zero), hipMemcpyHostToDevice);
        return PVOL_E_LIMIT;
    }
    return PVOL_OK;
}

int pvol_li_batch_device(pvol_ctx *c, const pvol_ray *dRays, uint32_t nRays, pvol_stream *dStreams, uint32_t nStreams,
                         int outputKind, float *dOut, uint32_t *dDraws, void *hipStream) {
    if (!c || (nRays && !dRays) || (nStreams && !dStreams) || (nRays && !dOut)) return PVOL_E_INVALID;
    if (outputKind != PVOL_OUT_SPECTRAL && outputKind != PVOL_OUT_XYZ) return PVOL_E_INVALID;
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    if (!nStreams) return PVOL_OK;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    BatchArgs b = {};   // maxRaysPerStream 0: the stream table lives on the device
    b.rays = dRays; b.nRays = nRays; b.streams = dStreams; b.nStreams = nStreams; b.outputKind = outputKind; b.out = dOut; b.draws = dDraws;
    b.stream = (hipStream_t)hipStream;
    return pvol_launch_batch(c, b);
}

int pvol_check_errors(pvol_ctx *c) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device)) || !ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;
    return check_errors(c);
}

static int host_batch(pvol_ctx *c, const pvol_ray *rays, uint32_t nRays, pvol_stream *streams, uint32_t nStreams, int outputKind,
                      float *out, uint32_t *draws, uint32_t *mtState, int transOnly) {
    if (!c || (nRays && (!rays || !out)) || (nStreams && !streams)) return PVOL_E_INVALID;
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    // VolumeIntegrator::Li() is called by every SamplerRendererTask thread at once (samplerrenderer.cpp:247): calls on one
    // context are serialised here, from the upload to the copy-back (the launches share the context's scratch)
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    uint32_t maxRays = 1;
    if (!streams_partition(streams, nStreams, nRays, &maxRays)) return PVOL_E_INVALID;
    if (!nStreams || !nRays) return PVOL_OK;
    const size_t width = transOnly ? 60 : (outputKind == PVOL_OUT_SPECTRAL ? 60 : 4);
    std::vector<float> rows(transOnly ? width * nRays : 0);   // the kernel writes [Lv(30) | T(30)] rows; the ABI returns T only
    HostStage st;
    BatchArgs b = {};
    b.rays = st.in(rays, nRays); b.nRays = nRays; b.nStreams = nStreams; b.outputKind = transOnly ? PVOL_OUT_SPECTRAL : outputKind;
    b.out = st.out(transOnly ? rows.data() : out, width * nRays);
    b.streams = st.inout(streams, nStreams);
    b.draws = draws ? st.out(draws, nRays) : st.scratch<uint32_t>(nRays);
    b.initState = b.finalState = st.inout(mtState, 625 * (size_t)nStreams);
    b.transOnly = transOnly; b.maxRaysPerStream = maxRays;
    int rc = st.upload();
    if (rc != PVOL_OK) return rc;
    if (!ok(hipMemset(b.out, 0, sizeof(float) * width * nRays))) return PVOL_E_NO_DEVICE;
    rc = pvol_launch_batch(c, b);
    if (rc == PVOL_OK && !ok(hipStreamSynchronize(0))) rc = PVOL_E_NO_DEVICE;
    if (rc == PVOL_OK) rc = check_errors(c);
    if (rc == PVOL_OK) rc = st.download();
    if (rc != PVOL_OK) return rc;
    for (size_t i = 0; i < rows.size() / 60; ++i) memcpy(out + i * 30, rows.data() + i * 60 + 30, sizeof(float) * 30);
    return PVOL_OK;
}

int pvol_li_batch(pvol_ctx *c, const pvol_ray *rays, uint32_t nRays, pvol_stream *streams, uint32_t nStreams, int outputKind,
                  float *out, uint32_t *draws) {
    if (outputKind != PVOL_OUT_SPECTRAL && outputKind != PVOL_OUT_XYZ) return PVOL_E_INVALID;
    return host_batch(c, rays, nRays, streams, nStreams, outputKind, out, draws, 0, 0);
}

int pvol_transmittance_batch(pvol_ctx *c, const pvol_ray *rays, uint32_t nRays, pvol_stream *streams, uint32_t nStreams, float *out) {
    return host_batch(c, rays, nRays, streams, nStreams, PVOL_OUT_SPECTRAL, out, 0, 0, 1);
}

int pvol_li(pvol_ctx *c, const pvol_ray *ray, uint32_t *mt, int32_t *mti, float *Lv, float *T) {
    if (!c || !ray || !mt || !mti || !Lv || !T) return PVOL_E_INVALID;
    if (*mti < 0 || *mti > 624) return PVOL_E_INVALID;
    if (c->co.maxBatch.load(std::memory_order_relaxed) > 1) return pvol_li_coalesced(c, ray, mt, mti, Lv, T);   // pvol_li_coalesce.hip
    return pvol_li_lone(c, ray, mt, mti, Lv, T);
}

// One call as its own batch of one stream on the null stream: pvol_li with coalescing off.
int pvol_li_lone(pvol_ctx *c, const pvol_ray *ray, uint32_t *mt, int32_t *mti, float *Lv, float *T) {
    uint32_t state[625];
    memcpy(state, mt, sizeof(uint32_t) * 624);
    state[624] = (uint32_t)*mti;
    pvol_stream st;
    memset(&st, 0, sizeof(st));
    st.n_rays = 1;
    float out[60];
    int rc = host_batch(c, ray, 1, &st, 1, PVOL_OUT_SPECTRAL, out, 0, state, 0);
    if (rc != PVOL_OK) return rc;
    memcpy(Lv, out, sizeof(float) * 30);
    memcpy(T, out + 30, sizeof(float) * 30);
    memcpy(mt, state, sizeof(uint32_t) * 624);
    *mti = (int32_t)state[624];
    return PVOL_OK;
}

int pvol_set_volume_integrator(pvol_ctx *c, int kind) {
    if (!c || (kind != PVOL_VOLINT_PHOTON && kind != PVOL_VOLINT_SINGLE)) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device)) || !ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;   // batches in flight keep their integrator
    c->volInt = kind;
    return PVOL_OK;
}

int pvol_get_volume_integrator(pvol_ctx *c, int *kind) {
    if (!c || !kind) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    *kind = c->volInt;
    return PVOL_OK;
}

int pvol_enable_stats(pvol_ctx *c, int on) {
    if (!c) return PVOL_E_INVALID;
    c->statsOn = on != 0;
    return PVOL_OK;
}

int pvol_get_stats(pvol_ctx *c, pvol_stats *out, int reset) {
    if (!c || !out) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device)) || !ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;
    DevCounters h;
    if (!ok(hipMemcpy(&h, c->dCounters.get(), sizeof(h), hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
    memset(out, 0, sizeof(*out));
    out->n_rays = h.nRays; out->n_steps = h.nSteps; out->n_tested = h.nTested; out->n_kept = h.nKept;
    out->n_lookups_lt10 = h.nLookupsLt10; out->n_shadow_unoccluded = h.nShadowUnoccluded;
    out->n_guess_retries = h.pad;
    out->group_guess_failed = h.diag[0]; out->group_plan_skipped = h.diag[1]; out->cy_fallback = h.diag[2];
    out->group_deferred_overflow = h.diag[3]; out->group_deferred_too_few = h.diag[4]; out->group_attempts = h.diag[5];
    out->cy_search = h.cySearch; out->cy_select = h.cySelect; out->cy_flux = h.cyFlux; out->cy_total = h.cyTotal;
    if (reset && !ok(hipMemset(c->dCounters.get(), 0, sizeof(DevCounters)))) return PVOL_E_NO_DEVICE;
    return PVOL_OK;
}

const char *pvol_march_kernel_name(pvol_ctx *c) { return c ? c->lastKernel : ""; }
const char *pvol_tile_kernel_name(pvol_ctx *c) { return c ? c->lastTileKernel : ""; }
const char *pvol_tile_form_name(pvol_ctx *c) { return c ? c->lastTileForm : ""; }

int pvol_enable_phase_timing(pvol_ctx *c, int on) {
    if (!c) return PVOL_E_INVALID;
    c->phases.on = on != 0;
    return PVOL_OK;
}

int pvol_get_phase_ms(pvol_ctx *c, double *out6, int reset) {
    if (!c || !out6) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device)) || !ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;
    PhaseTimer &ph = c->phases;
    std::lock_guard<std::mutex> g(c->timer.mu);
    for (size_t i = 0; i + 1 < ph.marks.size(); ++i) {
        const int id = ph.marks[i].first;
        float ms = 0.f;
        if (id >= 0 && id < PVOL_N_PHASES && ok(hipEventElapsedTime(&ms, ph.marks[i].second.get(), ph.marks[i + 1].second.get()))) ph.ms[id] += ms;
    }
    for (size_t i = 0; i < ph.marks.size(); ++i) ph.pool.push_back(std::move(ph.marks[i].second));
    ph.marks.clear();
    for (int i = 0; i < PVOL_N_PHASES; ++i) out6[i] = ph.ms[i];
    if (reset) for (int i = 0; i < PVOL_N_PHASES; ++i) ph.ms[i] = 0.0;
    return PVOL_OK;
}

int pvol_kernel_time_ms(pvol_ctx *c, double *avgMs, uint64_t *launches, int reset) {
    if (!c || !avgMs) return PVOL_E_INVALID;
    BatchTimer &t = c->timer;
    std::lock_guard<std::mutex> g(t.mu);
    if (!harvest_events(t, true)) return PVOL_E_NO_DEVICE;
    *avgMs = t.launches ? t.timeMs / (double)t.launches : 0.0;
    if (launches) *launches = t.launches;
    if (reset) { t.timeMs = 0; t.launches = 0; }
    return PVOL_OK;
}

}  // extern "C"
