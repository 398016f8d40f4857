// pvol_env.h -- every environment knob of the library (DESIGN.md 4.10 lists them): a handful of parse primitives and one function per
// read point, each a pure function of a getter `get(name)` -> the variable's C string or NULL.  Plain C++, no HIP, no getenv: the
// read points pass pvol_env_get (pvol_api.hip, the one place that asks the process), tests/test_env_knobs.py passes a table
// (pvol_env_parse) and never touches the environment.
#ifndef PVOL_ENV_H
#define PVOL_ENV_H
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

__attribute__((visibility("hidden"))) const char *pvol_env_get(const char *name);   // the process environment (pvol_api.hip)

// ---- primitives: what a value means (v: the variable's string, NULL = unset)
static inline bool env_first_is_1(const char *v) { return v && v[0] == '1'; }   // "1", "10" on; "", "0", "01", "true" off
static inline int env_int_at_least(const char *v, int unset, int least) { return v ? std::max(least, atoi(v)) : unset; }
static inline int64_t env_i64(const char *v) { return v ? (int64_t)atoll(v) : (int64_t)0; }
static inline float env_real(const char *v) { return v ? (float)atof(v) : 0.f; }
static inline long env_long(const char *v) { return v ? atol(v) : 0; }
// a test knob that can only lower: a positive x gives min(v, x), anything else v
static inline uint32_t env_lowered(uint32_t v, long x) { return x > 0 ? (uint32_t)std::min<long>(v, x) : v; }
// PVOL_GROUP_PRECORE: unset or unreadable = the default, 0 = the rule off; a kappa above 1 would put theta beyond the guess itself
#define PVOL_PRECORE_DEFAULT 0.7f
static inline float env_precore_kappa(const char *v) {
    if (!v || !v[0]) return PVOL_PRECORE_DEFAULT;
    char *end = 0;
    const float k = strtof(v, &end);
    if (end == v || !(k >= 0.f)) return PVOL_PRECORE_DEFAULT;
    return std::min(k, 1.f);
}

// ---- pvol_create: the knobs a context keeps for its lifetime
struct CtxKnobs {
    bool forceSeq = false;      // PVOL_FORCE_SEQ=1: always take the stream-sequential kernel (testing)
    bool noGroup = false;       // PVOL_NO_GROUP=1: keep li_par_kernel (one wave per ray) where li_group_kernel (one ray per lane) would run
    bool noLite = false;        // PVOL_NO_LITE=1: keep the geometry inside the sequential resolve pass (testing)
    bool noMoments = false;     // PVOL_NO_MOMENTS=1: li_group_kernel keeps summing 30 bins where it would sum XYZ moments
    bool lpNoSort = false;      // PVOL_LPHOTON_NO_SORT=1: pvol_lphoton_batch* serves the points in the caller's order (testing; the same bytes)
    bool tileGeneral = false;   // PVOL_TILE_GENERAL=1: the COUNT-mode tile pre-pass keeps its general form where the plan would take PLAIN
    int groupWavesPerCU = 12;   // PVOL_GROUP_WAVES: resident li_group_kernel waves per CU (LDS plan: 8)
    int fixWavesPerCU = 16;     // PVOL_FIX_WAVES: li_fixup_kernel / li_fixup_group_kernel waves per CU (C3, 8 spp frame: 16.3 s at 8, 13.9 s at 16)
    int tileWaves = 0;          // PVOL_TILE_WAVES: waves per render task of the COUNT-mode tile pre-pass (0 = by tasks per CU)
    float groupPrecore = 0.f;   // PVOL_GROUP_PRECORE (env_precore_kappa): li_group_kernel settles the bucket's inner photons once per wave, 0 = off
};
template <class Get> static inline CtxKnobs pvol_env_context(Get get) {
    CtxKnobs k;
    k.forceSeq = env_first_is_1(get("PVOL_FORCE_SEQ")); k.noGroup = env_first_is_1(get("PVOL_NO_GROUP"));
    k.noLite = env_first_is_1(get("PVOL_NO_LITE")); k.noMoments = env_first_is_1(get("PVOL_NO_MOMENTS"));
    k.lpNoSort = env_first_is_1(get("PVOL_LPHOTON_NO_SORT")); k.tileGeneral = env_first_is_1(get("PVOL_TILE_GENERAL"));
    k.groupWavesPerCU = env_int_at_least(get("PVOL_GROUP_WAVES"), 12, 1); k.fixWavesPerCU = env_int_at_least(get("PVOL_FIX_WAVES"), 16, 1);
    k.tileWaves = env_int_at_least(get("PVOL_TILE_WAVES"), 0, 0);
    k.groupPrecore = env_precore_kappa(get("PVOL_GROUP_PRECORE"));
    return k;
}
// PVOL_LI_COALESCE=<max_batch>, also at pvol_create: the default of pvol_set_li_coalescing, for callers that cannot call it (an
// unchanged binding); 2 .. PVOL_LI_MAX_BATCH, anything else 0 = off
#define PVOL_LI_MAX_BATCH 4096u
template <class Get> static inline uint32_t pvol_env_li_coalesce(Get get) {
    const long v = env_long(get("PVOL_LI_COALESCE"));
    return (v > 1 && v <= (long)PVOL_LI_MAX_BATCH) ? (uint32_t)v : 0u;
}

// ---- every pvol_launch_batch, and the render driver for its batch size; 0 = unset, the default applies
struct LaunchKnobs {
    int64_t sliceRays, specPool, tileBatchRays;   // PVOL_SLICE_RAYS (>= 64: forced slice length), PVOL_SPEC_POOL, PVOL_TILE_BATCH_RAYS
    float groupGuess;                             // PVOL_GROUP_GUESS, already defaulted: li_group_kernel's bucket radius^2 factor
    float fxgWiden, fxgAim;                       // PVOL_FXG_WIDEN, PVOL_FXG_AIM (measurement knobs of li_fixup_group_kernel)
    int32_t fixExact;                             // PVOL_FIX_EXACT set (to anything, the empty string included)
};
template <class Get> static inline LaunchKnobs pvol_env_launch(Get get) {
    LaunchKnobs k;
    k.sliceRays = env_i64(get("PVOL_SLICE_RAYS")); k.specPool = env_i64(get("PVOL_SPEC_POOL")); k.tileBatchRays = env_i64(get("PVOL_TILE_BATCH_RAYS"));
    // li_group_kernel bucket radius^2 = this x the guessed k-th distance^2 (measured at 64 spp: 1.3 55.5, 1.2 57.5, 1.12 58.0,
    // 1.06 56.6, 1.0 51.0 Msamples/s)
    k.groupGuess = env_real(get("PVOL_GROUP_GUESS")); if (!(k.groupGuess >= 1.f)) k.groupGuess = 1.15f;
    k.fxgWiden = env_real(get("PVOL_FXG_WIDEN")); k.fxgAim = env_real(get("PVOL_FXG_AIM")); k.fixExact = get("PVOL_FIX_EXACT") != 0;
    return k;
}

// ---- every render of a -DPVOL_TIMING_KNOBS build: PVOL_TILE_DEBUG set overwrites *debugSkip, unset leaves it
template <class Get> static inline bool pvol_env_tile_debug(Get get, uint32_t *debugSkip) {
    const char *v = get("PVOL_TILE_DEBUG");
    if (v) *debugSkip = (uint32_t)atoi(v);
    return v != 0;
}
// ---- every volume-map build: PVOL_SUBGRID forces the 4 x 4 x 4 second level off (0) / on (1); -1 = unset, the occupancy decides
template <class Get> static inline int pvol_env_subgrid(Get get) {
    const char *v = get("PVOL_SUBGRID");
    return v ? atoi(v) != 0 : -1;
}
// ---- every preprocess (test knobs, applied with env_lowered): PVOL_SHOOT_RANK_CAP_MAX this rank's largest block pool, on a single
// GPU too (set on one rank, that rank alone fails); PVOL_SHOOT_POOL_START the pools' starting sizes (1: every pool is outgrown and
// the round redone)
struct ShootKnobs { long rankCapMax, poolStart; };
template <class Get> static inline ShootKnobs pvol_env_shoot(Get get) {
    return ShootKnobs{env_long(get("PVOL_SHOOT_RANK_CAP_MAX")), env_long(get("PVOL_SHOOT_POOL_START"))};
}
// ---- once per process, at the first shoot: PVOL_SHOOT_WPE, shoot_kernel's waves per SIMD: 3 or 4, everything else 2
template <class Get> static inline int pvol_env_shoot_wpe(Get get) {
    const char *v = get("PVOL_SHOOT_WPE");
    const int w = v ? atoi(v) : 2;
    return (w == 4 || w == 3) ? w : 2;
}

// ---- every parsed knob in one flat record, for the tests (pvol_env_parse, pvol_api.hip)
struct EnvKnobs {
    CtxKnobs ctx;
    uint32_t liCoalesce;
    int32_t subgrid;
    LaunchKnobs launch;
    uint32_t shootRankCapMax, shootPoolStart;   // env_lowered(0xffffffff, .): what the knob leaves of the largest value
    int32_t shootWpe;
    int32_t tileDebugSet; uint32_t tileDebug;   // tileDebug: 0 where unset
    uint32_t pad;
};
static_assert(sizeof(CtxKnobs) == 24 && sizeof(LaunchKnobs) == 40 && sizeof(EnvKnobs) == 96, "tests/test_env_knobs.py mirrors them");
template <class Get> static inline EnvKnobs pvol_env_all(Get get) {
    EnvKnobs k = {};
    k.ctx = pvol_env_context(get); k.liCoalesce = pvol_env_li_coalesce(get); k.subgrid = pvol_env_subgrid(get); k.launch = pvol_env_launch(get);
    const ShootKnobs s = pvol_env_shoot(get);
    k.shootRankCapMax = env_lowered(0xffffffffu, s.rankCapMax); k.shootPoolStart = env_lowered(0xffffffffu, s.poolStart);
    k.shootWpe = pvol_env_shoot_wpe(get);
    k.tileDebugSet = pvol_env_tile_debug(get, &k.tileDebug);
    return k;
}
#endif
