// pvol_map_host.hip -- the two photon maps of a context: the volume map (pvol_upload_photons, or pvol_finish_map behind the
// shooter) and the surface integrator's caustic map (pvol_set_surface_integrator).  Both are a PhotonGrid (pvol_host.h) built by
// build_photon_grid, as are the maps of pvol_compute_radiance (pvol_radiance.hip); what differs -- the first cell size, the volume map's second level -- stays with its caller.  Host code only:
// this unit defines no kernel (the build's kernels are in pvol_grid.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <mutex>
#include <vector>

#include "pvol_host.h"

static GridBuildArgs grid_args(const PhotonGrid &G, const float *const raw[3], const MapFilter &f, int sub) {
    GridBuildArgs g;
    memset(&g, 0, sizeof(g));
    g.p = raw[0]; g.wi = raw[1]; g.alpha = raw[2]; g.n = G.n;
    for (int a = 0; a < 3; ++a) { g.lo[a] = G.gridLo[a]; g.gdim[a] = G.gdim[a]; g.extLo[a] = f.extLo[a]; g.extHi[a] = f.extHi[a]; }
    g.inv = G.invCell;
    g.sub = sub;
    g.volKind = f.volKind;
    memcpy(g.w2v, f.w2v, sizeof(g.w2v));
    return g;
}

// One map from its raw device arrays (pvol_host.h)
int build_photon_grid(PhotonGrid &G, const float *const raw[3], const float *hostP, uint32_t n, double minExt,
                             const std::function<double(double)> &firstCell, const MapFilter &f) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], hostP[3 * i + a]); hi[a] = std::max(hi[a], hostP[3 * i + a]); }
    double ext[3], vol = 1;
    for (int a = 0; a < 3; ++a) { ext[a] = std::max((double)hi[a] - lo[a], minExt); vol *= ext[a]; }
    double cell = firstCell(vol);
    for (;;) {
        double cells = 1;
        for (int a = 0; a < 3; ++a) cells *= floor(ext[a] / cell) + 1;
        if (cells <= 16777216.0) break;
        cell *= 1.26;
    }
    G.n = n;
    G.cellSize = (float)cell;
    G.invCell = 1.f / G.cellSize;
    for (int a = 0; a < 3; ++a) {
        G.gridLo[a] = lo[a];
        G.gdim[a] = (int)floor(ext[a] / cell) + 1;
    }
    if (!G.pos4.alloc(n) || !G.alpha4.alloc(8 * (size_t)n) || !G.wi4.alloc(n) || !G.cellStart.alloc(G.cells() + 1)) return PVOL_E_NO_MEMORY;
    const GridBuildArgs g = grid_args(G, raw, f, 1);
    return ok(pvol_build_grid(&g, G.pos4.get(), G.alpha4.get(), G.wi4.get(), G.cellStart.get(), 0, 0)) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

void pvol_map_to_scene(const PhotonGrid &G, DevScene &h) {
    h.nPhotons = G.n; h.cellSize = G.cellSize; h.invCell = G.invCell;
    for (int a = 0; a < 3; ++a) { h.gridLo[a] = G.gridLo[a]; h.gdim[a] = G.gdim[a]; }
    h.cellStart = G.cellStart.get(); h.subStart = G.subStart.get(); h.pos4 = G.pos4.get(); h.alpha4 = G.alpha4.get(); h.wi4 = G.wi4.get();
    h.mom = G.mom.get();
}

// The moment rows of the volume map G under the scene h (DevScene::mom): h's moment constants and the gate's decision (*terms) are
// set either way; `mom` gets the rows where the gate passes and the map holds photons, and is emptied otherwise.  Runs where the
// map is built and where pvol_set_scene commits a scene over a kept map -- never inside a render or Li call.
int pvol_map_moments(const PhotonGrid &G, DevScene &h, DevPtr<float> &mom, int *terms) {
    MomentWeights w;
    *terms = pvol_moment_scene(h, &w);
    mom.reset();
    if (*terms < 1 || !G.n) return PVOL_OK;
    if (!mom.alloc((size_t)MOM_ROW * G.n)) return PVOL_E_NO_MEMORY;
    if (!ok(pvol_fill_moments(&w, G.alpha4.get(), mom.get(), G.n, 0))) { mom.reset(); return PVOL_E_NO_DEVICE; }
    return PVOL_OK;
}
static void map_to_surface(const PhotonGrid &G, uint32_t nPaths, DevSurfMap &sf) {
    sf.nPhotons = G.n; sf.nPaths = (int32_t)nPaths; sf.cellSize = G.cellSize; sf.invCell = G.invCell;
    for (int a = 0; a < 3; ++a) { sf.gridLo[a] = G.gridLo[a]; sf.gdim[a] = G.gdim[a]; }
    sf.cellStart = G.cellStart.get(); sf.pos4 = G.pos4.get(); sf.alpha4 = G.alpha4.get(); sf.wi4 = G.wi4.get();
}

// A map of the surface integrator from its raw device arrays: cells of maxdist / 2 (a lookup gathers everything within maxdist,
// never fewer), no Inside() filter -- surface photons count wherever they lie
static int build_surface_grid(PhotonGrid &G, const float *const raw[3], const float *hostP, uint32_t n, float maxDist) {
    MapFilter all;
    memset(&all, 0, sizeof(all));
    all.volKind = PVOL_VOLUME_GRID;
    const double first = 0.5 * maxDist;
    return build_photon_grid(G, raw, hostP, n, 1e-3 * maxDist, [first](double) { return first; }, all);
}

static bool all_finite(const float *v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}
// materials: what the scene's surfaces allow -- 0 matte only, 1 glass among them, 2 a kind the surface integrator does not cover
static int scene_materials(const pvol_ctx *c) {
    int m = 0;
    for (size_t i = 0; i < c->triMatHost.size(); ++i) {
        const int kind = c->hsh.mats[c->triMatHost[i]].kind;
        if (kind == PVOL_MATERIAL_GLASS) m = std::max(m, 1);
        else if (kind != PVOL_MATERIAL_MATTE) return 2;
    }
    for (int i = 0; i < c->hs.nSpheres; ++i) {
        const int kind = c->hsh.mats[c->hs.spheres[i].mat].kind;
        if (kind == PVOL_MATERIAL_GLASS) m = std::max(m, 1);
        else if (kind != PVOL_MATERIAL_MATTE) return 2;
    }
    return m;
}

extern "C" {

void pvol_free_photons(pvol_ctx *c) {
    c->dRawP.reset(); c->dRawWi.reset(); c->dRawAlpha.reset();
    c->volMap = PhotonGrid();
    pvol_map_to_scene(c->volMap, c->hs);
}

void pvol_free_caustic_map(pvol_ctx *c) {
    c->causticMap = PhotonGrid();
    c->indirectMap = PhotonGrid();
    memset(&c->hs.surf, 0, sizeof(c->hs.surf));
    c->specOn = false;
}

// The volume map: about 1.4 photons per cell, never more than PVOL_MAX_RING rings per lookup; a clumpy map gets the second level.
int pvol_finish_map(pvol_ctx *c, uint32_t n, const float *hostPositions) {
    DevScene &h = c->hs;
    const float maxDist = c->params.max_dist;
    const float *const raw[3] = {c->dRawP.get(), c->dRawWi.get(), c->dRawAlpha.get()};
    MapFilter f;
    f.volKind = h.volKind;
    memcpy(f.extLo, h.extLo, sizeof(f.extLo)); memcpy(f.extHi, h.extHi, sizeof(f.extHi)); memcpy(f.w2v, h.w2v, sizeof(f.w2v));
    double vol = 0;
    PhotonGrid &G = c->volMap;
    int rc = build_photon_grid(G, raw, hostPositions, n, 1e-3 * maxDist, [&](double boxVolume) {
        vol = boxVolume;
        double cell = cbrt(vol * 1.4 / std::max(1u, n));   // ~1.4 photons per cell measured best on MI355X (profiles/)
        if (c->params.grid_cell_scale > 0.f) cell *= c->params.grid_cell_scale;
        return std::max(cell, (double)maxDist / PVOL_MAX_RING * 1.0001);
    }, f);
    if (rc != PVOL_OK) { pvol_free_photons(c); pvol_push_scene(c); return rc; }
    h.ringMax = (int)ceil(maxDist / G.cellSize);
    if (h.ringMax > PVOL_MAX_RING) h.ringMax = PVOL_MAX_RING;
    if (h.ringMax < 1) h.ringMax = 1;
    // radius^2 of the ball that holds nUsed photons at the map's mean density: where a lookup with nothing better starts
    h.rkEstimate = (float)pow((double)c->params.n_used * vol / ((double)std::max(1u, n) * 4.18879020478639), 2.0 / 3.0);
    // clumpy map (an average photon shares its cell with more than 64 others -- pinkfloyd's beams: 4 700): sort again with
    // the 4 x 4 x 4 second level.  PVOL_SUBGRID=0/1 forces it off/on.
    const size_t ncells = G.cells();
    double sq = 0.0;
    const int forced = pvol_env_subgrid(pvol_env_get);
    bool want = false;
    if (forced >= 0) want = forced != 0;
    else if (ok(pvol_grid_occupancy(G.cellStart.get(), (uint32_t)ncells, &sq, 0))) want = sq / (double)n > 64.0;
    // (no room for the table: the coarse level alone is complete)
    if (want && ncells * 64 < 0xfffffff0ull && G.subStart.alloc(ncells * 64 + 1)) {
        const GridBuildArgs g = grid_args(G, raw, f, 4);
        if (!ok(pvol_build_grid(&g, G.pos4.get(), G.alpha4.get(), G.wi4.get(), G.cellStart.get(), G.subStart.get(), 0))) {
            pvol_free_photons(c); pvol_push_scene(c);
            return PVOL_E_NO_DEVICE;
        }
    }
    rc = pvol_map_moments(G, h, G.mom, &c->momentTerms);
    if (rc != PVOL_OK) { pvol_free_photons(c); pvol_push_scene(c); return rc; }
    pvol_map_to_scene(G, h);
    return pvol_push_scene(c);
}

int pvol_upload_photons(pvol_ctx *c, const float *p, const float *wi, const float *alpha, uint32_t n) {
    if (!c) return PVOL_E_INVALID;
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    if (n && (!p || !wi || !alpha)) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    hipDeviceSynchronize();
    pvol_free_photons(c);
    if (n == 0) return pvol_push_scene(c);
    bool good = c->dRawP.alloc(3 * (size_t)n) && c->dRawWi.alloc(3 * (size_t)n) && c->dRawAlpha.alloc(30 * (size_t)n);
    if (!good) { pvol_free_photons(c); pvol_push_scene(c); return PVOL_E_NO_MEMORY; }
    good = ok(hipMemcpy(c->dRawP.get(), p, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice)) &&
           ok(hipMemcpy(c->dRawWi.get(), wi, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice)) &&
           ok(hipMemcpy(c->dRawAlpha.get(), alpha, sizeof(float) * 30 * (size_t)n, hipMemcpyHostToDevice));
    if (!good) { pvol_free_photons(c); pvol_push_scene(c); return PVOL_E_NO_DEVICE; }
    return pvol_finish_map(c, n, p);
}

// PhotonIntegrator::Li in front of the volume term (include/pvol.h).  The caustic map gets the volume map's cell layout
// (pvol_grid.hip) with cells of about maxdist / 2: a lookup gathers everything within maxdist, never fewer.
int pvol_set_surface_integrator(pvol_ctx *c, const pvol_surface_params *sp, const float *p, const float *wo, const float *alpha, uint32_t n) {
    if (!c) return PVOL_E_INVALID;
    if (!c->haveScene) return PVOL_E_NO_SCENE;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    if (!sp) {
        hipDeviceSynchronize();
        pvol_free_caustic_map(c);
        return pvol_push_scene(c);
    }
    if (sp->n_used < 1 || !(sp->max_dist > 0.f) || sp->max_specular_depth < 0) return PVOL_E_INVALID;
    // matte and glass: a specular BSDF brings the recursion of SpecularReflect / SpecularTransmit (core/integrator.cpp:177-262,
    // pvol_spec_dev.h), walked for "maxspeculardepth" up to SPEC_MAX_DEPTH (the reference's default)
    const int materials = scene_materials(c);
    if (materials == 2) return PVOL_E_UNSUPPORTED;
    const bool anySpecular = materials == 1;
    if (anySpecular && sp->max_specular_depth > SPEC_MAX_DEPTH) return PVOL_E_UNSUPPORTED;
    // an indirect map makes PhotonIntegrator::Li gather: the final gather, or LPhoton(indirectMap) with 144 more rho draws
    // (photonmap.cpp:183-309).  This entry point takes the caustic map alone, so such an integrator is refused by name rather
    // than rendered wrong -- whether the map is the caller's (n_indirect_photons) or the store of the last pvol_preprocess;
    // pvol_set_surface_integrator_maps takes both maps (without the final gather).
    if (sp->n_indirect_photons > 0) return PVOL_E_UNSUPPORTED;
    if (sp->use_preprocess_store) {
        if (!c->surfKept) return PVOL_E_INVALID;   // nothing was kept: params.keep_surface_photons was 0, or no pvol_preprocess yet
        if (c->surf[2].n > 0) return PVOL_E_UNSUPPORTED;
    }
    uint32_t nPaths = sp->n_caustic_paths;
    std::vector<float> hp;
    const float *raw[3] = {0, 0, 0};
    DevPtr<float> up[3];
    if (sp->use_preprocess_store) {   // device to device; the positions come back once for the grid bounds
        const pvol_ctx::SurfStore &st = c->surf[0];
        n = st.n; nPaths = st.nPaths;
        raw[0] = st.p.get(); raw[1] = st.wo.get(); raw[2] = st.alpha.get();
        hp.resize(3 * (size_t)n);
        if (n && !ok(hipMemcpy(hp.data(), raw[0], sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
        p = hp.data();
    } else if (n) {
        if (!p || !wo || !alpha) return PVOL_E_INVALID;
        const size_t width[3] = {3, 3, 30};
        const float *src[3] = {p, wo, alpha};
        for (int i = 0; i < 3; ++i) {
            if (!up[i].alloc(width[i] * (size_t)n)) return PVOL_E_NO_MEMORY;
            if (!ok(hipMemcpy(up[i].get(), src[i], sizeof(float) * width[i] * (size_t)n, hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
            raw[i] = up[i].get();
        }
    }
    if (n && nPaths == 0) return PVOL_E_INVALID;
    hipDeviceSynchronize();
    pvol_free_caustic_map(c);
    if (n) {
        int rc = build_surface_grid(c->causticMap, raw, p, n, sp->max_dist);
        if (rc != PVOL_OK) { pvol_free_caustic_map(c); pvol_push_scene(c); return rc; }
    }
    DevSurface &sf = c->hs.surf;
    sf.enabled = 1; sf.nLookup = sp->n_used; sf.maxSpecularDepth = sp->max_specular_depth;
    c->specOn = anySpecular && sp->max_specular_depth > 1;
    sf.maxDistSq = sp->max_dist * sp->max_dist;   // photonmap.cpp:345-346
    map_to_surface(c->causticMap, nPaths, sf.map[SURF_MAP_CAUSTIC]);
    return pvol_push_scene(c);
}

// Every status of pvol_set_surface_integrator_maps (include/pvol.h) in its one order, a pure function of its arguments: no context, no
// HIP call.  materials: scene_materials() above; storesKept, storeN / storePaths [0] caustic [1] indirect: what the last
// pvol_preprocess* kept; hostPointers: the arrays can be read (their values must be finite).
int pvol_check_surface_maps(const pvol_surface_params *sp, int haveScene, int materials, int storesKept, const uint32_t *storeN,
                            const uint32_t *storePaths, const pvol_photon_array *caustic, const pvol_photon_array *indirect, int hostPointers) {
    if (!sp) return PVOL_E_INVALID;
    if (sp->n_used < 1 || !(sp->max_dist > 0.f) || sp->max_specular_depth < 0) return PVOL_E_INVALID;
    if (materials == 2) return PVOL_E_UNSUPPORTED;
    if (materials == 1 && sp->max_specular_depth > SPEC_MAX_DEPTH) return PVOL_E_UNSUPPORTED;
    if (!haveScene) return PVOL_E_NO_SCENE;
    uint32_t nIndirect = 0;
    if (sp->use_preprocess_store) {
        if (caustic || indirect || !storesKept || !storeN || !storePaths) return PVOL_E_INVALID;
        for (int m = 0; m < 2; ++m) if (storeN[m] > 0 && storePaths[m] == 0) return PVOL_E_INVALID;
        nIndirect = storeN[1];
    } else {
        const pvol_photon_array *maps[2] = {caustic, indirect};
        for (int m = 0; m < 2; ++m) {
            const pvol_photon_array *M = maps[m];
            if (!M || !M->n) continue;
            if (!M->p || !M->wi || !M->alpha || !M->n_paths) return PVOL_E_INVALID;
            if (hostPointers && (!all_finite(M->p, 3 * (size_t)M->n) || !all_finite(M->wi, 3 * (size_t)M->n) || !all_finite(M->alpha, 30 * (size_t)M->n)))
                return PVOL_E_INVALID;
        }
        nIndirect = indirect ? indirect->n : 0u;
    }
    // LPhoton(indirectMap) is the branch WITHOUT the final gather (photonmap.cpp:183, :307-309); the gather itself is not built
    if (sp->final_gather != 0 && nIndirect > 0) return PVOL_E_UNSUPPORTED;
    return PVOL_OK;
}

// PhotonIntegrator with both maps of its LPhoton calls (include/pvol.h).  Both grids are built aside and committed last: a
// rejected call leaves the integrator as it was.
int pvol_set_surface_integrator_maps(pvol_ctx *c, const pvol_surface_params *sp, const pvol_photon_array *caustic, const pvol_photon_array *indirect) {
    if (!c) return PVOL_E_INVALID;
    std::lock_guard<std::recursive_mutex> api(c->apiMu);
    const uint32_t storeN[2] = {c->surf[0].n, c->surf[2].n}, storePaths[2] = {c->surf[0].nPaths, c->surf[2].nPaths};
    int rc = pvol_check_surface_maps(sp, c->haveScene, scene_materials(c), c->surfKept, storeN, storePaths, caustic, indirect, 1);
    if (rc != PVOL_OK) return rc;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const pvol_photon_array *arrays[2] = {caustic, indirect};
    const int storeKind[2] = {0, 2};
    PhotonGrid grid[2];
    uint32_t nPaths[2] = {0, 0};
    for (int m = 0; m < 2; ++m) {
        std::vector<float> hp;
        const float *raw[3] = {0, 0, 0}, *hostP = 0;
        DevPtr<float> up[3];
        uint32_t n = 0;
        if (sp->use_preprocess_store) {   // device to device; the positions come back once for the grid bounds
            const pvol_ctx::SurfStore &st = c->surf[storeKind[m]];
            n = st.n; nPaths[m] = st.nPaths;
            raw[0] = st.p.get(); raw[1] = st.wo.get(); raw[2] = st.alpha.get();
            hp.resize(3 * (size_t)n);
            if (n && !ok(hipMemcpy(hp.data(), raw[0], sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost))) return PVOL_E_NO_DEVICE;
            hostP = hp.data();
        } else if (arrays[m] && arrays[m]->n) {
            n = arrays[m]->n; nPaths[m] = arrays[m]->n_paths;
            const size_t width[3] = {3, 3, 30};
            const float *src[3] = {arrays[m]->p, arrays[m]->wi, arrays[m]->alpha};
            for (int i = 0; i < 3; ++i) {
                if (!up[i].alloc(width[i] * (size_t)n)) return PVOL_E_NO_MEMORY;
                if (!ok(hipMemcpy(up[i].get(), src[i], sizeof(float) * width[i] * (size_t)n, hipMemcpyHostToDevice))) return PVOL_E_NO_DEVICE;
                raw[i] = up[i].get();
            }
            hostP = arrays[m]->p;
        }
        if (!n) continue;
        rc = build_surface_grid(grid[m], raw, hostP, n, sp->max_dist);
        if (rc != PVOL_OK) return rc;
        if (!ok(hipDeviceSynchronize())) return PVOL_E_NO_DEVICE;   // the build has read `up` and the stores
    }
    hipDeviceSynchronize();   // an earlier batch may still read the maps replaced here
    const int materials = scene_materials(c);
    c->causticMap = std::move(grid[0]);
    c->indirectMap = std::move(grid[1]);
    DevSurface &sf = c->hs.surf;
    memset(&sf, 0, sizeof(sf));
    sf.enabled = 1; sf.nLookup = sp->n_used; sf.maxSpecularDepth = sp->max_specular_depth;
    c->specOn = materials == 1 && sp->max_specular_depth > 1;
    sf.maxDistSq = sp->max_dist * sp->max_dist;   // photonmap.cpp:345-346
    map_to_surface(c->causticMap, nPaths[0], sf.map[SURF_MAP_CAUSTIC]);
    map_to_surface(c->indirectMap, nPaths[1], sf.map[SURF_MAP_INDIRECT]);
    return pvol_push_scene(c);
}

int pvol_photon_count(pvol_ctx *c, uint32_t *n) {
    if (!c || !n) return PVOL_E_INVALID;
    *n = c->volMap.n;
    return PVOL_OK;
}

int pvol_download_photons(pvol_ctx *c, float *p, float *wi, float *alpha, uint32_t capacity) {
    if (!c || !p || !wi || !alpha) return PVOL_E_INVALID;
    uint32_t n = std::min(capacity, c->volMap.n);
    if (!n) return PVOL_OK;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    bool good = ok(hipMemcpy(p, c->dRawP.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                ok(hipMemcpy(wi, c->dRawWi.get(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost)) &&
                ok(hipMemcpy(alpha, c->dRawAlpha.get(), sizeof(float) * 30 * (size_t)n, hipMemcpyDeviceToHost));
    return good ? PVOL_OK : PVOL_E_NO_DEVICE;
}

}  // extern "C"
