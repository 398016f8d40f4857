/*
 * pvol.h -- C ABI of the MI355X-native volumetric photon-mapping hot path.
 *
 * This is the drop-in boundary for ONE path of the pbrt-v2 fork piwell/CS348B-pbrt:
 *   core/photonshooter.cpp   (volume-photon shooting, PhotonShooter::Preprocess)
 *   integrators/photonvolume.cpp (PhotonVolumeIntegrator::Li / Transmittance / LPhoton)
 * Every entry point below names the reference interface (file:line under the reference
 * tree) it replaces.  Plain pointers and sizes only; no C++/torch types.  All functions
 * return PVOL_OK (0) or a negative pvol_status; they never abort, never print, and fail
 * loudly (PVOL_E_NO_DEVICE) instead of falling back to a CPU path when no HIP device
 * is usable.
 *
 * Conventions
 *   - Spectra are 30 fp32 bins, 400..700 nm (core/spectrum.h:44-46).  The two tag floats
 *     of the reference's 128-byte Spectrum are not carried: `lambda` is re-derived by
 *     extractLambda() (core/spectrum.h:266-279), `intensity` is never read on the path.
 *   - Matrices are row-major 4x4, m[r*4+c] == Transform::m.m[r][c] (core/transform.h).
 *   - One MT19937 stream per render tile (renderers/samplerrenderer.cpp:73).  A batch
 *     groups rays by stream; rays of one stream are consumed in array order, exactly as
 *     the reference's tile loop consumes its RNG.
 */
#ifndef PVOL_H
#define PVOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVOL_NBINS 30
#define PVOL_MT_N 624
#define PVOL_ABI_VERSION 3

typedef enum pvol_status {
    PVOL_OK = 0,
    PVOL_E_INVALID = -1,      /* bad argument / inconsistent sizes            */
    PVOL_E_NO_DEVICE = -2,    /* no usable HIP device / HIP runtime error     */
    PVOL_E_NO_SCENE = -3,     /* pvol_set_scene has not succeeded yet         */
    PVOL_E_NO_MEMORY = -4,
    PVOL_E_UNSUPPORTED = -5,  /* volume/light/material kind out of scope      */
    PVOL_E_LIMIT = -6,        /* a ray needs more march steps than the kernel's LDS plan */
    PVOL_E_SHOOT_FAILED = -7  /* "Unable to store enough photons" (photonshooter.cpp:285-299) */
} pvol_status;

typedef struct pvol_spectrum { float c[PVOL_NBINS]; } pvol_spectrum;

/* ---- scene: a flattened POD copy of what the path reads from Scene ------------------ */

typedef enum pvol_volume_kind {
    PVOL_VOLUME_NONE = 0,
    PVOL_VOLUME_HOMOGENEOUS = 1,  /* volumes/homogeneous.h:43-89 */
    PVOL_VOLUME_GRID = 2,         /* volumes/volumegrid.{h,cpp}  */
    PVOL_VOLUME_RAINBOW = 3,      /* volumes/rainbow.{h,cpp} (homogeneous + rainbowReflection) */
    PVOL_VOLUME_EXPONENTIAL = 4   /* volumes/exponential.h:43-68 (density a * expf(-b * height) inside the extent) */
} pvol_volume_kind;

typedef struct pvol_volume {
    int32_t kind;
    float extent_min[3], extent_max[3]; /* BBox extent in volume space                   */
    float world_to_volume[16];          /* WorldToVolume.m                               */
    float volume_to_world[16];          /* its inverse (WorldBound: homogeneous.h:57-59) */
    pvol_spectrum sigma_a, sigma_s, le;
    float g;                            /* HG asymmetry (core/volume.cpp:150-154)        */
    int32_t nx, ny, nz;                 /* grid only                                     */
    const float *density;               /* grid: nx*ny*nz floats, x fastest (volumegrid.h:60-65).  exponential: 5 floats
                                           {a, b, updir.x, updir.y, updir.z} with nx = ny = nz = 0; updir is as the scene
                                           file gives it, pvol_set_scene normalises it as Normalize() does (exponential.h:51)
                                           and answers PVOL_E_INVALID for NULL, a non-finite value or a zero-length updir */
} pvol_volume;

typedef enum pvol_light_kind {
    PVOL_LIGHT_POINT = 0,   /* lights/point.cpp   */
    PVOL_LIGHT_SPOT = 1,    /* lights/spot.cpp    */
    PVOL_LIGHT_DISTANT = 2  /* lights/distant.cpp */
} pvol_light_kind;

typedef struct pvol_light {
    int32_t kind;
    float pos[3];               /* lightPos (point, spot)                                 */
    float dir[3];               /* lightDir, already normalised (distant)                 */
    float light_to_world[16];
    float world_to_light[16];
    pvol_spectrum intensity;    /* I (point, spot) or L (distant)                         */
    float cos_total_width;      /* spot.cpp:45                                            */
    float cos_falloff_start;    /* spot.cpp:46                                            */
} pvol_light;

typedef enum pvol_material_kind {
    PVOL_MATERIAL_MATTE = 0,  /* materials/matte.cpp:42-63, sigma == 0 => Lambertian      */
    PVOL_MATERIAL_GLASS = 1   /* materials/glass.cpp:42-59 + dispersive SpecularTransmission */
} pvol_material_kind;

typedef struct pvol_material {
    int32_t kind;
    pvol_spectrum kd;   /* matte: Kd (already clamped >= 0)                               */
    pvol_spectrum kr;   /* glass: Kr                                                      */
    pvol_spectrum kt;   /* glass: Kt                                                      */
    float ior;          /* glass "index"                                                  */
    float vn;           /* glass Abbe number; > 0 => dispersive (materials/glass.h:57)    */
} pvol_material;

typedef struct pvol_triangle {
    float p[3][3];          /* world-space vertices p1,p2,p3 (shapes/trianglemesh.cpp:70-71) */
    int32_t material;       /* index into materials[]                                     */
    int32_t flip_normal;    /* ReverseOrientation ^ TransformSwapsHandedness (core/diffgeom.cpp:52-53) */
} pvol_triangle;

/* Shape "sphere" (shapes/sphere.cpp), intersected analytically in object space exactly as Sphere::Intersect / IntersectP do
 * (:59-157, :160-216); the fields are what the Sphere constructor stores (:41-49).  At most 8 per scene. */
typedef struct pvol_sphere {
    float object_to_world[16];  /* ObjectToWorld.m                                            */
    float world_to_object[16];  /* WorldToObject.m                                            */
    float radius;
    float z_min, z_max;         /* clamped to [-radius, radius] and ordered                   */
    float theta_min, theta_max; /* acosf(Clamp(z/radius, -1, 1)) of z_min, z_max              */
    float phi_max;              /* radians                                                    */
    int32_t material;           /* index into materials[]                                     */
    int32_t flip_normal;        /* ReverseOrientation ^ TransformSwapsHandedness              */
} pvol_sphere;

typedef struct pvol_scene {
    pvol_volume volume;
    uint32_t n_lights;
    const pvol_light *lights;
    uint32_t n_triangles;
    const pvol_triangle *triangles;
    uint32_t n_materials;
    const pvol_material *materials;
    float world_min[3], world_max[3];  /* Scene::WorldBound(): geometry U volume (core/scene.cpp:59-60) */
    pvol_spectrum cie_x, cie_y, cie_z; /* SampledSpectrum::X/Y/Z bin averages (core/spectrum.h:370-381) */
    float xyz_scale;                   /* (700-400)/(CIE_Y_integral*30)  (core/spectrum.h:427-428)     */
    uint32_t n_spheres;                /* ABI 3 */
    const pvol_sphere *spheres;
} pvol_scene;

/* ---- integrator / shooter parameters (CreatePhotonVolumeIntegrator photonvolume.cpp:224-229,
 *      CreatePhotonShooter photonshooter.cpp:529-548) ---------------------------------- */
typedef struct pvol_params {
    float step_size;            /* VolumeIntegrator "stepsize"  (default 1)               */
    int32_t n_used;             /* VolumeIntegrator "nused"     (default 250)             */
    float max_dist;             /* VolumeIntegrator "maxdist"   (default 0.1)             */
    uint32_t n_volume_photons;  /* VolumeIntegrator "volumephotons" (default 0)           */
    float shooter_step_size;    /* SurfaceIntegrator "stepsize" (default 0.1)             */
    int32_t max_photon_depth;   /* SurfaceIntegrator "maxphotondepth" (default 5)         */
    uint32_t n_caustic_photons; /* SurfaceIntegrator "causticphotons" (default 20000)     */
    uint32_t n_indirect_photons;/* SurfaceIntegrator "indirectphotons" (default 10000)    */
    int32_t final_gather;       /* SurfaceIntegrator "finalgather" (default true)         */
    int32_t device;             /* HIP device ordinal                                     */
    float grid_cell_scale;      /* 0 = auto; else photon-grid cell edge as a multiple of the auto choice */
    uint32_t keep_surface_photons; /* 1: pvol_preprocess also KEEPS the caustic / direct / indirect / radiance photons it deposits
                                      (photonshooter.cpp:148-189); 0: they are only counted (their counts steer the shooting)   */
    uint32_t reserved[6];
} pvol_params;

/* ---- ray batches --------------------------------------------------------------------- */

/* One camera ray handed to Li() (PhotonVolumeIntegrator::Li, photonvolume.cpp:112-222). */
typedef struct pvol_ray {
    float o[3];
    float mint;
    float d[3];
    float maxt;
    float time;
    float scatter_u;   /* sample->oneD[scatterSampleOffset][0]  (photonvolume.cpp:135)   */
    uint32_t rng_skip; /* draws of this ray's stream the CALLER consumed since the previous
                          ray of the stream (sampler + surface integrator), skipped before Li */
    uint32_t flags;    /* reserved, 0                                                     */
} pvol_ray;            /* 48 bytes                                                        */

/* One MT19937 stream == one render tile (samplerrenderer.cpp:73 `RNG rng(taskNum)`).     */
typedef struct pvol_stream {
    uint32_t seed;        /* RNG(seed)                                                    */
    uint32_t first_ray;   /* rays [first_ray, first_ray+n_rays) of the batch, in order    */
    uint32_t n_rays;
    uint32_t reserved;
    uint64_t start_draw;  /* RandomUInt() calls already made on this stream before the batch */
    uint64_t end_draw;    /* OUT: calls made after the last ray of the batch               */
} pvol_stream;            /* 32 bytes                                                     */

typedef enum pvol_output_kind {
    PVOL_OUT_SPECTRAL = 0, /* per ray: Lv[30] then T[30]          (60 floats)             */
    PVOL_OUT_XYZ = 1       /* per ray: Lv as X,Y,Z then T.y()     (4 floats)              */
} pvol_output_kind;

typedef struct pvol_stats {
    uint64_t n_rays;           /* Li() calls                                              */
    uint64_t n_steps;          /* march steps == photon lookups (non-rainbow)             */
    uint64_t n_tested;         /* photons distance-tested by the gather                   */
    uint64_t n_kept;           /* photons that entered a flux sum                         */
    uint64_t n_lookups_lt10;   /* lookups that found < 10 photons (photonvolume.cpp:83)   */
    uint64_t n_shadow_unoccluded;
    uint64_t n_guess_retries;  /* lookups redone exactly: predicted radius held < k photons (lphoton), or not served by the bucket plan (group kernel) */
    uint64_t cy_search;        /* s_memtime cycles summed over wavefronts: candidate search ...          */
    uint64_t cy_select;        /* ... k-selection ...                                                     */
    uint64_t cy_flux;          /* ... flux sum ...                                                        */
    uint64_t cy_total;         /* ... whole kernel                                                        */
    uint64_t group_guess_failed;  /* li_group_kernel: lookups whose guessed search radius was too small or too large ...   */
    uint64_t group_plan_skipped;  /* ... whose shared photon bucket overflowed (or k outside the plan) ...                 */
    uint64_t cy_fallback;         /* ... and the cycles of li_fixup_kernel, whose exact wave-cooperative lookups serve what the plan handed over (n_guess_retries counts them) */
    uint64_t group_deferred_overflow;  /* handed-over lookups whose last attempt ended in a bucket overflow ...                */
    uint64_t group_deferred_too_few;   /* ... or found fewer than k photons inside a radius below the maximum                  */
    uint64_t group_attempts;           /* shared-bucket attempts (stagings), per wavefront                                     */
} pvol_stats;

/* ---- tile driver, SURVEY 8(f)-1: the caller of Li() (LD sampler, perspective camera) and its
 * consumer (image film) on the device, so that a whole SamplerRendererTask (renderers/
 * samplerrenderer.cpp:59-157) runs without leaving HBM.  Surface radiance is NOT computed here: the
 * driver is exact for renders whose surface integrator adds nothing and draws nothing (Ls = Lvi). ---- */
#define PVOL_MAX_SAMPLE_ARRAYS 16
#define PVOL_FILTER_TABLE_SIZE 16
#define PVOL_MAX_PIXEL_SAMPLES 1024

typedef struct pvol_camera {     /* PerspectiveCamera (cameras/perspective.cpp:41-49, core/camera.cpp:83-102) */
    float raster_to_camera[16];  /* ProjectiveCamera::RasterToCamera.m, row-major                 */
    float camera_to_world[16];   /* Camera::CameraToWorld of a static camera (startTransform->m)  */
    float shutter_open, shutter_close;
    float lens_radius;           /* must be 0 (pinhole); the lens samples are still drawn          */
    float focal_distance;
} pvol_camera;

typedef struct pvol_film {       /* ImageFilm (film/image.cpp:37-75); its crop window travels apart, as a pvol_film_window */
    int32_t x_resolution, y_resolution;
    float filter_xwidth, filter_ywidth;              /* Filter::xWidth, yWidth                     */
    float filter_table[PVOL_FILTER_TABLE_SIZE * PVOL_FILTER_TABLE_SIZE];  /* ImageFilm::filterTable */
} pvol_film;

/* ImageFilm's film image extent (film/image.cpp:48-51): the pixels [x_pixel_start, x_pixel_start + x_pixel_count) x
 * [y_pixel_start, y_pixel_start + y_pixel_count) of the frame are the ones the film stores (:54), splats into (:86-89, :121) and
 * writes (:179-219).  Taken by the *_window entry points; a NULL window there is the whole frame (crop 0 1 0 1), which is what
 * the entry points without a window render.  Valid: starts >= 0, counts > 0, inside the resolution. */
typedef struct pvol_film_window {
    int32_t x_pixel_start, y_pixel_start;
    int32_t x_pixel_count, y_pixel_count;
} pvol_film_window;

typedef struct pvol_sampler {    /* LDSampler (samplers/lowdiscrepancy.cpp:40-80) + the Sample layout  */
    int32_t x_start, x_end, y_start, y_end;          /* Film::GetSampleExtent (film/image.cpp:157-166) */
    uint32_t pixel_samples;                          /* power of two, <= PVOL_MAX_PIXEL_SAMPLES    */
    uint32_t n_tasks;                                /* taskCount of SamplerRenderer::Render (samplerrenderer.cpp:206-208) */
    uint32_t n1d_count, n2d_count;                   /* Sample::n1D / n2D as the integrators requested them */
    uint32_t n1d[PVOL_MAX_SAMPLE_ARRAYS], n2d[PVOL_MAX_SAMPLE_ARRAYS];
    uint32_t tau_index, scatter_index;               /* positions in n1d of tauSampleOffset / scatterSampleOffset (photonvolume.cpp:9-13) */
} pvol_sampler;

typedef struct pvol_render_debug {   /* optional DEVICE buffers that receive the intermediate records, sized for all samples of the call */
    pvol_ray *d_rays;            /* camera rays after Scene::Intersect clipped maxt, tile-major    */
    float *d_image_xy;           /* 2 floats per sample: CameraSample::imageX, imageY              */
    float *d_xyz;                /* 4 floats per sample: Lvi as X,Y,Z and T.y()                    */
    pvol_stream *d_streams;      /* one per task of the call, end_draw filled                      */
    float *d_surf_xyz;           /* 3 floats per sample: the surface integrator's Li as X,Y,Z      */
                                 /* (only with pvol_set_surface_integrator enabled; may be NULL)   */
} pvol_render_debug;

/* Surface integrator in front of the volume term: PhotonIntegrator::Li
 * (integrators/photonmap.cpp:154-319) for camera rays that end on MATTE surfaces, without an indirect
 * map (`indirectphotons 0`, both BASELINE scenes) or with one and `finalgather false`
 * (pvol_set_surface_integrator_maps): UniformSampleAllLights over delta lights
 * (core/integrator.cpp:47-79, :117-174), the estimate LPhoton (photonmap.cpp:62-108) over each map and the
 * RNG traffic of the rest of that Li() (2 x BSDF::rho, 2 x BSDFSample, one draw per unoccluded light). */
typedef struct pvol_surface_params {
    int32_t n_used;              /* "nused" (photonmap.cpp:340), lookup size of the caustic estimate */
    float max_dist;              /* "maxdist" (photonmap.cpp:345)                                    */
    int32_t max_specular_depth;  /* "maxspeculardepth" (photonmap.cpp:341): > 1 costs 6 draws per hit */
    int32_t final_gather;        /* "finalgather": without an indirect map it changes nothing              */
    uint32_t n_caustic_paths;    /* nCausticPaths (photonshooter.cpp:215) of the map passed along    */
    int32_t use_preprocess_store;/* 1: take the caustic photons (and path count) the last pvol_preprocess kept
                                    (params.keep_surface_photons) instead of the arrays passed        */
    uint32_t n_indirect_photons; /* photons in the integrator's INDIRECT map (0 with `indirectphotons 0`, both BASELINE
                                    scenes).  > 0 makes Li() gather (photonmap.cpp:183-309): pvol_set_surface_integrator,
                                    which takes the caustic map alone, answers PVOL_E_UNSUPPORTED.
                                    pvol_set_surface_integrator_maps takes the indirect map itself and does not read this */
    uint32_t reserved[1];
} pvol_surface_params;

typedef struct pvol_ctx pvol_ctx;

/* Version of this ABI (PVOL_ABI_VERSION). */
int pvol_abi_version(void);
/* Static string for a pvol_status. */
const char *pvol_strerror(int status);
/* Number of usable HIP devices (0 when none; never a CPU fallback). */
int pvol_device_count(void);

/* Fill *p with the reference defaults (photonvolume.cpp:224-229, photonshooter.cpp:529-548). */
void pvol_default_params(pvol_params *p);

/* Replaces CreatePhotonVolumeIntegrator + CreatePhotonShooter (photonvolume.cpp:224-229,
 * photonshooter.cpp:529-548; constructed from core/api.cpp:572-586,1225-1230). */
int pvol_create(const pvol_params *params, pvol_ctx **out);
/* Replaces ~PhotonShooter / ~PhotonVolumeIntegrator (photonshooter.cpp:423-430). */
void pvol_destroy(pvol_ctx *ctx);

/* Copies the flattened scene to the device (what Li()/followPhoton read through
 * `const Scene *`: core/scene.h:42-73) and, beyond 64 triangles, builds the triangle hierarchy there (pvol_get_accel_info).
 * May be called again to replace the scene; a rejected scene leaves the previous one in place.
 * Limits (PVOL_E_UNSUPPORTED): 8 lights, 2^24 triangles, 8 spheres, 8 materials; PVOL_E_INVALID: a material index out of
 * range, a non-finite vertex, a sphere radius <= 0. */
int pvol_set_scene(pvol_ctx *ctx, const pvol_scene *scene);

/* Per-vertex shading normals of the scene's triangles (`"normal N"` of a trianglemesh; Triangle::GetShadingGeometry,
 * shapes/trianglemesh.cpp:293-368, with the default uvs): n holds 9 * n_triangles floats, the three vertex normals of every triangle
 * in the scene's triangle order and in the triangle's vertex order, in WORLD space (Transform::operator()(const Normal&) of the mesh's
 * ObjectToWorld applied to each, not normalised).  A triangle whose nine values are all zero has no shading normals.  Call it after
 * pvol_set_scene; NULL with n_triangles 0 clears the normals, and pvol_set_scene clears them too (as it disables the surface
 * integrator).  PVOL_E_NO_SCENE without a scene; PVOL_E_INVALID for a count that differs from the scene's or a non-finite value; a
 * rejected call changes nothing.  Sphere hits are untouched. */
int pvol_set_triangle_normals(pvol_ctx *ctx, const float *n, uint32_t n_triangles);

/* Installs a volume photon map computed elsewhere (e.g. by the reference's own
 * PhotonShooter) and builds the device search structure; replaces
 * `volumeMap = new KdTree<Photon>(volumePhotons)` (photonshooter.cpp:502-503).
 * p, wi: 3*n floats (xyz interleaved); alpha: 30*n floats.  n == 0 clears the map
 * (a NULL map is legal, photonvolume.cpp:69). */
int pvol_upload_photons(pvol_ctx *ctx, const float *p, const float *wi,
                        const float *alpha, uint32_t n);

/* Replaces PhotonShooter::Preprocess (photonshooter.cpp:457-526): shoots volume photons
 * on the device with `n_tasks` virtual PhotonShootingTasks (task t uses RNG(31*t) and its
 * own Halton permutation, photonshooter.cpp:235,243), merges them in task order per block
 * round (photonshooter.cpp:280-351) and builds the search structure. */
int pvol_preprocess(pvol_ctx *ctx, uint32_t n_tasks);

/* The same with `block_paths` (1 .. 4096) paths per virtual task and round instead of PhotonShootingTask::Run's 4096
 * (photonshooter.cpp:247): the merge rule is unchanged (task order per round, volume photons divided by the running nshot,
 * :280-351), only finer.  What it is for: a store stops growing at the first merge that fills it, so what is stored overshoots
 * the request by up to one round = n_tasks x block_paths paths' worth of photons -- with 4096-path blocks a prism scene cannot
 * use more than a few hundred tasks (C3: 256 waves on a 1024-SIMD chip, and still 6.7 M stored for 4 M asked); with small blocks
 * thousands of tasks keep the chip busy at the same overshoot.  Not the reference's block size, hence not its photon set:
 * statistically the same map (tests/test_gpu_shooter.py: counts, flux, spatial and spectral histograms), and still equal to the
 * oracle photon for photon when the oracle runs the same block size. */
int pvol_preprocess_blocks(pvol_ctx *ctx, uint32_t n_tasks, uint32_t block_paths);

/* How the ranks of a sharded shoot (pvol_preprocess_ranks) exchange data.  Exactly one of the two is set:
 * nccl_comm, an ncclComm_t of n_ranks ranks made by the caller with RCCL (ncclCommInitRank), whose ncclAllGather moves device
 * buffers on the null stream; or allgather, a host all-gather: every rank passes `bytes` bytes at `send` and receives
 * n_ranks x bytes at `recv`, rank-major, returning 0 on success (for gloo or a test's own transport).  `user` is handed to it. */
typedef struct pvol_shoot_comm {
    void *nccl_comm;
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
    void *user;
} pvol_shoot_comm;

/* pvol_preprocess_blocks sharded over n_ranks ranks (one GPU each): rank `rank` shoots only the virtual tasks
 * pvol_partition_tasks(n_tasks, rank, n_ranks) deals it (task t keeps RNG(31*t) and its Halton permutation wherever it runs).
 * Each round the ranks all-gather one count row per task and a status word per rank, and every rank runs the single-rank merge
 * rule on the gathered table; after the last round one all-gather of every rank's taken rows per store places them where
 * pvol_preprocess_blocks puts them.  Every rank ends with the same photon map (and, with keep_surface_photons, the same surface
 * stores) as pvol_preprocess_blocks(ctx, n_tasks, block_paths) on one GPU, bit for bit, and the same pvol_get_shoot_stats.
 * All ranks call it with the same scene, parameters, n_tasks and block_paths; n_ranks = 1 runs the whole protocol too.
 * A rank's own failure (PVOL_E_NO_MEMORY, PVOL_E_LIMIT: a block outgrew the largest pool, PVOL_E_NO_DEVICE) is reported at the
 * next exchange and every rank returns the lowest-ranked rank's code, so no rank is left waiting in a collective; only a failed
 * exchange itself (PVOL_E_NO_DEVICE) can leave the ranks disagreeing.  PVOL_E_INVALID: a NULL ctx or comm, rank >= n_ranks,
 * n_tasks or block_paths out of pvol_preprocess_blocks' range, or not exactly one of nccl_comm and allgather set (all checked
 * before the device is touched).  RCCL is bound at run time as for pvol_render_frame_ranks, and only when nccl_comm is given. */
int pvol_preprocess_ranks(pvol_ctx *ctx, uint32_t n_tasks, uint32_t block_paths, uint32_t rank, uint32_t n_ranks,
                          const pvol_shoot_comm *comm);

/* Seconds the last pvol_preprocess_ranks spent in its all-gathers, host staging included (part of the shooting time that
 * pvol_get_preprocess_seconds reports in out[0]).  0.0 after a single-rank shoot (pvol_preprocess, pvol_preprocess_blocks),
 * which exchanges nothing. */
int pvol_get_exchange_seconds(pvol_ctx *ctx, double *out);

/* Work counters of the last pvol_preprocess (the figures SURVEY 6 reports for the reference shooter):
 * out[12] = paths, followPhoton calls, calls ending without a surface hit, transmittance-march steps,
 * volume interactions, absorbed, stored volume / caustic / direct / indirect photons, spectral-split
 * children, nshot. */
int pvol_get_shoot_stats(pvol_ctx *ctx, uint64_t *out12);

/* Wall-clock seconds of the last pvol_preprocess: out[0] the shooting rounds and merges
 * (PhotonShootingTask::Run, photonshooter.cpp:232-357), out[1] the device search-structure build that replaces
 * the kd-tree construction (photonshooter.cpp:502-503, core/kdtree.h:100-147). */
int pvol_get_preprocess_seconds(pvol_ctx *ctx, double *out2);

/* The triangle accelerator of the scene set last (replaces CreateBVHAccelerator / `new BVHAccel`, core/api.cpp:1284-1290,
 * accelerators/bvh.cpp:301-389): scenes of up to 64 triangles are scanned linearly out of the scalar cache; larger ones
 * (up to 2^24 triangles) get a linear BVH built on the device inside pvol_set_scene.  Closest / any hit results do not
 * depend on which one serves them (smallest t; of several triangles at the same t the one latest in the scene's order).
 * out[0] = triangles in the hierarchy (0: linear scan), out[1] = device build time in milliseconds. */
int pvol_get_accel_info(pvol_ctx *ctx, double *out2);

/* The surface stores of the last pvol_preprocess (params.keep_surface_photons = 1): what PhotonShooter::Preprocess hands to
 * its caustic / direct / indirect kd-trees (photonshooter.cpp:495-503), in the reference's merge order (:303-327).
 * kind: 0 caustic, 1 direct, 2 indirect.  n_paths = nCausticPaths / nDirectPaths / nIndirectPaths.  p, wo: 3 floats,
 * alpha: 30 floats per photon (NOT divided by the path count: the surface estimate divides at lookup, photonmap.cpp:89). */
int pvol_surface_photon_count(pvol_ctx *ctx, int kind, uint32_t *n, uint32_t *n_paths);
int pvol_download_surface_photons(pvol_ctx *ctx, int kind, float *p, float *wo, float *alpha, uint32_t capacity);
/* Radiance photons (photonshooter.cpp:182-189): position, normal facing the arriving photon, rho_r, rho_t (30 floats each). */
int pvol_radiance_photon_count(pvol_ctx *ctx, uint32_t *n);
int pvol_download_radiance_photons(pvol_ctx *ctx, float *p, float *n, float *rho_r, float *rho_t, uint32_t capacity);

/* ---- radiance photons: the tail of PhotonShooter::Preprocess with `finalgather` (photonshooter.cpp:505-524) ----
 * ComputeRadianceTask::Run (photonshooter.cpp:359-395) gives every radiance photon Lo = INV_PI rho_r E(n) + INV_PI rho_t E(-n), E the
 * sum of three k-NN irradiance estimates EPhoton (:17-35; PhotonProcess, photonshooter.h:186-203; the visit test of
 * core/kdtree.h:180) over the direct, indirect and caustic maps, and the photons become radianceMap, which the final gather asks for
 * the nearest photon facing a point (RadiancePhotonProcess, photonshooter.h:63-78; integrators/photonmap.cpp:226-230).  Nothing
 * else calls these: pvol_preprocess* does not compute radiance, and the final gather that asks radianceMap exists as entry points
 * of its own (pvol_gather_* and pvol_final_gather* below) and inside pvol_radiance_gather_batch*, the caller-ray path; the tile
 * driver does not gather: pvol_set_surface_integrator_maps still refuses `finalgather` with an indirect map. */
typedef struct pvol_photon_array {   /* host arrays: p, wi 3 floats, alpha 30 floats per photon */
    const float *p, *wi, *alpha; uint32_t n; uint32_t n_paths;
} pvol_photon_array;

/* ComputeRadianceTask over the stores the last pvol_preprocess* kept (keep_surface_photons):
   direct + indirect + caustic maps, the kept radiance photons, rho_r = Kd of the photon's matte material,
   rho_t = 0 (as pvol_download_radiance_photons reports them).  n_lookup / max_dist are the SURFACE
   integrator's "nused" / "maxdist" (CreatePhotonShooter, photonshooter.cpp:534,543).
   PVOL_E_INVALID: NULL ctx, n_lookup < 1, max_dist not > 0 or not finite, no kept stores; PVOL_E_UNSUPPORTED: n_lookup > 576.
   Zero radiance photons is PVOL_OK with count 0.  A rejected call changes nothing; a second compute replaces the first; every
   new shoot drops the result. */
int pvol_compute_radiance(pvol_ctx *ctx, int32_t n_lookup, float max_dist);

/* The same from the caller's arrays (maps computed elsewhere, as pvol_upload_photons allows for the volume map).
   maps[0] caustic, maps[1] direct, maps[2] indirect (the `kind` order of pvol_surface_photon_count);
   a NULL entry or n == 0 is EPhoton's `if (!map) return 0`.  Needs no scene.  rp_p, rp_n: 3 floats, rho_r, rho_t: 30 floats per
   radiance photon.  Also PVOL_E_INVALID: a NULL array with a count > 0, a map with n > 0 and n_paths == 0, a non-finite value. */
int pvol_compute_radiance_arrays(pvol_ctx *ctx, int32_t n_lookup, float max_dist, const pvol_photon_array *const maps[3],
                                 const float *rp_p, const float *rp_n, const float *rho_r, const float *rho_t, uint32_t n_rp);

int pvol_radiance_lo_count(pvol_ctx *ctx, uint32_t *n);            /* 0 until one of the two above succeeded */
int pvol_download_radiance_lo(pvol_ctx *ctx, float *p, float *n, float *lo, uint32_t capacity);  /* input order; lo 30 floats */

/* radianceMap->Lookup(p, RadiancePhotonProcess(n), INFINITY): the nearest radiance photon with Dot(rp.n, n) > 0, no radius
   limit.  lo: 30 floats per query (that photon's Lo; zeros when none), found: 1 / 0.  PVOL_E_INVALID before any compute.  The
   device form takes DEVICE pointers and is enqueued on `hip_stream` without synchronising. */
int pvol_radiance_lookup(pvol_ctx *ctx, const float *p, const float *n, uint32_t count, float *lo, uint32_t *found);
int pvol_radiance_lookup_device(pvol_ctx *ctx, const float *d_p, const float *d_n, uint32_t count, float *d_lo,
                                uint32_t *d_found, void *hip_stream);

/* ---- final gather, sampling half: what PhotonIntegrator::Li does between `if (finalGather && indirectMap != NULL)` and the moment a
 * gather ray is traced (integrators/photonmap.cpp:183-219, :248-265), and the weight each ray carries (:233-243, :280-291) ----
 * The gather map is the indirect map as the reference's own kd-tree (KdTree<Photon>::KdTree, core/kdtree.h:99-147), because the
 * photon-sampled loop picks photonDirs[j] by its PLACE in the heap PhotonProcess leaves (core/photonshooter.h:186-203), and that
 * place depends on the tree's visiting order (kdtree.h:157-183).  Results are exact, ties included: CompareNode breaks a
 * coordinate tie by the photon's index in the store, ClosePhoton::operator< a distance tie by the node number, and the heap
 * routines leave libstdc++'s layout.
 *
 * Statuses, decided in this one order (pvol_check_gather):
 *   1. PVOL_E_INVALID      NULL ctx
 *   builds:
 *   2. PVOL_E_INVALID      pvol_build_gather_map without kept stores; _arrays: NULL `indirect`, NULL p or wi with n > 0, a
 *                          non-finite p or wi (a non-finite position in the kept store is answered the same way, once the
 *                          store has been read back)
 *   3. PVOL_E_UNSUPPORTED  fewer than 50 photons (photonmap.cpp:194-199 does not terminate on such a map) or more than 2^24
 *   lookups:
 *   2. PVOL_E_INVALID      max_dist not > 0, not finite, or so small that max_dist^2 is 0 in fp32 (the doubling would never leave
 *                          it); n_samples outside 1..256; cos_gather_angle not inside (-1, 1); a NULL array with count > 0
 *   3. PVOL_E_INVALID      no gather map built
 *   then PVOL_E_NO_DEVICE / PVOL_E_NO_MEMORY from the device, as everywhere.
 * A rejected call changes nothing; a second build replaces the first; whatever drops the radiance result above (a new shoot,
 * freeing the kept stores) drops the map too. */

/* Replaces `new KdTree<Photon>(indirectPhotons)` (photonshooter.cpp:502) for the gather: from the indirect store (kind 2) the last
   pvol_preprocess* kept. */
int pvol_build_gather_map(pvol_ctx *ctx);
/* The same from the caller's host arrays (p and wi are read, alpha and n_paths are not); needs no scene. */
int pvol_build_gather_map_arrays(pvol_ctx *ctx, const pvol_photon_array *indirect);
int pvol_gather_map_count(pvol_ctx *ctx, uint32_t *n);   /* 0 until a build succeeded */

/* Replaces photonmap.cpp:189-199: per query point p (3 floats) the loop `md2 = searchDist2; nFound = 0; Lookup(p, proc, md2);
   searchDist2 *= 2` from searchDist2 = max_dist^2 until 50 photons are found.  index: 50 per query, the photons' indices in the
   store's order, in the order of proc.photons[]; d2: their squared distances; found: 50, or fewer when even a round over the whole
   map (md2 = +inf) did not hold 50 -- a non-finite query, a d^2 that overflows; the tail of index and d2 is then zero and the call
   still returns PVOL_OK; rounds: Lookup calls made.  The device form takes DEVICE pointers and is enqueued on `hip_stream` without
   synchronising. */
int pvol_gather_photons(pvol_ctx *ctx, const float *p, uint32_t count, float max_dist, uint32_t *index, float *d2, uint32_t *found,
                        uint32_t *rounds);
int pvol_gather_photons_device(pvol_ctx *ctx, const float *d_p, uint32_t count, float max_dist, uint32_t *d_index, float *d_d2,
                               uint32_t *d_found, uint32_t *d_rounds, void *hip_stream);

/* One gather ray as either loop samples it.  weight: what multiplies fr * Lindir in the sum (AbsDot(wi, n) * wt / pdf; neither
   fr = Kd INV_PI nor Lindir is multiplied in); photon_index: the store index of photonDirs[photonNum] in the photon loop,
   0xffffffff in the BSDF loop; valid 0: the reference `continue`s (pdf == 0 or fr black), wi, weight and the pdfs are then 0. */
typedef struct pvol_gather_sample {
    float wi[3], weight, bsdf_pdf, photon_pdf; uint32_t photon_index, valid;
} pvol_gather_sample;

/* Replaces photonmap.cpp:189-219 and :248-265 with the weights of :233-243 and :280-291, for a BSDF of one Lambertian lobe: the
   lookup above, then n_samples BSDF-sampled and n_samples photon-sampled gather rays per query.  frames: 9 floats per query,
   dgShading.nn, dgShading.dpdu, ng (the frame is built as BSDF::BSDF does, core/reflection.cpp:619-627); wo: 3 floats;
   u_bsdf, u_photon: per query and sample uComponent, uDir[0], uDir[1] in [0, 1); cos_gather_angle: PhotonShooter's
   cosGatherAngle (photonshooter.cpp:413).  out_bsdf, out_photon: n_samples records per query.  A query whose lookup found fewer
   than 50 gets invalid records. */
int pvol_gather_directions(pvol_ctx *ctx, const float *p, const float *frames, const float *wo, uint32_t count, float max_dist,
                           int32_t n_samples, float cos_gather_angle, const float *u_bsdf, const float *u_photon,
                           pvol_gather_sample *out_bsdf, pvol_gather_sample *out_photon);
int pvol_gather_directions_device(pvol_ctx *ctx, const float *d_p, const float *d_frames, const float *d_wo, uint32_t count,
                                  float max_dist, int32_t n_samples, float cos_gather_angle, const float *d_u_bsdf,
                                  const float *d_u_photon, pvol_gather_sample *d_out_bsdf, pvol_gather_sample *d_out_photon,
                                  void *hip_stream);

/* ---- final gather, tracing half: what PhotonIntegrator::Li does with every gather ray of both loops from the construction of
 * bounceRay to `L += Li / gatherSamples` (integrators/photonmap.cpp:219-231, :243-246, :265-278, :291-295), on top of the
 * sampling half above.  Per query point p (the dgShading.p of a Lambertian hit) and per valid sample of pvol_gather_directions:
 * the ray (p, wi, mint = ray_eps, maxt = +inf) meets the scene (Scene::Intersect: any primitive counts, glass too; a miss
 * contributes nothing and draws nothing); nGather = Faceforward(dg.nn, -wi) with the GEOMETRIC normal; Lindir is the Lo of
 * radianceMap->Lookup(hit point, RadiancePhotonProcess(nGather), INFINITY) -- the walk of pvol_radiance_lookup -- or 0 when no
 * photon faces; Lindir *= Transmittance over [ray_eps, t_hit], which draws one RandomFloat per ray that hits exactly when the scene
 * has a volume region, and for a homogeneous medium is exp(-sigma_t |p(t0) - p(t1)|) whatever was drawn
 * (volumes/homogeneous.h:78-82).  Then
 *     L = sum_bsdf (Kd INV_PI) Lindir weight / n_samples + sum_photon (Kd INV_PI) Lindir weight / n_samples,
 * each loop summed in sample order; draws counts the RandomFloat calls.  A query whose Kd is black in every bin, or whose lookup
 * found fewer than 50 photons, gives L = 0 and zero draws with nothing traced.  pvol_radiance_gather_batch* calls this at every
 * Lambertian hit of the caller's rays; the tile driver does not: pvol_set_surface_integrator_maps still refuses `finalgather` with
 * an indirect map.
 *
 * Statuses, decided in this one order (pvol_check_final_gather):
 *   1. PVOL_E_INVALID      NULL ctx
 *   2. PVOL_E_INVALID      the argument faults of pvol_gather_directions; a NULL kd, ray_eps, L or draws with count > 0
 *   3. PVOL_E_NO_SCENE
 *   4. PVOL_E_UNSUPPORTED  the scene's medium is a density region (VolumeGrid, exponential), as behind the surface integrator
 *   5. PVOL_E_INVALID      no gather map built
 *   6. PVOL_E_INVALID      no radiance result, or one with zero radiance photons (the reference's lookup on an empty tree is
 *                          undefined)
 *   then PVOL_E_NO_DEVICE / PVOL_E_NO_MEMORY from the device.  A rejected call writes nothing. */

/* One traced gather ray.  All zero for an invalid sample and for every sample of a dead query; a valid ray that misses has hit 0,
   radiance_index 0xffffffff and the rest zero. */
typedef struct pvol_gather_ray {      /* 32 bytes; one per query, loop and sample */
    float t, n_gather[3];             /* the hit's ray parameter; Faceforward(dg.nn, -wi) */
    uint32_t radiance_index;          /* the radiance photon found, in the input order of the radiance photons
                                         (pvol_download_radiance_lo); 0xffffffff: none faces */
    int32_t prim;                     /* triangle index in upload order, -1 - i for sphere i */
    uint32_t hit, drew;               /* 1 / 0; RandomFloat calls of this ray's Transmittance (0 or 1) */
} pvol_gather_ray;

/* Queries are walked in slices so that the per-ray scratch (a direction record and a ray record, 64 bytes) stays within this
   bound; the scratch belongs to the context. */
#define PVOL_FINAL_GATHER_SCRATCH_BYTES (256ull << 20)

/* p, frames, wo, max_dist, cos_gather_angle, u_bsdf, u_photon: exactly as for pvol_gather_directions.  kd: 30 floats per query
   (the Lambertian's R); ray_eps: isect.rayEpsilon per query; n_samples: gatherSamples after RequestSamples has halved and rounded
   it.  L: 30 floats, draws: one count per query.  rays_bsdf, rays_photon: n_samples records per query, optional (NULL: not
   reported).  The host form holds the context from upload to copy-back; the device form takes DEVICE pointers, is enqueued on
   `hip_stream` and not synchronised. */
int pvol_final_gather(pvol_ctx *ctx, const float *p, const float *frames, const float *wo, const float *kd, const float *ray_eps,
                      uint32_t count, float max_dist, int32_t n_samples, float cos_gather_angle, const float *u_bsdf,
                      const float *u_photon, float *L, uint32_t *draws, pvol_gather_ray *rays_bsdf, pvol_gather_ray *rays_photon);
int pvol_final_gather_device(pvol_ctx *ctx, const float *d_p, const float *d_frames, const float *d_wo, const float *d_kd,
                             const float *d_ray_eps, uint32_t count, float max_dist, int32_t n_samples, float cos_gather_angle,
                             const float *d_u_bsdf, const float *d_u_photon, float *d_L, uint32_t *d_draws,
                             pvol_gather_ray *d_rays_bsdf, pvol_gather_ray *d_rays_photon, void *hip_stream);

/* ---- LPhoton at explicit points
 * PhotonVolumeIntegrator::LPhoton (integrators/photonvolume.cpp:65-108) on the current volume map, with the context's n_used and
 * max_dist, at n points the caller names: the k-nearest-photon estimate of the in-scattered radiance the march evaluates at every
 * step.  p, w: n x 3 floats, world space; w is the direction LPhoton is given (the phase function is p(photon.p, photon.wi, -w))
 * and may be NULL only when the medium's g is 0.  out: n x 30 floats (PVOL_OUT_SPECTRAL), or n x 4 (PVOL_OUT_XYZ): X, Y, Z of
 * the CIE projection, then 0.  n_found (optional): proc.nFound = min(n_used, photons with dist^2 < max_dist^2).  radius2
 * (optional): the reference's maxmd, the largest fp32 DistanceSquared among the kept photons, 0 when none was kept.  Both are
 * written even where n_found < 10 and out is therefore zero (photonvolume.cpp:83-84).  sigma_s is taken at the point: zero
 * outside a homogeneous (or rainbow) extent, density x sigma_s in a VolumeGrid or exponential region; out is zero where it is
 * black.  Results are in the caller's order; there are no atomics: two runs agree byte for byte, and a point's bytes do not depend
 * on which other points share the call.  n == 0 does nothing.  The points are walked in slices whose ordering scratch (16 bytes a
 * point, the context's) stays within PVOL_LPHOTON_SCRATCH_BYTES; PVOL_LPHOTON_NO_SORT=1 (read at pvol_create) serves the points in
 * the caller's order instead of by grid cell, with the same bytes.
 *
 * Statuses, decided in this one order (pvol_check_lphoton):
 *   1. PVOL_E_INVALID      NULL ctx
 *   2. PVOL_E_INVALID      an unknown output_kind; with n > 0: a NULL p or out, or a NULL w under a medium with g != 0
 *   3. PVOL_E_NO_SCENE
 *   then PVOL_E_NO_DEVICE / PVOL_E_NO_MEMORY from the device.  No map, or an empty one: PVOL_OK and zeros everywhere.  A rejected
 *   call writes nothing.
 * The host form holds the context from upload to copy-back; the device form takes DEVICE pointers, is enqueued on `hip_stream`
 * and not synchronised. */
#define PVOL_LPHOTON_SCRATCH_BYTES (64ull << 20)
int pvol_lphoton_batch(pvol_ctx *ctx, const float *p, const float *w, uint32_t n, int output_kind, float *out, uint32_t *n_found,
                       float *radius2);
int pvol_lphoton_batch_device(pvol_ctx *ctx, const float *d_p, const float *d_w, uint32_t n, int output_kind, float *d_out,
                              uint32_t *d_n_found, float *d_radius2, void *hip_stream);

/* Number of photons in the current volume map. */
int pvol_photon_count(pvol_ctx *ctx, uint32_t *n);
/* Copies the current map back (same layout as pvol_upload_photons); capacity in photons. */
int pvol_download_photons(pvol_ctx *ctx, float *p, float *wi, float *alpha, uint32_t capacity);

/* Replaces PhotonVolumeIntegrator::Li (photonvolume.cpp:112-222) for a batch of rays
 * grouped into MT19937 streams.  Host pointers; `out` has n_rays*60 (SPECTRAL) or
 * n_rays*4 (XYZ) floats; `draws` (optional) receives per ray the number of RandomUInt
 * calls Li() made (4+6n+n+r+u).  streams[i].end_draw is written.
 * The streams must partition the ray array in order: streams[0].first_ray == 0 and
 * streams[i+1].first_ray == streams[i].first_ray + streams[i].n_rays (PVOL_E_INVALID otherwise). */
int pvol_li_batch(pvol_ctx *ctx, const pvol_ray *rays, uint32_t n_rays,
                  pvol_stream *streams, uint32_t n_streams,
                  int output_kind, float *out, uint32_t *draws);

/* Same, all pointers are DEVICE pointers and the work is enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream) without synchronising. */
int pvol_li_batch_device(pvol_ctx *ctx, const pvol_ray *d_rays, uint32_t n_rays,
                         pvol_stream *d_streams, uint32_t n_streams,
                         int output_kind, float *d_out, uint32_t *d_draws,
                         void *hip_stream);

/* ---- full radiance for rays the caller generated
 * SamplerRenderer::Li (renderers/samplerrenderer.cpp:228-251, :95-97) per ray of the batch, in its stream's order, for a caller with
 * its own camera and sampler (pvol_render_tasks_device insists on LDSampler and a pinhole PerspectiveCamera):
 *   1. Scene::Intersect over [mint, maxt] (:236): with a hit at t <= maxt, maxt becomes t; without one Ls = 0 and nothing is drawn.
 *   2. No surface integrator described (pvol_set_surface_integrator*), or one switched off: Ls = 0, nothing is drawn at the hit, and
 *      the result is pvol_li_batch's on the clipped ray, for every medium.
 *   3. Surface integrator on: PhotonIntegrator::Li at the hit (integrators/photonmap.cpp:154-319) as pvol_render_tasks_device runs it --
 *      matte: direct light + LPhoton(caustic) + LPhoton(indirect, `finalgather false`), their BSDF::rho draws, one draw per unoccluded
 *      light sample under a medium, 6 for the two absent lobes; glass: SpecularReflect + SpecularTransmit (core/integrator.cpp:177-262),
 *      3 draws each, the spawned ray through these same steps at depth + 1 on the parent's scatter_u and time, in post-order, before the
 *      parent's own volume Li().
 *   4. L = T (.) Ls + Lvi and T, T the ray's own volume transmittance (PhotonVolumeIntegrator::Li, photonvolume.cpp:112-222).
 * rays[i].rng_skip is what the CALLER drew since the previous ray of the stream (its sampler); the surface integrator's draws are this
 * entry point's business.  streams[].end_draw is written as pvol_li_batch writes it.
 *
 * Statuses, decided in this one order (pvol_radiance_batch_check):
 *   1. PVOL_E_INVALID      NULL ctx
 *   2. PVOL_E_INVALID      an unknown output_kind
 *   3. PVOL_E_INVALID      NULL rays with n_rays > 0, NULL streams with n_streams > 0
 *   4. PVOL_E_INVALID      NULL out, or NULL out->L, with n_rays > 0
 *   5. PVOL_E_NO_SCENE
 *   6. PVOL_E_UNSUPPORTED  a surface integrator that is on over a density region (VolumeGrid, exponential): the shadow rays'
 *                          transmittance there needs drawn values, as pvol_render_tasks_device refuses it
 *   then PVOL_E_INVALID for streams that do not partition the rays in order (as pvol_li_batch; the device form reads its table back
 *   to see), and PVOL_E_NO_DEVICE / PVOL_E_NO_MEMORY from the device.  A rejected call writes nothing; n_rays == 0 or n_streams == 0
 *   does nothing and returns PVOL_OK.
 * The rays are walked in slices whose scratch (the context's) stays within PVOL_RADIANCE_SCRATCH_BYTES: 324 bytes per ray and spawned
 * ray, 248 per ray.  A slice is sized for rays that spawn nothing, its spawned rays are counted, and it is cut back to the longest
 * run of its rays that fits (never fewer than one ray); it may end inside a stream, which the next slice continues.  No atomics of
 * its own and no pool that can overflow. */
#define PVOL_RADIANCE_SCRATCH_BYTES (256ull << 20)
typedef struct pvol_radiance_out {   /* host arrays in the host form, device arrays in the device form; all but L optional (NULL) */
    float    *L;           /* per ray, pvol_output_kind's layout: T (.) Ls + Lvi, then T (Spectrum Li, *T of samplerrenderer.cpp:228)    */
    float    *surf_xyz;    /* 3 per ray: Ls as X, Y, Z (what pvol_render_debug.d_surf_xyz reports)                                       */
    float    *t_hit;       /* per ray: maxt after the clip (ray.maxt behind Scene::Intersect, samplerrenderer.cpp:236)                   */
    uint32_t *draws;       /* per ray: RandomUInt calls of the ray's own volume Li(), as pvol_li_batch                                   */
    uint32_t *surf_draws;  /* per ray: calls made for it before that Li(), the caller's rng_skip excluded -- the surface integrator at   */
                           /* the hit, every spawned ray's surface draws and volume Li()                                                 */
    uint32_t *n_segments;  /* per ray: rays the specular recursion spawned (core/integrator.cpp:198, :243)                               */
} pvol_radiance_out;
/* Host pointers; holds the context from upload to copy-back and checks the device's error flag (pvol_check_errors) itself. */
int pvol_radiance_batch(pvol_ctx *ctx, const pvol_ray *rays, uint32_t n_rays, pvol_stream *streams, uint32_t n_streams, int output_kind,
                        const pvol_radiance_out *out);
/* All arrays (the members of *out too; *out itself is host memory) are DEVICE pointers; the work is enqueued on `hip_stream`.  That
 * stream is synchronised once to read the stream table back and twice per slice (the slice's expanded size comes back, its stream
 * table goes up; pvol_li_batch_device synchronises it likewise where it sizes a slice); the kernels of the last slice are left in flight. */
int pvol_radiance_batch_device(pvol_ctx *ctx, const pvol_ray *d_rays, uint32_t n_rays, pvol_stream *d_streams, uint32_t n_streams,
                               int output_kind, const pvol_radiance_out *out, void *hip_stream);

/* ---- ... with the final gather
 * pvol_radiance_batch* with the final-gather branch of PhotonIntegrator::Li (integrators/photonmap.cpp:183-296) at every Lambertian
 * hit of every member of a ray's block -- the ray itself and every ray the specular recursion spawns for it, as the reference's
 * recursion evaluates it.  Everything is as steps 1 to 4 above; at a matte hit with a non-black Kd, in addition:
 *   query   p = the hit point, frame = the shading nn, dpdu and the geometric normal, wo = -d of the member, kd the material's,
 *           ray_eps the hit's: one query of pvol_final_gather
 *   samples u_bsdf, u_photon per CALLER ray and sample (uComponent, uDir[0], uDir[1]); every member of a ray's block reads its caller
 *           ray's rows, because spawned rays see the same Sample (core/integrator.cpp:198, :243)
 *   value   Lg and its draws are what pvol_final_gather_device returns for that query with max_dist, n_samples and cos_gather_angle
 *           passed on unchanged
 *   sum     Ls_matte becomes Ls_matte + Lg before T (.) Ls is formed; surf_xyz includes the gather
 *   stream  the gather's draws (one per gather ray that hits, only under a medium) come after the hit's other surface draws and before
 *           that member's own volume Li(); surf_draws includes them and streams[].end_draw moves accordingly
 * The reference evaluates either the gather or LPhoton(indirectMap), never both (:183, :307): the surface integrator must be on and
 * must describe NO indirect map (pvol_set_surface_integrator, or pvol_set_surface_integrator_maps with an empty indirect array), so
 * no indirect LPhoton and none of its 2 x 72 rho draws happen.  A matte hit with a black Kd, a glass hit, a miss and a query whose
 * lookup finds fewer than 50 photons add nothing and draw nothing.  pvol_set_surface_integrator_maps still refuses `finalgather`
 * with an indirect map, and the tile driver (pvol_render_tasks*) does not gather.
 *
 * Statuses, decided in this one order (pvol_radiance_gather_check):
 *   1. items 1 to 4 of pvol_radiance_batch's list, for the same arguments
 *   2. PVOL_E_INVALID      NULL gather; the argument faults of pvol_gather_directions (max_dist, n_samples, cos_gather_angle; a NULL
 *                          u_bsdf or u_photon with n_rays > 0)
 *   3. PVOL_E_NO_SCENE
 *   4. PVOL_E_UNSUPPORTED  the scene's medium is a density region
 *   5. PVOL_E_INVALID      no surface integrator is on
 *   6. PVOL_E_INVALID      the surface integrator describes a non-empty indirect map
 *   7. PVOL_E_INVALID      no gather map built
 *   8. PVOL_E_INVALID      no radiance result, or one with zero radiance photons
 *   then the stream-partition fault and the device's own codes, as for pvol_radiance_batch.  A rejected call writes nothing; n_rays == 0
 *   or n_streams == 0 does nothing and returns PVOL_OK.
 * A slice's scratch, the queries included (308 + 24 n_samples bytes per ray and spawned ray on top of pvol_radiance_batch's), stays
 * within PVOL_RADIANCE_SCRATCH_BYTES; pvol_final_gather_device's own bound and slices apply inside.  No atomics: two runs agree byte
 * for byte. */
typedef struct pvol_gather_params {
    float max_dist;                  /* the gather lookup's first radius, as for pvol_gather_directions                      */
    int32_t n_samples;               /* gatherSamples after RequestSamples has halved and rounded it, 1..256                */
    float cos_gather_angle;          /* PhotonShooter's cosGatherAngle, inside (-1, 1)                                      */
    const float *u_bsdf, *u_photon;  /* n_rays x n_samples x 3 floats each; host arrays in the host form, device in the other */
} pvol_gather_params;
typedef struct pvol_radiance_gather_out {   /* pvol_radiance_out's members in their order, then: */
    float    *L, *surf_xyz, *t_hit;
    uint32_t *draws, *surf_draws, *n_segments;
    uint32_t *gather_draws;  /* per ray (optional): the gather's RandomFloat calls, summed over the ray's block; part of surf_draws */
} pvol_radiance_gather_out;
int pvol_radiance_gather_batch(pvol_ctx *ctx, const pvol_ray *rays, uint32_t n_rays, pvol_stream *streams, uint32_t n_streams,
                               int output_kind, const pvol_gather_params *gather, const pvol_radiance_gather_out *out);
/* Device arrays throughout (u_bsdf, u_photon and the members of *out too; *gather and *out themselves are host memory); synchronises
 * `hip_stream` as pvol_radiance_batch_device does. */
int pvol_radiance_gather_batch_device(pvol_ctx *ctx, const pvol_ray *d_rays, uint32_t n_rays, pvol_stream *d_streams, uint32_t n_streams,
                                      int output_kind, const pvol_gather_params *gather, const pvol_radiance_gather_out *out,
                                      void *hip_stream);

/* Device-side error flags of the batches enqueued so far (pvol_li_batch_device, pvol_render_tasks_device): waits
 * for the device and returns PVOL_E_LIMIT if a ray needed more march steps than the kernels' record/LDS plan holds
 * (such a ray's output is zero, never a guess), clearing the flag.  The host entry points check this themselves. */
int pvol_check_errors(pvol_ctx *ctx);

/* Single call with the caller's live RNG (the per-sample shim behind
 * VolumeIntegrator::Li): mt[624] / *mti are core/rng.h:57-58 narrowed to 32 bits and are
 * advanced exactly as the reference would advance them.  Lv, T: 30 floats each.
 * Thread-safe: concurrent calls on one context (every SamplerRendererTask thread calls
 * VolumeIntegrator::Li, samplerrenderer.cpp:247) are serialised inside the library, as are all
 * other host-pointer entry points. */
int pvol_li(pvol_ctx *ctx, const pvol_ray *ray, uint32_t *mt, int32_t *mti,
            float *Lv, float *T);

/* n independent pvol_li calls in one device batch: ray i with its own live state mt[i*624..],
 * mti[i] (advanced in place), Lv / T: n x 30 floats.  Every call's results are the bytes a lone
 * pvol_li gives on the same input, whatever the other calls of the batch.  The batch runs after
 * the context's device work still in flight (pvol_li_batch_device, pvol_render_tasks_device on
 * any stream, and whatever runs on the default stream).  status (optional):
 * one PVOL_* code per call, its outputs and state are written only where it is PVOL_OK.  Returns
 * PVOL_OK or the first non-OK code in call order; PVOL_E_INVALID (nothing run) for a NULL
 * array or an mti outside 0..624.  n == 0 does nothing. */
int pvol_li_many(pvol_ctx *ctx, const pvol_ray *rays, uint32_t n, uint32_t *mt, int32_t *mti,
                 float *Lv, float *T, int32_t *status);

/* Coalescing of concurrent pvol_li calls on one context.  max_batch <= 1 (the default): every
 * call is its own batch, serialised.  Otherwise calls made at the same time queue, and whenever
 * no batch is in flight one of them sends up to max_batch queued calls as one pvol_li_many batch;
 * an idle sender waits up to max_wait_us for more callers first.  Results are unchanged.
 * PVOL_E_INVALID: max_batch > 4096 or max_wait_us > 1000.  At pvol_create the environment
 * variable PVOL_LI_COALESCE=<max_batch> sets the default (wait 0). */
int pvol_set_li_coalescing(pvol_ctx *ctx, uint32_t max_batch, uint32_t max_wait_us);
/* out6 (since creation or the last reset): calls served through coalesced batches, coalesced
 * batches, largest coalesced batch, calls that queued while a batch was in flight; then, over
 * every batch of pvol_li_many and the coalescer: batches redone call by call because the
 * hand-over backup fired (each call then runs as a lone pvol_li), calls that failed on their own
 * (PVOL_E_LIMIT: such a call's error is its own, it never reaches pvol_check_errors). */
int pvol_get_li_coalescing_stats(pvol_ctx *ctx, uint64_t *out6, int reset);

/* Replaces PhotonVolumeIntegrator::Transmittance with sample == NULL
 * (photonvolume.cpp:15-30): step = 4*stepSize, offset = one RandomFloat per ray.
 * Rays are grouped into streams like pvol_li_batch; out: 30 floats per ray. */
int pvol_transmittance_batch(pvol_ctx *ctx, const pvol_ray *rays, uint32_t n_rays,
                             pvol_stream *streams, uint32_t n_streams, float *out);

/* Which VolumeIntegrator the context's Li() is (core/api.cpp:575-581).  PVOL_VOLINT_PHOTON, the default at pvol_create:
 * PhotonVolumeIntegrator::Li (photonvolume.cpp:112-222).  PVOL_VOLINT_SINGLE: SingleScatteringIntegrator::Li (single.cpp:66-139) --
 * the same march, light samples and RNG traffic, Tr accumulated over the steps, Lv += Tr Lve + Tr sigma_s p Ld nLights / pdf, no
 * photon map (one that is uploaded stays and is ignored).  The setter waits for the context's work in flight and uploads nothing.
 * PVOL_E_INVALID: a NULL argument or an unknown kind.
 * Under SINGLE: pvol_li_batch, pvol_li_batch_device, pvol_li and pvol_li_many are served with every medium but the rainbow, any
 * number of lights and the roulette; pvol_transmittance_batch is the same function under both integrators.  The render driver
 * (pvol_render_tasks*_device, the rank and group frames) and pvol_radiance_batch* are served within one limit: at most one light, a
 * homogeneous extent or no medium in which no ray can reach the roulette (the extent's world-space diagonal times the largest
 * sigma_t below 6.8), no specular material under the surface integrator.  PVOL_E_UNSUPPORTED, before anything is launched or
 * written: a rainbow medium; everything beyond that limit in the render driver and pvol_radiance_batch*;
 * pvol_radiance_gather_batch*, whatever else the call is (its other checks come behind this one). */
#define PVOL_VOLINT_PHOTON 0
#define PVOL_VOLINT_SINGLE 1
int pvol_set_volume_integrator(pvol_ctx *ctx, int kind);
int pvol_get_volume_integrator(pvol_ctx *ctx, int *kind);

/* Work counters accumulated since the last reset (feeds the algorithmic-bytes formula
 * B_lookup = 20*V + 132*K of SURVEY 8(d)). */
int pvol_get_stats(pvol_ctx *ctx, pvol_stats *out, int reset);
/* Enable/disable counter collection in the kernels (off by default: atomics cost time). */
int pvol_enable_stats(pvol_ctx *ctx, int on);

/* Average device time of the dominant (march+gather) kernel over the launches since
 * the last reset, measured with HIP events on the launch stream. */
int pvol_kernel_time_ms(pvol_ctx *ctx, double *avg_ms, uint64_t *launches, int reset);
/* Name of the march+gather kernel the last batch was dispatched to ("li_group_kernel", "li_par_kernel",
 * "li_replay_kernel", "li_seq_kernel"; under PVOL_VOLINT_SINGLE "single_par_kernel", "single_seq_kernel"; "" before the first batch): the
 * kernel the time above belongs to. */
const char *pvol_march_kernel_name(pvol_ctx *ctx);
/* Form of the tile pre-pass the context's last pvol_render_tasks_device batch that ran one actually launched: "tile_kernel<count>",
 * "tile_kernel<fused>", "tile_mw_kernel<2>", "<4>", "<8>" or "<16>" (the multi-wave COUNT form; a requested wave count is rounded down
 * to one of these, and sliced launches take the one-wave kernel whatever was asked); "" before the first. */
const char *pvol_tile_kernel_name(pvol_ctx *ctx);
/* Which of its two compilations that launch was: "plain" (COUNT mode over a homogeneous extent lit by a distant first light, at most 64
 * triangles, no spheres, no surface integrator: the tests of all of these compiled out) or "general" (everything else, and every scene
 * with PVOL_TILE_GENERAL=1 in the environment when the context was created).  Both give the same rays and stream ends bit for bit. */
const char *pvol_tile_form_name(pvol_ctx *ctx);

/* Per-phase device time of pvol_render_tasks_device, HIP events on the launch stream (off by default).  out[6], milliseconds
 * summed since the last reset: [0] tile pre-pass (LDSampler + camera + Scene::Intersect clip + draw count: tile_kernel),
 * [1] unused, [2] march + gather (li_group_kernel and its hand-over passes, or the slice loop incl. its RNG pass),
 * [3] surface integrator, [4] ImageFilm::AddSample, [5] unused.  What one rank of a multi-GPU render spends where
 * (bench.py --emulate-rank). */
int pvol_enable_phase_timing(pvol_ctx *ctx, int on);
int pvol_get_phase_ms(pvol_ctx *ctx, double *out6, int reset);

/* GaussianFilter::Evaluate tabulated as ImageFilm's constructor does (filters/gaussian.h:44-58,
 * film/image.cpp:57-68). */
void pvol_gaussian_filter_table(float xwidth, float ywidth, float alpha, float *table256);

/* Sampler::ComputeSubWindow (core/sampler.cpp:55-74) for task `task` of s->n_tasks: out = x0,x1,y0,y1. */
void pvol_compute_sub_window(const pvol_sampler *s, uint32_t task, int32_t out[4]);

/* Total camera samples of the given tasks (pixels of the sub-windows x pixel_samples). */
uint64_t pvol_render_sample_count(const pvol_sampler *s, const uint32_t *task_ids, uint32_t n_task_ids);

/* Runs SamplerRendererTask::Run (samplerrenderer.cpp:59-157) for the listed tasks: per task RNG(taskNum),
 * LDSampler::GetMoreSamples -> LDPixelSample per pixel, PerspectiveCamera::GenerateRayDifferential,
 * Scene::Intersect (clips the ray), PhotonVolumeIntegrator::Li, ImageFilm::AddSample.  d_pixels holds
 * x_resolution*y_resolution*4 floats (Lxyz[3], weightSum as ImageFilm::Pixel) and is ACCUMULATED into,
 * so ranks that render disjoint task sets sum their buffers (RCCL all-reduce) before pvol_film_resolve.
 * Enqueued on hip_stream; work buffers live in the context. */
int pvol_render_tasks_device(pvol_ctx *ctx, const pvol_camera *camera, const pvol_film *film,
                             const pvol_sampler *sampler, const uint32_t *task_ids, uint32_t n_task_ids,
                             float *d_pixels, const pvol_render_debug *debug, void *hip_stream);

/* Enables (sp != NULL) or disables (sp == NULL) the surface integrator for pvol_render_tasks_device:
 * SamplerRendererTask::Run then computes Ls = surface Li, and the film receives T * Ls + Lvi
 * (samplerrenderer.cpp:95-97,239-251).  p/wo/alpha: the caustic map's n photons (p 3, wo 3, alpha 30
 * floats each; n == 0: no caustic map, as when the shooter stored no caustic photon).
 * Media covered: none, homogeneous and rainbow, at any nused and Henyey-Greenstein g, with or without a volume photon
 * map, with any number of lights, and dense enough for the Russian roulette (T is the last march step's Tr, doubled by a
 * survival, 0 after a kill: photonvolume.cpp:150-160).  Glass (the specular recursion, maxspeculardepth <= 5) composes
 * its T the same way.
 * PVOL_E_UNSUPPORTED: a triangle of the scene carries a material other than matte or glass, maxspeculardepth > 5 with
 * glass present, or an indirect photon map exists (sp->n_indirect_photons > 0, or use_preprocess_store and the shooter kept
 * indirect photons) (here); a VolumeGrid medium, whose T is a product of stepped taus with drawn offsets, or glass in a
 * medium dense enough for the roulette (from pvol_render_tasks_device).  PVOL_E_INVALID:
 * use_preprocess_store without a pvol_preprocess that ran with params.keep_surface_photons.  pvol_set_scene disables the
 * surface integrator again.  This entry point describes an integrator WITHOUT an indirect map: it drops one that
 * pvol_set_surface_integrator_maps set, whether it enables or disables. */
int pvol_set_surface_integrator(pvol_ctx *ctx, const pvol_surface_params *sp, const float *p, const float *wo,
                                const float *alpha, uint32_t n);

/* PhotonIntegrator with both maps LPhoton reads (photonmap.cpp:179-180, :307-309): the caustic estimate and, WITHOUT the final
 * gather, the same estimate over the indirect map with nIndirectPaths in its norm and 2 x 72 more BSDF::rho draws per
 * Lambertian hit.  pvol_photon_array::wi is Photon::wi (the `wo` of pvol_set_surface_integrator).  A NULL array or n == 0:
 * no such map (LPhoton's `if (map && ...)`).  sp->use_preprocess_store = 1: both arrays must be NULL; the caustic map is store 0
 * and the indirect map store 2 of the last pvol_preprocess*, each with its own path count, copied device to device.
 * sp->n_caustic_paths and sp->n_indirect_photons are not read: the arrays or stores carry them.
 * Statuses, the first that applies: PVOL_E_INVALID a NULL ctx or sp, n_used < 1, max_dist not > 0, max_specular_depth < 0;
 * PVOL_E_UNSUPPORTED a material other than matte or glass, maxspeculardepth > 5 with glass; PVOL_E_NO_SCENE;
 * PVOL_E_INVALID an array with n > 0 and a NULL pointer or n_paths == 0, a non-finite value, use_preprocess_store together
 * with an array or without kept stores; PVOL_E_UNSUPPORTED sp->final_gather != 0 with a non-empty indirect map (the final
 * gather, photonmap.cpp:183-306, is not built).  With an empty indirect map final_gather changes nothing and the call equals
 * pvol_set_surface_integrator.  A rejected call changes nothing; a successful one replaces both maps; pvol_set_scene drops them. */
int pvol_set_surface_integrator_maps(pvol_ctx *ctx, const pvol_surface_params *sp, const pvol_photon_array *caustic,
                                     const pvol_photon_array *indirect);

/* ---- multi-GPU frame (north_star: pixel tiles partitioned over the GPUs of a node, one RCCL reduce of the film) ----
 * Rank `rank` of `n_ranks` renders the tasks rank, rank + n_ranks, ... of SamplerRenderer::Render's task loop
 * (renderers/samplerrenderer.cpp:206-221).  out_ids may be NULL to ask for the count only. */
int pvol_partition_tasks(uint32_t n_tasks, uint32_t rank, uint32_t n_ranks, uint32_t *out_ids, uint32_t capacity, uint32_t *n_out);

/* One rank's part of a frame, enqueued on hip_stream: d_pixels (x*y*4 floats, this rank's device) is zeroed, the rank's tasks are
 * rendered into it (pvol_render_tasks_device), ONE ncclReduce(sum, root 0) over `nccl_comm` (an ncclComm_t of n_ranks ranks made by
 * the caller with RCCL: ncclCommInitRank; ignored when n_ranks == 1) adds the ranks' films -- the Gaussian filter splats across tile
 * borders (film/image.cpp:82-134), so the films are summed, not gathered -- and rank 0 resolves into d_rgb (x*y*3 floats; may be
 * NULL on the other ranks).  Every rank needs the whole photon map first: either each runs pvol_preprocess with the same task
 * count (replicated), or the ranks share the shoot with pvol_preprocess_ranks, which leaves the same map on every rank.
 * RCCL is bound at run time (the copy already in the process, else librccl.so.1): PVOL_E_NO_DEVICE if none is in reach. */
int pvol_render_frame_ranks(pvol_ctx *ctx, const pvol_camera *camera, const pvol_film *film, const pvol_sampler *sampler,
                            uint32_t rank, uint32_t n_ranks, void *nccl_comm, float *d_pixels, float *d_rgb, void *hip_stream);

/* ---- several GPUs from ONE process: the two calls above with an in-process transport instead of a rendezvous and RCCL ----
 * ctxs: n_ctx (1 .. 64) distinct contexts made by pvol_create, each with its own params.device (several may share a device), all given
 * the same pvol_set_scene (and the same pvol_set_surface_integrator, if one is used).  Both calls run one host thread per context and
 * join them all before they return, so no context is ever left waiting for another.  A context takes part in one call at a time. */

/* pvol_preprocess_ranks(ctxs[i], n_tasks, block_paths, i, n_ctx, &comm) on every context at once, `comm` a host all-gather between the
 * threads (a barrier and one staging buffer, rank-major).  Every context ends with the map, the surface stores (keep_surface_photons)
 * and the pvol_get_shoot_stats of pvol_preprocess_blocks(ctx, n_tasks, block_paths) on one context, bit for bit.  Checked on every
 * context before any thread starts: PVOL_E_INVALID (NULL array or entry, n_ctx 0 or > 64, a context listed twice, n_tasks or
 * block_paths out of pvol_preprocess_blocks' range), PVOL_E_NO_SCENE, PVOL_E_NO_DEVICE (hipSetDevice fails).  An all-gather that
 * waits for a context whose thread has returned fails, which the ranks protocol turns into PVOL_E_NO_DEVICE on the others; the call
 * returns the code of the lowest-indexed context that failed on its own, else the code the protocol made every context agree on. */
int pvol_preprocess_group(pvol_ctx *const *ctxs, uint32_t n_ctx, uint32_t n_tasks, uint32_t block_paths);

/* One frame over the contexts: context i zeroes its own full-frame film d_pixels[i] (x*y*4 floats on its device, 16-byte aligned) and
 * renders the tasks pvol_partition_tasks(sampler->n_tasks, i, n_ctx) deals it into it (pvol_render_tasks_device) on hip_streams[i].
 * Once every context has, context 0's stream hip_streams[0] waits for the others', copies films 1 .. n_ctx-1 (hipMemcpyPeerAsync)
 * into a staging buffer context 0 keeps (grown on demand, freed by pvol_destroy), adds them in index order into d_pixels[0] and
 * resolves that into d_rgb (x*y*3 floats on context 0's device; NULL: no resolve).  Returns once all of it is enqueued:
 * synchronising hip_streams[0] covers every device, and until then films 1 .. n_ctx-1 are still being read.  hip_streams may be
 * NULL, and a NULL entry is the null stream of that context's device.  If any context fails nothing is reduced or resolved, and
 * the call returns the code of the lowest-indexed failing context.  PVOL_E_INVALID, checked before any device is touched: NULL
 * ctxs, d_pixels, camera, film or sampler, a NULL or duplicate context, a NULL or misaligned d_pixels[i], n_ctx 0 or > 64, an
 * empty film. */
int pvol_render_frame_group(pvol_ctx *const *ctxs, uint32_t n_ctx, const pvol_camera *camera, const pvol_film *film,
                            const pvol_sampler *sampler, float *const *d_pixels, float *d_rgb, void *const *hip_streams);

/* ImageFilm::AddSample (film/image.cpp:78-137) for n samples: d_image_xy 2 floats, d_xyz `xyz_stride`
 * floats per sample (X,Y,Z first). */
int pvol_film_add_samples_device(pvol_ctx *ctx, const pvol_film *film, const float *d_image_xy,
                                 const float *d_xyz, uint32_t xyz_stride, uint64_t n,
                                 float *d_pixels, void *hip_stream);

/* ImageFilm::WriteRGB (film/image.cpp:178-214) without splats: d_rgb gets 3 floats per pixel. */
int pvol_film_resolve_device(pvol_ctx *ctx, const pvol_film *film, const float *d_pixels, float *d_rgb,
                             void *hip_stream);

/* ---- crop window: Film "image" `"float cropwindow" [x0 x1 y0 y1]` (CreateImageFilm, film/image.cpp:254-264) ----
 * A crop render is not a cut-out of the full render: the window moves Film::GetSampleExtent, so Sampler::ComputeSubWindow deals
 * different tiles and every task's MT19937 stream covers different pixels.  The window goes to the film (below), its sample extent
 * into pvol_sampler.x_start .. y_end; the camera and the film's resolution stay those of the whole frame. */

/* ImageFilm's constructor (film/image.cpp:48-51): x_pixel_start = Ceil2Int(xRes * crop[0]), x_pixel_count =
 * max(1, Ceil2Int(xRes * crop[1]) - x_pixel_start), the same in y with crop[2], crop[3].  Host code, no GPU needed.
 * PVOL_E_INVALID: a NULL argument, a crop value outside [0, 1] (or NaN), crop[0] > crop[1] or crop[2] > crop[3] (CreateImageFilm
 * clamps and orders them first, :258-261), or a window that leaves the resolution (a crop that starts at 1). */
int pvol_film_window_from_crop(const pvol_film *film, const float *crop4, pvol_film_window *out);

/* ImageFilm::GetSampleExtent (film/image.cpp:157-166) of the window (NULL: the whole frame): out = x_start, x_end, y_start, y_end
 * for pvol_sampler.  Host code.  PVOL_E_INVALID: a NULL film or out, an invalid window. */
int pvol_film_sample_extent(const pvol_film *film, const pvol_film_window *window, int32_t out[4]);

/* pvol_render_tasks_device into a film that holds the window's pixels only: d_pixels has x_pixel_count * y_pixel_count * 4 floats,
 * row-major over the window.  A sample's footprint is clamped to the window and addressed relative to it (film/image.cpp:86-89,
 * :121): samples in the filter apron outside the window add to the pixels inside, a sample whose clamped footprint is empty adds
 * nothing but is rendered and draws like any other.  `sampler` carries the sample extent (pvol_film_sample_extent): the tasks'
 * sub-windows, the debug records and pvol_render_sample_count follow it, and a task whose sub-window is empty (more tasks than
 * the extent has columns; GetSubSampler returns NULL, samplers/lowdiscrepancy.cpp:61-66) renders nothing and draws nothing
 * (end_draw 0).  PVOL_E_INVALID for an invalid window, otherwise as pvol_render_tasks_device. */
int pvol_render_tasks_window_device(pvol_ctx *ctx, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window,
                                    const pvol_sampler *sampler, const uint32_t *task_ids, uint32_t n_task_ids,
                                    float *d_pixels, const pvol_render_debug *debug, void *hip_stream);

/* pvol_film_add_samples_device / pvol_film_resolve_device over the window's pixels (ImageFilm::AddSample, WriteRGB with
 * nPix = xPixelCount * yPixelCount, film/image.cpp:179): d_pixels 4, d_rgb 3 floats per pixel of the window. */
int pvol_film_add_samples_window_device(pvol_ctx *ctx, const pvol_film *film, const pvol_film_window *window, const float *d_image_xy,
                                        const float *d_xyz, uint32_t xyz_stride, uint64_t n, float *d_pixels, void *hip_stream);
int pvol_film_resolve_window_device(pvol_ctx *ctx, const pvol_film *film, const pvol_film_window *window, const float *d_pixels,
                                    float *d_rgb, void *hip_stream);

/* pvol_render_frame_ranks / pvol_render_frame_group with window-sized films: what is zeroed, reduced (ncclReduce; the staging buffer
 * and the sum of the group), and resolved is x_pixel_count * y_pixel_count pixels.  The tasks are dealt as before
 * (pvol_partition_tasks): which stream renders which pixel does not depend on the number of GPUs. */
int pvol_render_frame_ranks_window(pvol_ctx *ctx, const pvol_camera *camera, const pvol_film *film, const pvol_film_window *window,
                                   const pvol_sampler *sampler, uint32_t rank, uint32_t n_ranks, void *nccl_comm, float *d_pixels,
                                   float *d_rgb, void *hip_stream);
int pvol_render_frame_group_window(pvol_ctx *const *ctxs, uint32_t n_ctx, const pvol_camera *camera, const pvol_film *film,
                                   const pvol_film_window *window, const pvol_sampler *sampler, float *const *d_pixels, float *d_rgb,
                                   void *const *hip_streams);

#ifdef __cplusplus
}
#endif
#endif /* PVOL_H */
