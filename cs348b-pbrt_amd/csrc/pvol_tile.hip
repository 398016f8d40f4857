// pvol_tile.hip -- the image film and the small host restatements at the boundary of the render driver (pvol_render_host.hip): the film
// kernels (ImageFilm::AddSample / WriteRGB, film/image.cpp:78-137,178-214), film_add and the film entry points; the Gaussian filter
// table, Sampler::ComputeSubWindow, the sample count of a task list and ImageFilm's crop-window arithmetic; the round-robin deal of a
// frame's tasks to ranks and the run-time binding of RCCL.  The per-task sampler/camera kernel is pvol_tile_dev.h (compiled with the
// march kernels).
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include <dlfcn.h>

#include "pvol_host.h"
#include "pvol_math.h"

// ------------------------------------------------------------------------------------------ host restatements
extern "C" void pvol_gaussian_filter_table(float xw, float yw, float alpha, float *table) {
    // filters/gaussian.h:44-58 (expX, expY, Gaussian()), film/image.cpp:57-68 (table at cell centres)
    const float expX = expf(-alpha * xw * xw), expY = expf(-alpha * yw * yw);
    float *ftp = table;
    for (int y = 0; y < PVOL_FILTER_TABLE_SIZE; ++y) {
        float fy = ((float)y + .5f) * yw / PVOL_FILTER_TABLE_SIZE;
        for (int x = 0; x < PVOL_FILTER_TABLE_SIZE; ++x) {
            float fx = ((float)x + .5f) * xw / PVOL_FILTER_TABLE_SIZE;
            float gx = std::max(0.f, float(expf(-alpha * fx * fx) - expX));
            float gy = std::max(0.f, float(expf(-alpha * fy * fy) - expY));
            *ftp++ = gx * gy;
        }
    }
}

static inline float lerp_host(float t, float a, float b) { return (1.f - t) * a + t * b; }

extern "C" void pvol_compute_sub_window(const pvol_sampler *s, uint32_t num, int32_t out[4]) {   // core/sampler.cpp:55-74
    int count = (int)s->n_tasks;
    int dx = s->x_end - s->x_start, dy = s->y_end - s->y_start;
    int nx = count, ny = 1;
    while ((nx & 0x1) == 0 && 2 * dx * ny < dy * nx) {
        nx >>= 1;
        ny <<= 1;
    }
    int xo = (int)num % nx, yo = (int)num / nx;
    float tx0 = float(xo) / float(nx), tx1 = float(xo + 1) / float(nx);
    float ty0 = float(yo) / float(ny), ty1 = float(yo + 1) / float(ny);
    out[0] = (int)floorf(lerp_host(tx0, (float)s->x_start, (float)s->x_end));
    out[1] = (int)floorf(lerp_host(tx1, (float)s->x_start, (float)s->x_end));
    out[2] = (int)floorf(lerp_host(ty0, (float)s->y_start, (float)s->y_end));
    out[3] = (int)floorf(lerp_host(ty1, (float)s->y_start, (float)s->y_end));
}

extern "C" uint64_t pvol_render_sample_count(const pvol_sampler *s, const uint32_t *taskIds, uint32_t n) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        int32_t w[4];
        total += pvol_task_samples(s, taskIds[i], w);
    }
    return total;
}

// ImageFilm's constructor: the film image extent of a crop window (film/image.cpp:48-51)
extern "C" int pvol_film_window_from_crop(const pvol_film *film, const float *crop, pvol_film_window *out) {
    if (!film_ok(film) || !crop || !out) return PVOL_E_INVALID;
    for (int i = 0; i < 4; ++i) if (!(crop[i] >= 0.f && crop[i] <= 1.f)) return PVOL_E_INVALID;   // NaN fails too
    if (crop[0] > crop[1] || crop[2] > crop[3]) return PVOL_E_INVALID;
    pvol_film_window w;
    w.x_pixel_start = (int)ceilf(film->x_resolution * crop[0]);
    w.x_pixel_count = std::max(1, (int)ceilf(film->x_resolution * crop[1]) - w.x_pixel_start);
    w.y_pixel_start = (int)ceilf(film->y_resolution * crop[2]);
    w.y_pixel_count = std::max(1, (int)ceilf(film->y_resolution * crop[3]) - w.y_pixel_start);
    if (!pvol_window_ok(film, &w)) return PVOL_E_INVALID;   // crop[0] == crop[1] == 1: the reference's one pixel past the frame
    *out = w;
    return PVOL_OK;
}

// ImageFilm::GetSampleExtent (film/image.cpp:157-166)
extern "C" int pvol_film_sample_extent(const pvol_film *film, const pvol_film_window *window, int32_t out[4]) {
    if (!film_ok(film) || !out || !pvol_window_ok(film, window)) return PVOL_E_INVALID;
    const pvol_film_window w = pvol_window_or_full(film, window);
    out[0] = (int)floorf(w.x_pixel_start + 0.5f - film->filter_xwidth);
    out[1] = (int)ceilf(w.x_pixel_start + 0.5f + w.x_pixel_count + film->filter_xwidth);
    out[2] = (int)floorf(w.y_pixel_start + 0.5f - film->filter_ywidth);
    out[3] = (int)ceilf(w.y_pixel_start + 0.5f + w.y_pixel_count + film->filter_ywidth);
    return PVOL_OK;
}

// ------------------------------------------------------------------------------------------ film kernels
struct DevFilm {
    int32_t xres, yres;
    float xw, yw, invXW, invYW;
    float table[PVOL_FILTER_TABLE_SIZE * PVOL_FILTER_TABLE_SIZE];
};

__device__ __forceinline__ float wave_sum_f(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// ImageFilm::AddSample.  The samples of one pixel are neighbours in the array, so a wave's 64 footprints
// usually share one small pixel window: weights are summed over the wave first and one lane issues the atomics
// (the reference adds sample by sample with AtomicAdd in thread order, i.e. in no particular order either).
// `guard`: the unexpected-radiance checks of samplerrenderer.cpp:118-133 applied to the XYZ record.
//
// WINDOW: the film holds the pixels [wx0, wx1] x [wy0, wy1] of the frame only (ImageFilm's crop window): the footprint is clamped to
// the window (film/image.cpp:86-89) and a pixel is addressed relative to it, `pitch` pixels per row (:121).  A sample in the filter
// apron outside the window still reaches the pixels inside; one whose clamped footprint is empty leaves before any reduction or
// atomic, and a wave of such samples returns at the ballot.  The full-frame form has the four bounds and the pitch as the constants
// they were, so film_add_kernel compiles to what it was before the window existed.
template <bool WINDOW>
__device__ __forceinline__ void film_add_body(const DevFilm &F, const int wx0, const int wy0, const int wx1, const int wy1, const int pitch,
                                              const float *xy, const float *xyz, uint32_t stride, unsigned long long n, int guard, float *pixels) {
    __shared__ float table[PVOL_FILTER_TABLE_SIZE * PVOL_FILTER_TABLE_SIZE];
    table[threadIdx.x] = F.table[threadIdx.x];
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = i < n;
    float X = 0.f, Y = 0.f, Z = 0.f, dimageX = 0.f, dimageY = 0.f;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    if (on) {
        X = xyz[i * stride]; Y = xyz[i * stride + 1]; Z = xyz[i * stride + 2];
        if (guard && (isnan(X) || isnan(Y) || isnan(Z) || Y < -1e-5 || isinf(Y))) { X = 0.f; Y = 0.f; Z = 0.f; }
        dimageX = xy[2 * i] - 0.5f;
        dimageY = xy[2 * i + 1] - 0.5f;
        x0 = (int)ceilf(dimageX - F.xw); x1 = (int)floorf(dimageX + F.xw);
        y0 = (int)ceilf(dimageY - F.yw); y1 = (int)floorf(dimageY + F.yw);
        x0 = max(x0, WINDOW ? wx0 : 0); x1 = min(x1, WINDOW ? wx1 : F.xres - 1);
        y0 = max(y0, WINDOW ? wy0 : 0); y1 = min(y1, WINDOW ? wy1 : F.yres - 1);
    }
    const bool valid = on && (x1 - x0) >= 0 && (y1 - y0) >= 0;
    if (!__ballot(valid)) return;
    const int bx = wave_min_i(valid ? x0 : 0x7fffffff), ex = wave_max_i(valid ? x1 : -0x7fffffff);
    const int by = wave_min_i(valid ? y0 : 0x7fffffff), ey = wave_max_i(valid ? y1 : -0x7fffffff);
    if (ex - bx < 8 && ey - by < 8) {
        // the wave's sums for a pixel are four numbers in every lane; lanes 4 g .. 4 g + 3 keep those of the g-th pixel touched, and ONE
        // atomic instruction adds sixteen pixels' worth (the L2 atomic rate is per wave-instruction, MI355X_MICROARCH.md): 2 instead
        // of 100 instructions for a 5 x 5 footprint
        float *myAddr = 0;
        float myVal = 0.f;
        int slot = 0;
        for (int y = by; y <= ey; ++y) {
            const bool iny = valid && y >= y0 && y <= y1;
            const float fy = fabsf((y - dimageY) * F.invYW * PVOL_FILTER_TABLE_SIZE);
            const int iy = min((int)floorf(fy), PVOL_FILTER_TABLE_SIZE - 1);
            for (int x = bx; x <= ex; ++x) {
                float wt = 0.f;
                if (iny && x >= x0 && x <= x1) {
                    const float fx = fabsf((x - dimageX) * F.invXW * PVOL_FILTER_TABLE_SIZE);
                    const int ix = min((int)floorf(fx), PVOL_FILTER_TABLE_SIZE - 1);
                    wt = table[iy * PVOL_FILTER_TABLE_SIZE + ix];
                }
                if (!__ballot(wt != 0.f)) continue;
                const float sx = wave_sum_f(wt * X), sy = wave_sum_f(wt * Y), sz = wave_sum_f(wt * Z), sw = wave_sum_f(wt);
                if ((lane >> 2) == slot) {
                    const int c = lane & 3;
                    myAddr = pixels + 4 * (WINDOW ? (size_t)(y - wy0) * pitch + (x - wx0) : (size_t)y * F.xres + x) + c;
                    myVal = c == 0 ? sx : (c == 1 ? sy : (c == 2 ? sz : sw));
                }
                if (++slot == 16) {
                    atomicAdd(myAddr, myVal);   // all 64 lanes hold one
                    myAddr = 0; slot = 0;
                }
            }
        }
        if (myAddr) atomicAdd(myAddr, myVal);
    } else if (valid) {
        for (int y = y0; y <= y1; ++y) {
            const float fy = fabsf((y - dimageY) * F.invYW * PVOL_FILTER_TABLE_SIZE);
            const int iy = min((int)floorf(fy), PVOL_FILTER_TABLE_SIZE - 1);
            for (int x = x0; x <= x1; ++x) {
                const float fx = fabsf((x - dimageX) * F.invXW * PVOL_FILTER_TABLE_SIZE);
                const int ix = min((int)floorf(fx), PVOL_FILTER_TABLE_SIZE - 1);
                const float wt = table[iy * PVOL_FILTER_TABLE_SIZE + ix];
                float *p = pixels + 4 * (WINDOW ? (size_t)(y - wy0) * pitch + (x - wx0) : (size_t)y * F.xres + x);
                atomicAdd(p, wt * X); atomicAdd(p + 1, wt * Y); atomicAdd(p + 2, wt * Z); atomicAdd(p + 3, wt);
            }
        }
    }
}

__global__ __launch_bounds__(256) void film_add_kernel(DevFilm F, const float *xy, const float *xyz, uint32_t stride,
                                                      unsigned long long n, int guard, float *pixels) {
    film_add_body<false>(F, 0, 0, 0, 0, 0, xy, xyz, stride, n, guard, pixels);
}
// W = xPixelStart, yPixelStart, xPixelCount, yPixelCount
__global__ __launch_bounds__(256) void film_add_window_kernel(DevFilm F, int4 W, const float *xy, const float *xyz, uint32_t stride,
                                                             unsigned long long n, int guard, float *pixels) {
    film_add_body<true>(F, W.x, W.y, W.x + W.z - 1, W.y + W.w - 1, W.z, xy, xyz, stride, n, guard, pixels);
}

// ImageFilm::WriteRGB without splats (film/image.cpp:178-214), XYZToRGB core/spectrum.h:51-55: nPix = xPixelCount * yPixelCount
__global__ void film_resolve_kernel(int nPix, const float *pixels, float *rgb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPix) return;
    const float4 p = reinterpret_cast<const float4 *>(pixels)[i];
    float r = 3.240479f * p.x - 1.537150f * p.y - 0.498535f * p.z;
    float g = -0.969256f * p.x + 1.875991f * p.y + 0.041556f * p.z;
    float b = 0.055648f * p.x - 0.204043f * p.y + 1.057311f * p.z;
    if (p.w != 0.f) {
        const float invWt = 1.f / p.w;
        r = fmaxf(0.f, r * invWt); g = fmaxf(0.f, g * invWt); b = fmaxf(0.f, b * invWt);
    }
    rgb[3 * i] = r; rgb[3 * i + 1] = g; rgb[3 * i + 2] = b;
}

static DevFilm dev_film(const pvol_film *f) {
    DevFilm F;
    F.xres = f->x_resolution; F.yres = f->y_resolution;
    F.xw = f->filter_xwidth; F.yw = f->filter_ywidth;
    F.invXW = 1.f / f->filter_xwidth; F.invYW = 1.f / f->filter_ywidth;   // Filter ctor, core/filter.h:47-49
    memcpy(F.table, f->filter_table, sizeof(F.table));
    return F;
}

int film_add(pvol_ctx *c, const pvol_film *film, const pvol_film_window *window, const float *dXY, const float *dXYZ, uint32_t stride,
             uint64_t n, int guard, float *dPixels, hipStream_t stream) {
    if (!n) return PVOL_OK;
    const DevFilm F = dev_film(film);
    const unsigned long long blocks = (n + 255ull) / 256ull;
    if (blocks > 0x7fffffffull) return PVOL_E_LIMIT;
    if (!window) {
        hipLaunchKernelGGL(film_add_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, F, dXY, dXYZ, stride, (unsigned long long)n, guard, dPixels);
    } else {
        const int4 W = make_int4(window->x_pixel_start, window->y_pixel_start, window->x_pixel_count, window->y_pixel_count);
        hipLaunchKernelGGL(film_add_window_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, F, W, dXY, dXYZ, stride, (unsigned long long)n, guard,
                           dPixels);
    }
    return ok(hipGetLastError()) ? PVOL_OK : PVOL_E_NO_DEVICE;
}

extern "C" int pvol_film_add_samples_window_device(pvol_ctx *c, const pvol_film *film, const pvol_film_window *window, const float *dXY,
                                                   const float *dXYZ, uint32_t stride, uint64_t n, float *dPixels, void *hipStream) {
    if (!c || !film_ok(film) || !pvol_window_ok(film, window) || (n && (!dXY || !dXYZ || !dPixels)) || stride < 3) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    return film_add(c, film, window, dXY, dXYZ, stride, n, 0, dPixels, (hipStream_t)hipStream);
}
extern "C" int pvol_film_add_samples_device(pvol_ctx *c, const pvol_film *film, const float *dXY, const float *dXYZ, uint32_t stride,
                                            uint64_t n, float *dPixels, void *hipStream) {
    return pvol_film_add_samples_window_device(c, film, 0, dXY, dXYZ, stride, n, dPixels, hipStream);
}

extern "C" int pvol_film_resolve_window_device(pvol_ctx *c, const pvol_film *film, const pvol_film_window *window, const float *dPixels,
                                               float *dRgb, void *hipStream) {
    if (!c || !film_ok(film) || !pvol_window_ok(film, window) || !dPixels || !dRgb) return PVOL_E_INVALID;
    if (!ok(hipSetDevice(c->params.device))) return PVOL_E_NO_DEVICE;
    const pvol_film_window w = pvol_window_or_full(film, window);
    const int nPix = w.x_pixel_count * w.y_pixel_count;   // film/image.cpp:179
    hipLaunchKernelGGL(film_resolve_kernel, dim3((nPix + 255) / 256), dim3(256), 0, (hipStream_t)hipStream, nPix, dPixels, dRgb);
    return ok(hipGetLastError()) ? PVOL_OK : PVOL_E_NO_DEVICE;
}
extern "C" int pvol_film_resolve_device(pvol_ctx *c, const pvol_film *film, const float *dPixels, float *dRgb, void *hipStream) {
    return pvol_film_resolve_window_device(c, film, 0, dPixels, dRgb, hipStream);
}

// ------------------------------------------------------------------------------------------ tasks of a rank, RCCL
// The frame's render tasks dealt round-robin to the ranks: rank r renders tasks r, r + n, r + 2n, ... so that every rank's share
// is spread over the whole frame (SamplerRenderer::Render's task loop, renderers/samplerrenderer.cpp:206-221, cut n ways).
extern "C" int pvol_partition_tasks(uint32_t nTasks, uint32_t rank, uint32_t nRanks, uint32_t *outIds, uint32_t capacity, uint32_t *nOut) {
    if (!nRanks || rank >= nRanks || !nOut) return PVOL_E_INVALID;
    const uint32_t n = rank < nTasks ? (nTasks - rank + nRanks - 1) / nRanks : 0;
    *nOut = n;
    if (!outIds) return PVOL_OK;
    if (capacity < n) return PVOL_E_INVALID;
    for (uint32_t i = 0; i < n; ++i) outIds[i] = rank + i * nRanks;
    return PVOL_OK;
}

// RCCL is bound at run time: a process that already holds a copy (the application's own, or the one PyTorch ships) keeps using
// that one, and a single-GPU user of this library never loads it.  0 when no RCCL is in reach.
extern "C" void *pvol_rccl_symbol(const char *name) {
    if (void *sym = dlsym(RTLD_DEFAULT, name)) return sym;
    static void *lib = 0;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names)
            if ((lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    });
    return lib ? dlsym(lib, name) : 0;
}
