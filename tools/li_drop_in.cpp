// tools/li_drop_in.cpp -- the per-sample entry point as an unchanged SamplerRenderer drives it: T threads, each with its own
// live MT19937 state, call pvol_li in a loop on ONE context (renderers/samplerrenderer.cpp:247), with the library's coalescing
// off or on.  Native threads, so that the rate measured is the library's (Python threads would measure the GIL).
//
// DIR holds the inputs of tools/pvol_prof (tools/make_prof_inputs.py: scene, params, device-shot photon map, camera rays).
// usage: li_drop_in DIR THREADS MAX_BATCH WAIT_US [SECONDS]
//   MAX_BATCH <= 1: coalescing off (every call is its own batch, serialised).  Prints one JSON line.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../include/pvol.h"

static std::vector<unsigned char> slurp(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return b;
}
#define CK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, pvol_strerror(rc_)); return 1; } } while (0)

static void mt_seed(uint32_t *mt, uint32_t seed) {   // core/rng.cpp:41-49
    mt[0] = seed;
    for (int i = 1; i < PVOL_MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: li_drop_in DIR THREADS MAX_BATCH WAIT_US [SECONDS]\n"); return 64; }
    const std::string dir = argv[1];
    const int nThreads = std::max(1, atoi(argv[2]));
    const uint32_t maxBatch = (uint32_t)std::max(0, atoi(argv[3])), waitUs = (uint32_t)std::max(0, atoi(argv[4]));
    const double seconds = argc > 5 ? atof(argv[5]) : 3.0;
    std::vector<unsigned char> sb = slurp(dir + "/scene.bin"), pb = slurp(dir + "/params.bin"), phb = slurp(dir + "/photons.bin"),
                               rb = slurp(dir + "/rays.bin");
    pvol_scene scene;
    memcpy(&scene, sb.data(), sizeof(scene));
    size_t off = sizeof(scene);
    scene.lights = (const pvol_light *)(sb.data() + off); off += sizeof(pvol_light) * scene.n_lights;
    scene.triangles = (const pvol_triangle *)(sb.data() + off); off += sizeof(pvol_triangle) * scene.n_triangles;
    scene.materials = (const pvol_material *)(sb.data() + off); off += sizeof(pvol_material) * scene.n_materials;
    scene.volume.density = scene.volume.kind == PVOL_VOLUME_GRID ? (const float *)(sb.data() + off) : 0;
    pvol_params params;
    memcpy(&params, pb.data(), sizeof(params));
    uint32_t nPh, nRays;
    memcpy(&nPh, phb.data(), 4);
    const float *pp = (const float *)(phb.data() + 4), *pw = pp + 3 * (size_t)nPh, *pa = pw + 3 * (size_t)nPh;
    memcpy(&nRays, rb.data(), 4);
    std::vector<pvol_ray> rays(nRays);
    memcpy(rays.data(), rb.data() + 8, sizeof(pvol_ray) * (size_t)nRays);
    for (auto &r : rays) r.rng_skip = 0;   // the caller's own state is handed in: nothing to skip

    pvol_ctx *ctx = 0;
    CK(pvol_create(&params, &ctx));
    CK(pvol_set_scene(ctx, &scene));
    CK(pvol_upload_photons(ctx, pp, pw, pa, nPh));
    CK(pvol_set_li_coalescing(ctx, maxBatch, waitUs));
    {   // warm-up: first-use allocations of the context (record plan, hand-over list, staging) outside the timed window
        uint32_t mt[PVOL_MT_N];
        mt_seed(mt, 1);
        int32_t mti = PVOL_MT_N;
        float Lv[PVOL_NBINS], T[PVOL_NBINS];
        for (int k = 0; k < 4; ++k) CK(pvol_li(ctx, &rays[(size_t)k % nRays], mt, &mti, Lv, T));
    }
    uint64_t st[6];
    CK(pvol_get_li_coalescing_stats(ctx, st, 1));

    std::atomic<bool> stop{false};
    std::atomic<int> failed{0};
    std::vector<std::vector<float> > lat(nThreads);
    std::vector<double> checksum(nThreads, 0.0);
    auto worker = [&](int t) {
        uint32_t mt[PVOL_MT_N];
        mt_seed(mt, 1000u + (uint32_t)t);
        int32_t mti = PVOL_MT_N;
        float Lv[PVOL_NBINS], T[PVOL_NBINS];
        lat[t].reserve(1 << 16);
        for (size_t k = (size_t)t; !stop.load(std::memory_order_relaxed); k += (size_t)nThreads) {   // thread t: rays t, t + T, ...
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = pvol_li(ctx, &rays[k % nRays], mt, &mti, Lv, T);
            const auto t1 = std::chrono::steady_clock::now();
            if (rc != PVOL_OK) { fprintf(stderr, "thread %d: pvol_li -> %s\n", t, pvol_strerror(rc)); failed = 1; return; }
            lat[t].push_back((float)std::chrono::duration<double, std::micro>(t1 - t0).count());
            checksum[t] += Lv[0] + Lv[15] + T[29];
        }
    };
    const auto w0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < nThreads; ++t) th.emplace_back(worker, t);
    std::this_thread::sleep_for(std::chrono::duration<double>(seconds));
    stop = true;
    for (auto &x : th) x.join();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    if (failed) { pvol_destroy(ctx); return 1; }
    CK(pvol_get_li_coalescing_stats(ctx, st, 0));
    std::vector<float> all;
    double sum = 0.0;
    for (int t = 0; t < nThreads; ++t) { all.insert(all.end(), lat[t].begin(), lat[t].end()); sum += checksum[t]; }
    std::sort(all.begin(), all.end());
    auto pct = [&](double q) { return all.empty() ? 0.0 : (double)all[std::min(all.size() - 1, (size_t)(q * (double)all.size()))]; };
    const double calls = (double)all.size();
    printf("{\"threads\": %d, \"max_batch\": %u, \"wait_us\": %u, \"calls\": %.0f, \"wall_s\": %.3f, \"calls_per_s\": %.1f, "
           "\"mean_batch\": %.2f, \"largest_batch\": %llu, \"queued_behind\": %llu, \"p50_us\": %.1f, \"p99_us\": %.1f, \"photons\": %u, "
           "\"checksum\": %.6g}\n",
           nThreads, maxBatch, waitUs, calls, wall, calls / wall, st[1] ? (double)st[0] / (double)st[1] : 1.0, (unsigned long long)st[2],
           (unsigned long long)st[3], pct(0.50), pct(0.99), nPh, sum);
    pvol_destroy(ctx);
    return 0;
}
