"""The yardstick of the final gather's sum (integrators/photonmap.cpp:231-246, :277-295): from the direction records of
both loops, what every gather ray found -- (hit, Lo row, path length in the medium) -- the query's Kd and the medium's sigma_t to
    L = (Kd INV_PI) (.) [ sum_bsdf weight Lindir T + sum_photon weight Lindir T ] / n_samples,   T = exp(-sigma_t length),
in float64, and to the number of RandomFloat calls.  The tracing itself is not restated here: the GPU tests take it from entry points
that are pinned on their own (pvol_gather_directions, pvol_probe_hits, pvol_radiance_lookup, pvol_download_radiance_lo).

loops_f32() is the literal transcription of the two loops, sample by sample in float32, that the yardstick is checked against."""
import numpy as np

F = np.float32
INV_PI = F(0.31830988618379067154)   # core/pbrt.h:192
NONE = 0xffffffff


def dead_queries(kd):
    """Queries that trace nothing: Kd black in every bin (fr.IsBlack()).  A query whose lookup found fewer than 50 photons has
    no valid record in either loop and needs no flag."""
    return ~(np.asarray(kd) != 0).any(axis=1)


def final_gather(dirs_b, dirs_p, found_b, found_p, kd, sigma_t, medium):
    """dirs_*: [count, n_samples] records with fields `weight` and `valid`; found_*: per loop a tuple (hit[count, n_samples] bool,
    lo[count, n_samples, 30] -- zeros where no photon faces --, length[count, n_samples]); kd[count, 30]; sigma_t[30]; medium: the
    scene has a volume region.  Returns (L[count, 30] float64, draws[count] uint32)."""
    kd = np.asarray(kd, np.float64)
    count, n_samples = dirs_b.shape
    dead = dead_queries(kd)
    total = np.zeros((count, 30))
    draws = np.zeros(count, np.uint32)
    for dirs, (hit, lo, length) in ((dirs_b, found_b), (dirs_p, found_p)):
        use = (dirs["valid"] == 1) & np.asarray(hit, bool) & ~dead[:, None]
        T = np.exp(-np.asarray(sigma_t, np.float64)[None, None, :] * np.asarray(length, np.float64)[:, :, None]) if medium else 1.0
        term = dirs["weight"].astype(np.float64)[:, :, None] * np.asarray(lo, np.float64) * T
        total += np.where(use[:, :, None], term, 0.0).sum(axis=1)
        if medium:
            draws += use.sum(axis=1).astype(np.uint32)   # one RandomFloat per gather ray that hits, even when Lindir is 0
    return kd * np.float64(INV_PI) * total / n_samples, draws


def loops_f32(dirs_b, dirs_p, found_b, found_p, kd, sigma_t, medium):
    """The two loops as the reference writes them, one sample at a time in float32:
        Lindir = Lo;  Lindir *= Exp(-tau);  Li += fr * Lindir * (AbsDot(wi, n) * wt / pdf);   ...   L += Li / gatherSamples"""
    count, n_samples = dirs_b.shape
    sigma_t = np.asarray(sigma_t, F)
    L = np.zeros((count, 30), F)
    draws = np.zeros(count, np.uint32)
    for q in range(count):
        fr = np.asarray(kd[q], F) * INV_PI
        if not (fr != 0).any():
            continue
        for dirs, (hit, lo, length) in ((dirs_b, found_b), (dirs_p, found_p)):
            Li = np.zeros(30, F)
            for s in range(n_samples):
                if dirs["valid"][q, s] != 1 or not hit[q, s]:
                    continue
                Lindir = np.asarray(lo[q, s], F)
                if medium:
                    draws[q] += 1
                    Lindir = Lindir * np.exp(-(sigma_t * F(length[q, s]))).astype(F)
                Li = Li + fr * Lindir * F(dirs["weight"][q, s])
            L[q] = L[q] + Li / F(n_samples)
    return L, draws


def rel_l2(got, want):
    """Per query ||got - want|| / max(||want||, 1e-6 of the largest value in the call) over the 30 bins."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    floor = 1e-6 * float(np.abs(want).max()) if want.size else 0.0
    return np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), max(floor, 1e-300))
