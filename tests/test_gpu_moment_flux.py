"""li_group_kernel's moment form (an XYZ result of a nearly grey medium sums nine moments per photon instead
of 30 bins) through pvol_li_batch_device on the committed 6 k-photon map with nused 50: per sample against the oracle at
tests/test_gpu_group.py's bar (1e-4 rel. L2, draw counts exact), the same rays with PVOL_NO_MOMENTS=1 in a fresh child process at the
same bar, and a scene whose sigma_t fails the gate, which keeps the 30-bin form and must give what the parent commit gave.

The batch is built to reach every branch of the changed code: a ray count that is no multiple of 64 or 512 (partial last group and
chunk), rays that miss the volume, a sparse map (short sets: fewer than k inside maxdist, fewer than 10 found), groups of one pixel's
samples (every served lane shares most members: the shared-member sum runs) and groups of samples from all over the frame (few shared
members: it does not; quartets of disagreeing slots come out partial), and lookups handed to li_fixup_kernel, so that rays receive
terms from both kernels.  What the device counts (pvol_stats, a stats launch of the same rays: the selection is the same code in
either form) is asserted; the shared-member sum and the partial quartets have no counter in pvol_stats and follow from the batch's
construction alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, abi, blob, load_photons, load_scene, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_group.py


def _scene(coloured):
    s = dict(load_scene("volumescene_h"))
    if coloured:   # sigma_t varying +-20 % over the bins: the gate refuses it (tests/test_moment_plan.py)
        f = np.linspace(0.8, 1.2, 30).astype(np.float32)
        s["vol.sigma_a"] = s["vol.sigma_a"] * f
        s["vol.sigma_s"] = s["vol.sigma_s"] * f
    return s


MAX_DIST = 0.85   # the 6 k photons lie in clumps: the rays' query points see 50 and more inside this radius, 10 .. 49, and fewer than 10


def _params(s):
    return abi.params_from_blob(s, n_used=50, max_dist=MAX_DIST)


def _neighbour_counts(s, photons, rays):
    """Photons within MAX_DIST of points along a sample of the rays, inside the medium (host arithmetic)."""
    w2v = s["vol.w2v"].reshape(4, 4).astype(np.float64)
    ext = s["vol.extent"].astype(np.float64)
    sub = rays[:: max(1, len(rays) // 150)]
    t = np.arange(0.25, 40.0, 0.5)
    pts = (sub["o"].astype(np.float64)[:, None, :] + sub["d"].astype(np.float64)[:, None, :] * t[None, :, None]).reshape(-1, 3)
    pv = pts @ w2v[:3, :3].T + w2v[:3, 3]
    pts = pts[((pv >= ext[:3]) & (pv <= ext[3:])).all(1)]
    pos = photons[0].astype(np.float64)
    counts = np.empty(len(pts), np.int64)
    for i in range(0, len(pts), 512):
        d2 = ((pts[i:i + 512, None, :] - pos[None, :, :]) ** 2).sum(-1)
        counts[i:i + 512] = (d2 < MAX_DIST * MAX_DIST).sum(1)
    return counts


def _batch(orc, s, spread_tasks=(700, 1500, 3000)):
    """~7 k rays: one render task at 64 spp in bucket order (compact groups), three tasks at 16 spp shuffled (spread groups), 7 misses, 512 fanned out."""
    def camera(spp, tasks):
        cam = abi.perspective_camera(float(s["camera.fov"][0]), 640, 360, s["camera.c2w"])
        film = abi.make_film(640, 360, orc.gaussian_filter_table())
        smp = abi.make_sampler(640, 360, spp, 4096)
        o = orc.Oracle(abi.SceneHolder(s), _params(s))   # no photon map: only the rays are wanted
        return orc.render_tasks(o, cam, film, smp, np.asarray(tasks, np.uint32))["rays"]
    compact = camera(64, [2100])
    spread = camera(16, list(spread_tasks))
    spread = spread[np.random.default_rng(5).permutation(len(spread))]
    miss = compact[:7].copy()
    miss["o"] = miss["o"] + np.array([0, 1000, 0], np.float32)   # far above the medium, looking further up
    miss["d"] = np.array([0, 1, 0], np.float32)
    # fans of parallel rays across squares of growing width: their groups' query points lie too far apart for one bucket, the
    # attempts serve halves of them and hand the rest over
    rng = np.random.default_rng(6)
    d0 = compact["d"].astype(np.float64).mean(0)
    d0 /= np.linalg.norm(d0)
    u = np.cross(d0, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(d0, u)
    fan = compact[:4 * 128].copy()
    width = np.repeat([0.6, 1.2, 2.5, 5.0], 128)[:, None]
    ab = (rng.random((len(fan), 2)) - 0.5) * width
    fan["o"] = (compact["o"][0].astype(np.float64) + ab[:, :1] * u + ab[:, 1:] * v).astype(np.float32)
    fan["d"] = d0.astype(np.float32)
    fan["scatter_u"] = rng.random(len(fan)).astype(np.float32)
    rays = np.concatenate([compact, miss, spread, fan])
    while len(rays) % 64 == 0 or len(rays) % 512 == 0:
        rays = rays[:-1]
    n = len(rays)
    assert 3000 < n < 8000
    counts = np.array([n // 3, n // 3, n - 2 * (n // 3)], np.uint32)
    return np.ascontiguousarray(rays), abi.make_streams(np.array([11, 12, 13], np.uint32), counts)


def _device_li(pvol, s, photons, rays, streams, stats=False):
    """pvol_li_batch_device, XYZ: (out[n, 4], draws[n], end_draw per stream, pvol_stats or None)."""
    import torch
    pv = pvol.PhotonVolume(_params(s))
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*photons)
        n = len(rays)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_streams = torch.from_numpy(streams.copy().view(np.uint8)).cuda()
        d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        d_draws = torch.zeros(n, dtype=torch.int32, device="cuda")
        if stats:
            pv.enable_stats(True)
            pv.stats(reset=True)
        pv.li_device(d_rays.data_ptr(), n, d_streams.data_ptr(), len(streams), abi.OUT_XYZ, d_out.data_ptr(), d_draws.data_ptr(), 0)
        torch.cuda.synchronize()
        pv.check_errors()
        assert pv.march_kernel_name() == "li_group_kernel"
        end = d_streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)["end_draw"].copy()
        return d_out.cpu().numpy(), d_draws.cpu().numpy().astype(np.uint32), end, (pv.stats() if stats else None)
    finally:
        pv.close()


def _child(path_in, path_out):
    """The fresh process of the PVOL_NO_MOMENTS=1 leg: same rays, same map, the knob read when the context is created."""
    import importlib
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    d = np.load(path_in)
    rays, streams = d["rays"].view(abi.RAY_DTYPE).reshape(-1), d["streams"].view(abi.STREAM_DTYPE).reshape(-1)
    out, draws, end, _ = _device_li(pvol, _scene(bool(d["coloured"])), load_photons("vh"), rays, streams)
    np.save(path_out, np.concatenate([out.reshape(-1), draws.astype(np.float32), end.astype(np.float32)]))


def _no_moments(tmp_path, rays, streams, coloured):
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npy")
    np.savez(src, rays=rays.view(np.uint8), streams=streams.view(np.uint8), coloured=coloured)
    env = dict(os.environ, PVOL_NO_MOMENTS="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", src, dst], env=env, check=True, timeout=120, cwd=ROOT)
    n = len(rays)
    flat = np.load(dst)
    return flat[:4 * n].reshape(n, 4), flat[4 * n:5 * n].astype(np.uint32)


@pytest.fixture(scope="module")
def pvol():
    import importlib
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1
    return m


@pytest.fixture(scope="module")
def grey(pvol, orc):
    """The batch, the oracle's answer and the device's (moment form), computed once for the tests below."""
    s = _scene(False)
    photons = load_photons("vh")
    rays, streams = _batch(orc, s)
    o = orc.Oracle(abi.SceneHolder(s), _params(s))
    o.set_photons(*photons)
    o_streams = streams.copy()
    ref, rdraws = o.li_batch(rays, o_streams, abi.OUT_XYZ, n_threads=8)
    got, draws, end, _ = _device_li(pvol, s, photons, rays, streams)
    return dict(s=s, photons=photons, rays=rays, streams=streams, ref=ref, rdraws=rdraws, rend=o_streams["end_draw"].copy(), got=got, draws=draws, end=end)


def _check_against_oracle(got, draws, ref, rdraws):
    assert (draws == rdraws).all()
    floor = 1e-6 * float(np.abs(ref[:, :3]).max())
    err = rel_l2(got[:, :3], ref[:, :3], floor=floor)
    print("XYZ against the oracle: worst rel L2 %.3g at ray %d" % (err.max(), int(err.argmax())))
    assert err.max() <= TOL, "rel L2 %.3g at ray %d" % (err.max(), int(err.argmax()))
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=1e-7)


def test_the_batch_reaches_every_branch(pvol, grey):
    """From the device's own counters (a stats launch of the same rays; it sums 30 bins, the selection is the same code)."""
    n = len(grey["rays"])
    assert n % 64 and n % 512 and n > 512          # partial last group, partial last chunk, more than one chunk
    assert (grey["rdraws"] == 0).sum() >= 7          # rays that miss the volume draw nothing
    assert (np.linalg.norm(grey["ref"][:, :3], axis=1) > 0).sum() > n // 2
    _, _, _, st = _device_li(pvol, grey["s"], grey["photons"], grey["rays"], grey["streams"], stats=True)
    print({k: st[k] for k in ("n_rays", "n_steps", "n_kept", "n_lookups_lt10", "n_guess_retries", "group_attempts", "group_deferred_too_few")})
    assert st["n_rays"] == n
    assert st["n_kept"] > 0 and st["group_attempts"] > 0
    # lookups handed to li_fixup_kernel, far fewer than the rays' steps: rays get terms from both kernels
    assert 0 < st["n_guess_retries"] < st["n_steps"] // 4
    assert st["n_lookups_lt10"] > 0   # among the lookups handed over (li_fixup_kernel counts its own)
    # the query points see full sets, short sets with a flux (10 .. 49 photons inside maxdist) and short sets without (fewer than 10;
    # li_group_kernel has no counter for those, li_fixup_kernel counts the ones it was handed)
    counts = _neighbour_counts(grey["s"], grey["photons"], grey["rays"])
    print("photons inside maxdist at %d points: %d below 10, %d in 10..49, %d at 50 or more" %
          (len(counts), (counts < 10).sum(), ((counts >= 10) & (counts < 50)).sum(), (counts >= 50).sum()))
    assert (counts < 10).sum() > 20 and ((counts >= 10) & (counts < 50)).sum() > 20 and (counts >= 50).sum() > 20


def test_moment_form_matches_the_oracle(grey):
    _check_against_oracle(grey["got"], grey["draws"], grey["ref"], grey["rdraws"])
    assert (grey["end"] == grey["rend"]).all()


def test_thirty_bin_form_in_a_fresh_process_matches_the_oracle_too(grey, tmp_path):
    out, draws = _no_moments(tmp_path, grey["rays"], grey["streams"], False)
    _check_against_oracle(out, draws, grey["ref"], grey["rdraws"])
    scale = float(np.abs(out[:, :3]).max())
    rel = np.abs(grey["got"][:, :3].astype(np.float64) - out[:, :3]) / np.maximum(np.abs(out[:, :3]), 1e-6 * scale)
    # no bar beyond the oracle's: fp32 summation order (profiles/moment_flux_forms.txt keeps the figure)
    print("moment form against the 30-bin form: largest relative difference %.3g" % rel.max())


def test_a_coloured_medium_keeps_the_thirty_bins_and_the_parents_result(pvol, orc, tmp_path):
    """sigma_t +-20 % over the bins fails the gate: the result is the 30-bin form's, which is what the parent commit computed
    (tests/golden/li_moment_coloured_parent.bin, written by the parent commit's library for this batch).  Tolerance: what
    tests/test_gpu_group.py allows between two runs of one build, whose fp32 additions come in scheduling order."""
    s = _scene(True)
    photons = load_photons("vh")
    rays, streams = _batch(orc, s)
    got, draws, _, _ = _device_li(pvol, s, photons, rays, streams)
    parent = blob.load(os.path.join(GOLD, "li_moment_coloured_parent.bin"))
    want = parent["xyz"].reshape(-1, 4)
    assert want.shape == got.shape and (parent["draws"] == draws).all()
    scale = float(np.abs(want[:, :3]).max())
    np.testing.assert_allclose(got, want, rtol=5e-6, atol=1e-7 * scale)
    o = orc.Oracle(abi.SceneHolder(s), _params(s))
    o.set_photons(*photons)
    ref, rdraws = o.li_batch(rays, streams.copy(), abi.OUT_XYZ, n_threads=8)
    _check_against_oracle(got, draws, ref, rdraws)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2], sys.argv[3])
