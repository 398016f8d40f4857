"""li_group_kernel's settled class (the bucket's inner photons, members for every lane an attempt serves, leave
both selection passes and enter the shared-member sum) on the shapes of tests/test_gpu_group.py: the 150 k-photon device-shot
volumescene map, the rays of render tasks 700 and 2100 at 640 x 360 and 64 spp.  Two legs, the default knob in this process and
PVOL_GROUP_PRECORE=0 in a fresh child (the knob is read when a context is created), each launching the batch twice: XYZ as the
flagship does (the moment form) and with the device's counters on (the 30-bin form: the selection is the same code in either).
Both legs are held to the oracle at the project's bar, 1e-4 rel. L2 per ray, draw counts and stream ends exact; no bound is set on the
difference between the legs (fp32 summation order: the settled rows are summed once for the wave).  From the counters: the lanes'
passes run over fewer slots per attempt with the rule on, and the rule buys that with no hand-overs (n_guess_retries no higher than
the off leg's plus 1 % of the steps -- a condition, not a tolerance).  On the committed 6 k-photon map, whose lookups mostly search the
full radius, the rule gates itself off: same results, same n_tested."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, abi, load_photons, load_scene, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_group.py
KNOB = "PVOL_GROUP_PRECORE"


def _params(s, coarse):
    return abi.params_from_blob(s) if coarse else abi.params_from_blob(s, n_volume_photons=150000)


def _launch(pv, rays, streams, stats):
    """pvol_li_batch_device, XYZ: out[n, 4], draws[n], end_draw per stream, pvol_stats or None."""
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_streams = torch.from_numpy(streams.copy().view(np.uint8)).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    d_draws = torch.zeros(n, dtype=torch.int32, device="cuda")
    pv.enable_stats(stats)
    if stats:
        pv.stats(reset=True)
    pv.li_device(d_rays.data_ptr(), n, d_streams.data_ptr(), len(streams), abi.OUT_XYZ, d_out.data_ptr(), d_draws.data_ptr(), 0)
    torch.cuda.synchronize()
    pv.check_errors()
    assert pv.march_kernel_name() == "li_group_kernel"
    end = d_streams.cpu().numpy().view(abi.STREAM_DTYPE).reshape(-1)["end_draw"].copy()
    return d_out.cpu().numpy(), d_draws.cpu().numpy().astype(np.uint32), end, (pv.stats() if stats else None)


def _leg(pvol, photons, rays, streams, coarse):
    """One context (it reads the knob now), the batch without and with counters."""
    s = load_scene("volumescene_h")
    pv = pvol.PhotonVolume(_params(s, coarse))
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*photons)
        out, draws, end, _ = _launch(pv, rays, streams, False)
        sout, sdraws, send, st = _launch(pv, rays, streams, True)
        return dict(out=out, draws=draws, end=end, sout=sout, sdraws=sdraws, send=send, stats=st)
    finally:
        pv.close()


def _child(path_in, path_out):
    import importlib
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    d = np.load(path_in)
    rays, streams = d["rays"].view(abi.RAY_DTYPE).reshape(-1), d["streams"].view(abi.STREAM_DTYPE).reshape(-1)
    r = _leg(pvol, (d["p"], d["wi"], d["alpha"]), rays, streams, bool(d["coarse"]))
    st = r.pop("stats")
    np.savez(path_out, stats=json.dumps(st), **r)


def _fresh_process(tmp, tag, knob, photons, rays, streams, coarse):
    src, dst = str(tmp / (tag + "_in.npz")), str(tmp / (tag + "_out.npz"))
    np.savez(src, rays=rays.view(np.uint8), streams=streams.view(np.uint8), p=photons[0], wi=photons[1], alpha=photons[2], coarse=coarse)
    env = dict(os.environ)
    env.pop(KNOB, None)
    if knob is not None:
        env[KNOB] = knob
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", src, dst], env=env, check=True, timeout=120, cwd=ROOT)
    d = np.load(dst)
    r = {k: d[k] for k in ("out", "draws", "end", "sout", "sdraws", "send")}
    r["stats"] = json.loads(str(d["stats"]))
    return r


def _default_leg(pvol, photons, rays, streams, coarse):
    old = os.environ.pop(KNOB, None)   # the default is the unset knob
    try:
        return _leg(pvol, photons, rays, streams, coarse)
    finally:
        if old is not None:
            os.environ[KNOB] = old


@pytest.fixture(scope="module")
def pvol():
    import importlib
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1
    return m


@pytest.fixture(scope="module")
def batch(orc):
    """tests/test_gpu_group.py's camera batch: whole render tasks 700 and 2100 of 4096 at 640 x 360, 64 spp."""
    s = load_scene("volumescene_h")
    tasks = [700, 2100]
    cam = abi.perspective_camera(float(s["camera.fov"][0]), 640, 360, s["camera.c2w"])
    film = abi.make_film(640, 360, orc.gaussian_filter_table())
    smp = abi.make_sampler(640, 360, 64, 4096)
    o = orc.Oracle(abi.SceneHolder(s), abi.params_from_blob(s))   # no photon map: only the rays are wanted
    rays = orc.render_tasks(o, cam, film, smp, np.asarray(tasks, np.uint32))["rays"]
    counts = [orc.sub_window(smp, t) for t in tasks]
    counts = np.array([(w[1] - w[0]) * (w[3] - w[2]) * 64 for w in counts], np.uint32)
    assert 4096 <= len(rays) <= 9000
    return s, np.ascontiguousarray(rays), abi.make_streams(np.asarray(tasks, np.uint32), counts)


def _oracle(orc, s, coarse, photons, rays, streams):
    o = orc.Oracle(abi.SceneHolder(s), _params(s, coarse))
    o.set_photons(*photons)
    st = streams.copy()
    ref, rdraws = o.li_batch(rays, st, abi.OUT_XYZ, n_threads=8)
    return dict(ref=ref, rdraws=rdraws, rend=st["end_draw"].copy())


@pytest.fixture(scope="module")
def dense(pvol, orc, batch, tmp_path_factory):
    """The 150 k-photon map shot on the device, the oracle's answer, and the two legs: computed once, left unchanged."""
    s, rays, streams = batch
    pv = pvol.PhotonVolume(_params(s, False))
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.preprocess(8192)
        assert pv.photon_count() >= 150000
        photons = pv.download_photons()
    finally:
        pv.close()
    d = _oracle(orc, s, False, photons, rays, streams)
    d["on"] = _default_leg(pvol, photons, rays, streams, False)
    d["off"] = _fresh_process(tmp_path_factory.mktemp("precore"), "dense", "0", photons, rays, streams, False)
    return d


def _check_against_oracle(what, got, draws, end, d):
    assert (draws == d["rdraws"]).all()
    assert (end == d["rend"]).all()
    ref = d["ref"]
    floor = 1e-6 * float(np.abs(ref[:, :3]).max())
    err = rel_l2(got[:, :3], ref[:, :3], floor=floor)
    print("%s against the oracle: worst rel L2 %.3g at ray %d" % (what, err.max(), int(err.argmax())))
    assert err.max() <= TOL, "%s: rel L2 %.3g at ray %d" % (what, err.max(), int(err.argmax()))
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=1e-7)
    return float(err.max())


def _largest_difference(a, b):
    scale = float(np.abs(b[:, :3]).max())
    return float((np.abs(a[:, :3].astype(np.float64) - b[:, :3]) / np.maximum(np.abs(b[:, :3]), 1e-6 * scale)).max())


def test_default_knob_matches_the_oracle(dense):
    assert (np.linalg.norm(dense["ref"][:, :3], axis=1) > 0).sum() > len(dense["ref"]) // 4
    leg = dense["on"]
    _check_against_oracle("rule on, moment form", leg["out"], leg["draws"], leg["end"], dense)
    _check_against_oracle("rule on, 30 bins (counters on)", leg["sout"], leg["sdraws"], leg["send"], dense)


def test_rule_off_in_a_fresh_process_matches_the_oracle_too(dense):
    on, off = dense["on"], dense["off"]
    e_off = _check_against_oracle("rule off, moment form", off["out"], off["draws"], off["end"], dense)
    _check_against_oracle("rule off, 30 bins (counters on)", off["sout"], off["sdraws"], off["send"], dense)
    e_on = _check_against_oracle("rule on, moment form", on["out"], on["draws"], on["end"], dense)
    # no bar beyond the oracle's on the difference between the legs: fp32 summation order
    dm, db = _largest_difference(on["out"], off["out"]), _largest_difference(on["sout"], off["sout"])
    text = ("tests/test_gpu_group_precore.py: %d rays, 150 k-photon volumescene map, nused 50\n"
            "  rule on  (default knob): worst rel. L2 per ray against the oracle %.3g\n"
            "  rule off (%s=0, fresh process): worst rel. L2 per ray against the oracle %.3g\n"
            "  largest relative difference per component between the two legs: moment form %.3g, 30-bin form %.3g\n"
            % (len(dense["ref"]), e_on, KNOB, e_off, dm, db))
    print(text)
    with open(os.path.join(ROOT, "profiles", "precore_forms.txt"), "w") as f:
        f.write(text)


def test_fewer_slots_per_attempt_and_no_more_hand_overs(dense):
    on, off = dense["on"]["stats"], dense["off"]["stats"]
    for name, st in (("on", on), ("off", off)):
        print("rule %s:" % name, {k: st[k] for k in ("n_steps", "n_tested", "group_attempts", "n_guess_retries", "group_guess_failed", "n_kept")},
              "n_tested / group_attempts %.2f" % (st["n_tested"] / st["group_attempts"]))
    assert on["n_steps"] == off["n_steps"] and on["group_attempts"] > 0 and off["group_attempts"] > 0
    assert on["n_tested"] / on["group_attempts"] < off["n_tested"] / off["group_attempts"]
    assert on["n_guess_retries"] <= off["n_guess_retries"] + 0.01 * on["n_steps"]


def test_a_coarse_map_gates_the_rule_off(pvol, orc, batch, tmp_path):
    """The committed 6 k-photon map under the scene's own parameters: nearly every lookup searches the full radius."""
    s, rays, streams = batch
    photons = load_photons("vh")
    d = _oracle(orc, s, True, photons, rays, streams)
    on = _default_leg(pvol, photons, rays, streams, True)
    off = _fresh_process(tmp_path, "coarse", "0", photons, rays, streams, True)
    for name, leg in (("on", on), ("off", off)):
        _check_against_oracle("coarse map, rule " + name, leg["out"], leg["draws"], leg["end"], d)
        _check_against_oracle("coarse map, rule %s, counters on" % name, leg["sout"], leg["sdraws"], leg["send"], d)
        print("coarse map, rule %s:" % name, {k: leg["stats"][k] for k in ("n_steps", "n_tested", "group_attempts", "n_guess_retries")})
    floor = 1e-6 * float(np.abs(d["ref"][:, :3]).max())
    assert rel_l2(on["out"][:, :3], off["out"][:, :3], floor=floor).max() <= TOL
    assert (on["draws"] == off["draws"]).all() and (on["end"] == off["end"]).all()
    assert on["stats"]["n_tested"] == off["stats"]["n_tested"]


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2], sys.argv[3])
