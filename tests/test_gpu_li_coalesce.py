"""Per-sample calls in device batches: pvol_li_many, and the coalescer behind concurrent pvol_li calls on one context.

A batch of n calls is n one-ray streams, each with its caller's live MT19937 state, through the same sliced path a lone pvol_li
takes, so every call must give the bytes a lone pvol_li gives on the same input, whatever else is in its batch.  Lone pvol_li is
held to the reference's records by test_gpu_parity.py and test_gpu_shim.py; here the batches are held to lone pvol_li, byte for
byte, and freshly seeded calls also to the oracle."""
import ctypes as C
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import GOLD, LI_CASES, ROOT, abi, blob, load_li_case, load_photons, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = ["vh", "vh_k500", "grid16", "rainbow", "pf_k50", "vhg", "mesh", "sph"]


@pytest.fixture(scope="module")
def pvol():
    m = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert m.lib().pvol_device_count() >= 1, "no HIP device: the product has no CPU path"
    return m


def mt_seeded(seed):
    """RNG(seed)'s table before its first draw (core/rng.cpp:41-49); mti is then 624."""
    mt = np.zeros(624, np.uint32)
    mt[0] = seed
    for i in range(1, 624):
        mt[i] = (1812433253 * (int(mt[i - 1]) ^ (int(mt[i - 1]) >> 30)) + i) & 0xffffffff
    return mt


def _ctx(pvol, case):
    s, p, rays, streams, c = load_li_case(case)
    tag = LI_CASES[case][1]
    pv = pvol.PhotonVolume(p)
    holder = abi.SceneHolder(s)
    pv.set_scene(holder)
    ph = load_photons(tag) if tag else None
    if ph is not None:
        pv.upload_photons(*ph)
    rays = rays.copy()
    rays["rng_skip"] = 0
    return pv, s, p, holder, ph, rays


def _lone(pv, rays, mt, mti):
    """Call i alone through pvol_li (coalescing off): Lv, T, final mt, final mti."""
    n = len(rays)
    Lv, T, mt = np.zeros((n, 30), np.float32), np.zeros((n, 30), np.float32), mt.copy()
    mti = np.asarray(mti, np.int32).copy()
    for i in range(n):
        row = mt[i].copy()
        Lv[i], T[i], mti[i] = pv.li_single(rays[i:i + 1], row, int(mti[i]))
        mt[i] = row
    return Lv, T, mt, mti


def _states(pv, rays, n, seed0):
    """n states: even rows freshly seeded (mti 624), odd rows advanced part-way by one earlier call (mti < 624)."""
    mt = np.stack([mt_seeded(seed0 + i) for i in range(n)])
    mti = np.full(n, 624, np.int32)
    for i in range(1, n, 2):
        row = mt[i].copy()
        _, _, m = pv.li_single(rays[(i + 7) % len(rays):(i + 7) % len(rays) + 1], row, 624)
        mt[i], mti[i] = row, m
        assert 0 <= m < 624
    return mt, mti


def _pick(rays, n):
    return rays[np.arange(n) % len(rays)].copy()


@pytest.mark.parametrize("case", CASES)
def test_li_many_equals_lone_pvol_li_bit_for_bit(pvol, orc, case):
    pv, s, p, holder, ph, rays = _ctx(pvol, case)
    n = 24
    rays = _pick(rays, n)
    mt0, mti0 = _states(pv, rays, n, 500)
    lv_l, t_l, mt_l, mti_l = _lone(pv, rays, mt0, mti0)
    mt = mt0.copy()
    pv.li_coalescing_stats(reset=True)
    Lv, T, mti, status = pv.li_many(rays, mt, mti0)
    assert (status == abi.PVOL_OK).all()
    assert pv.li_coalescing_stats()["batches_redone"] == 0   # the hand-over backup's gate stayed closed: one batch served all
    assert Lv.tobytes() == lv_l.tobytes() and T.tobytes() == t_l.tobytes()
    assert mt.tobytes() == mt_l.tobytes() and mti.tobytes() == mti_l.tobytes()
    # freshly seeded rows against the oracle: radiance at the suite's bar, the RNG state exact
    o = orc.Oracle(holder, p)
    if ph is not None:
        o.set_photons(*ph)
    L = orc.lib()
    for i in range(0, n, 2):
        st = abi.make_streams(np.array([500 + i], np.uint32), np.array([1], np.uint32))
        ref, rdraws = o.li_batch(rays[i:i + 1], st)
        scale = max(float(np.linalg.norm(ref[0, :30])), 1e-30)
        assert rel_l2(Lv[i:i + 1], ref[:, :30], floor=1e-3 * scale).max() <= TOL, i
        assert rel_l2(T[i:i + 1], ref[:, 30:]).max() <= 1e-5, i
        total = int(rdraws[0])
        assert mti[i] == total % 624 or (mti[i] == 624 and total % 624 == 0)
        if mti[i] < 624:   # the state continues the reference's sequence: draw #total of RNG(seed)
            seq = np.zeros(total + 1, np.uint32)
            L.orc_rng_draws(500 + i, total + 1, seq.ctypes.data_as(C.POINTER(C.c_uint32)))
            y = int(mt[i, mti[i]])
            y ^= y >> 11
            y ^= (y << 7) & 0x9d2c5680
            y ^= (y << 15) & 0xefc60000
            y ^= y >> 18
            assert y == int(seq[total]), i
    pv.close()


@pytest.mark.parametrize("case", ["vh", "vh_k500", "grid16", "pf_k50", "sph"])
def test_a_calls_bits_do_not_depend_on_its_companions(pvol, case):
    pv, s, p, holder, ph, rays = _ctx(pvol, case)
    n = 96
    rays = _pick(rays, n)
    mt0, mti0 = _states(pv, rays, n, 900)

    def run(order, size):
        Lv, T = np.zeros((n, 30), np.float32), np.zeros((n, 30), np.float32)
        mt, mti = mt0.copy(), mti0.copy()
        for b in range(0, n, size):
            idx = order[b:b + size]
            sub_mt = mt0[idx].copy()
            lv, t, m, status = pv.li_many(rays[idx], sub_mt, mti0[idx])
            assert (status == abi.PVOL_OK).all()
            Lv[idx], T[idx], mt[idx], mti[idx] = lv, t, sub_mt, m
        return Lv.tobytes() + T.tobytes() + mt.tobytes() + mti.tobytes()

    ident = np.arange(n)
    pv.li_coalescing_stats(reset=True)
    want = run(ident, n)
    rng = np.random.default_rng(7)
    for size in (1, 7, 64, n):
        assert run(ident, size) == want, size
        assert run(rng.permutation(n), size) == want, ("shuffled", size)
    assert pv.li_coalescing_stats()["batches_redone"] == 0
    # two rows holding the same state are two independent calls
    mt = np.stack([mt0[3], mt0[3]])
    lv, t, m, status = pv.li_many(rays[[3, 3]], mt, mti0[[3, 3]])
    assert lv[0].tobytes() == lv[1].tobytes() and mt[0].tobytes() == mt[1].tobytes() and m[0] == m[1]
    pv.close()


N_THREADS, PER = 16, 24


def _thread_inputs(rays):
    return {t: (rays[(t * PER + np.arange(PER)) % len(rays)].copy(), mt_seeded(100 + t)) for t in range(N_THREADS)}


def _serial(pv, inputs):
    out = {}
    for t, (rs, mt0) in inputs.items():
        mt, mti, rows = mt0.copy(), 624, []
        for k in range(PER):
            Lv, T, mti = pv.li_single(rs[k:k + 1], mt, mti)
            rows.append(np.concatenate([Lv, T]))
        out[t] = (np.stack(rows).tobytes(), mt.tobytes(), mti)
    return out


def _concurrent(pvol, pv, inputs, bad_thread=None):
    got, errs = {}, {}
    barrier = threading.Barrier(N_THREADS)

    def worker(t):
        rs, mt0 = inputs[t]
        mt, mti, rows = mt0.copy(), 624, []
        barrier.wait()
        try:
            for k in range(PER):
                if t == bad_thread and k == PER // 2:
                    with pytest.raises(pvol.PvolError) as e:
                        pv.li_single(rs[k:k + 1], mt.copy(), 700)
                    errs[t] = e.value.status
                Lv, T, mti = pv.li_single(rs[k:k + 1], mt, mti)
                rows.append(np.concatenate([Lv, T]))
            got[t] = (np.stack(rows).tobytes(), mt.tobytes(), mti)
        except BaseException as e:   # reported below, on the main thread
            errs[t] = e

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(N_THREADS)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    return got, errs


@pytest.mark.parametrize("case", ["pf_k50", "vh"])
def test_concurrent_pvol_li_is_coalesced_and_unchanged(pvol, case):
    pv, s, p, holder, ph, rays = _ctx(pvol, case)
    inputs = _thread_inputs(rays)
    want = _serial(pv, inputs)
    pv.set_li_coalescing(64, 200)
    pv.li_coalescing_stats(reset=True)
    got, errs = _concurrent(pvol, pv, inputs)
    assert errs == {}
    for t in range(N_THREADS):
        assert got[t] == want[t], t
    st = pv.li_coalescing_stats()
    assert st["calls"] == N_THREADS * PER
    assert st["batches"] < st["calls"] and st["largest_batch"] > 1, st
    assert st["batches_redone"] == 0 and st["calls_failed"] == 0, st
    # a bad call fails alone, before it joins a batch; the other calls keep their bytes
    got, errs = _concurrent(pvol, pv, inputs, bad_thread=5)
    assert errs == {5: abi.PVOL_E_INVALID}
    for t in range(N_THREADS):
        assert got[t] == want[t], t
    # off means off: nothing goes through the coalescer any more, and the bytes stay
    pv.set_li_coalescing(0, 0)
    pv.li_coalescing_stats(reset=True)
    got, errs = _concurrent(pvol, pv, inputs)
    assert errs == {}
    for t in range(N_THREADS):
        assert got[t] == want[t], t
    assert pv.li_coalescing_stats() == {"calls": 0, "batches": 0, "largest_batch": 0, "queued_behind": 0, "batches_redone": 0, "calls_failed": 0}
    pv.close()


def test_limits_and_errors_of_the_batched_entry_points(pvol):
    pv, s, p, holder, ph, rays = _ctx(pvol, "vh")
    L = pvol.lib()
    for bad in [(4097, 0), (64, 1001)]:
        assert L.pvol_set_li_coalescing(pv._h, *bad) == abi.PVOL_E_INVALID
    pv.set_li_coalescing(4096, 1000)
    pv.set_li_coalescing(1, 0)
    mt = np.stack([mt_seeded(1), mt_seeded(2)])
    with pytest.raises(pvol.PvolError) as e:
        pv.li_many(rays[:2], mt, np.array([624, 625], np.int32))
    assert e.value.status == abi.PVOL_E_INVALID
    assert mt.tobytes() == np.stack([mt_seeded(1), mt_seeded(2)]).tobytes()
    # no scene yet: every call of the batch reports it
    q = pvol.PhotonVolume(p)
    Lv, T, mti, status = q.li_many(rays[:2], mt, np.array([624, 624], np.int32))
    assert (status == abi.PVOL_E_NO_SCENE).all()
    q.close()
    pv.close()


def test_a_ray_beyond_the_record_plan_fails_alone(pvol):
    """PVOL_E_LIMIT inside a batch: a ray whose march needs more steps than the record plan holds (its direction scaled down, so
    the same segment is 1000 times as many steps of the parameter) fails on its own.  Its state is left as it was, its companions
    keep the bytes of lone calls, and the error does not reach the context's shared count (pvol_check_errors)."""
    pv, s, p, holder, ph, rays = _ctx(pvol, "vh")
    n = 12
    rays = _pick(rays, n)
    mt0, mti0 = _states(pv, rays, n, 1300)
    lv_l, t_l, mt_l, mti_l = _lone(pv, rays, mt0, mti0)
    hit = int(np.argmax(np.abs(lv_l).sum(1) > 0))
    assert np.abs(lv_l[hit]).sum() > 0
    bad = rays.copy()
    bad["d"][hit] = bad["d"][hit] / 1000.0
    bad["mint"][hit] *= 1000.0
    bad["maxt"][hit] = min(float(bad["maxt"][hit]) * 1000.0, 3.0e38)
    with pytest.raises(pvol.PvolError) as e:   # the lone call: as before, through the shared count
        pv.li_single(bad[hit:hit + 1], mt0[hit].copy(), int(mti0[hit]))
    assert e.value.status == abi.PVOL_E_LIMIT
    pv.li_coalescing_stats(reset=True)
    mt = mt0.copy()
    Lv, T, mti, status = pv.li_many(bad, mt, mti0)
    assert status[hit] == abi.PVOL_E_LIMIT and (np.delete(status, hit) == abi.PVOL_OK).all()
    assert mt[hit].tobytes() == mt0[hit].tobytes() and mti[hit] == mti0[hit]
    keep = np.arange(n) != hit
    assert Lv[keep].tobytes() == lv_l[keep].tobytes() and T[keep].tobytes() == t_l[keep].tobytes()
    assert mt[keep].tobytes() == mt_l[keep].tobytes() and mti[keep].tobytes() == mti_l[keep].tobytes()
    assert pvol.lib().pvol_check_errors(pv._h) == abi.PVOL_OK
    # the same through the coalescer
    pv.set_li_coalescing(8, 0)
    with pytest.raises(pvol.PvolError) as e:
        pv.li_single(bad[hit:hit + 1], mt0[hit].copy(), int(mti0[hit]))
    assert e.value.status == abi.PVOL_E_LIMIT
    assert pvol.lib().pvol_check_errors(pv._h) == abi.PVOL_OK
    st = pv.li_coalescing_stats()
    assert st["calls_failed"] == 2 and st["batches_redone"] == 0, st
    pv.close()


def test_a_batch_runs_after_device_work_still_in_flight(pvol):
    """pvol_li_batch_device returns with its kernels running on the default stream, and they use the context's scratch
    (chunk counters, hand-over list) that a batch of pvol_li_many also uses: the batch must run after them.  A large device
    batch is enqueued and li_many called at once; both results must equal those of the two run one after the other."""
    import torch
    pv, s, p, holder, ph, rays = _ctx(pvol, "vh")   # li_group_kernel + hand-over list on both sides, about 2 ms of device batch
    n_dev, n_str = 1 << 18, 256
    drays = _pick(rays, n_dev)
    per = n_dev // n_str
    streams = abi.make_streams(np.arange(7, 7 + n_str, dtype=np.uint32), np.full(n_str, per, np.uint32))
    d_rays = torch.from_numpy(drays.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n_dev * 60, dtype=torch.float32, device="cuda")

    def device_batch():
        d_streams = torch.from_numpy(streams.copy().view(np.uint8)).cuda()
        d_out.zero_()
        torch.cuda.synchronize()
        pv.li_device(d_rays.data_ptr(), n_dev, d_streams.data_ptr(), n_str, abi.OUT_SPECTRAL, d_out.data_ptr(), 0, 0)
        return d_streams

    n = 32
    mrays = _pick(rays, n)
    mt0, mti0 = _states(pv, mrays, n, 1700)
    # one after the other
    ds = device_batch()
    torch.cuda.synchronize()
    want_dev = d_out.cpu().numpy().reshape(n_dev, 60).copy()
    mt_w = mt0.copy()
    want = pv.li_many(mrays, mt_w, mti0)
    # overlapping: li_many enqueued while the device batch still runs
    ds = device_batch()
    mt = mt0.copy()
    got = pv.li_many(mrays, mt, mti0)
    torch.cuda.synchronize()
    del ds
    got_dev = d_out.cpu().numpy().reshape(n_dev, 60)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert mt.tobytes() == mt_w.tobytes()
    # the device batch's hand-over pass adds with atomics (its last bits may vary run to run); a race on its scratch drops or
    # doubles whole rays
    scale = float(np.linalg.norm(want_dev[:, :30], axis=1).max())
    assert rel_l2(got_dev[:, :30], want_dev[:, :30], floor=1e-3 * max(scale, 1e-30)).max() <= 1e-5
    assert rel_l2(got_dev[:, 30:], want_dev[:, 30:]).max() <= 1e-6
    assert pvol.lib().pvol_check_errors(pv._h) == abi.PVOL_OK
    pv.close()


TOOL = os.path.join(ROOT, "oracle", "_ref", "shim_drive")


@pytest.mark.skipif(not os.path.exists(TOOL), reason="oracle/_ref/shim_drive is not built (needs the reference tree at build time)")
@pytest.mark.parametrize("name", ["vh", "vh_sparse", "vh_k500", "vh_nomap", "rainbow", "grid16", "pf", "pf_k50", "vhg", "mesh", "sph"])
def test_binding_li_through_the_coalescer(name, tmp_path):
    """The unchanged binding, its context's coalescing switched on from the environment (PVOL_LI_COALESCE).  shim_drive calls
    Li() from one thread, so every batch here holds one call: this checks the binding through the coalescer's n = 1 path (the
    queue, the staging, the context's stream), not the gathering of concurrent calls -- that is
    test_concurrent_pvol_li_is_coalesced_and_unchanged."""
    scene, tag = LI_CASES[name]
    out = str(tmp_path / "shim_out.bin")
    photons = os.path.join(GOLD, "photons_%s.bin" % tag) if tag else "-"
    env = dict(os.environ, PVOL_LI_COALESCE="64")
    r = subprocess.run([TOOL, "li", scene, photons, os.path.join(GOLD, "li_%s.bin" % name), out], timeout=600, capture_output=True,
                       text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    o = blob.load(out)
    np.testing.assert_array_equal(o["hip.draws"], o["ref.draws"])
    np.testing.assert_array_equal(o["hip.next_rng"], o["ref.next_rng"])
    ref, hip = o["ref.Lv"].reshape(-1, 30), o["hip.Lv"].reshape(-1, 30)
    scale = np.linalg.norm(ref.astype(np.float64), axis=1).max()
    assert rel_l2(hip, ref, floor=1e-3 * max(scale, 1e-30)).max() <= 1e-4
    assert rel_l2(o["hip.T"].reshape(-1, 30), o["ref.T"].reshape(-1, 30)).max() <= 1e-5
