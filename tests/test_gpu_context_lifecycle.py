"""A context's whole life, several times over: create, use everything that makes events, a stream or pinned memory on first use
(batch timing pairs, phase marks, the coalescer's stream and staging), close -- the last time with a batch still in flight -- and a
context created afterwards must give what the first one gave, byte for byte.  The contexts are created under PVOL_NO_GROUP=1: that
path has no float atomics.  70 unsynchronised device batches on one stream also take the timer's more-than-64-in-flight branch, and
every one of them must be counted exactly once."""
import importlib

import numpy as np
import pytest

from conftest import abi, load_li_case, load_photons
from test_gpu_li_coalesce import mt_seeded

pytestmark = pytest.mark.gpu
CYCLES, IN_FLIGHT, N_DEV = 3, 70, 64


def test_create_use_close_cycles_then_a_fresh_context(monkeypatch):
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    assert pvol.lib().pvol_device_count() >= 1
    monkeypatch.setenv("PVOL_NO_GROUP", "1")
    s, p, rays, streams, _ = load_li_case("vh")
    photons = load_photons("vh")
    assert len(rays) >= N_DEV and int(streams["n_rays"][0]) < N_DEV   # the device batch: a whole stream and the head of the next

    def context():
        pv = pvol.PhotonVolume(p)
        pv.enable_phase_timing(True)
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*photons)
        return pv

    def li(pv):
        st = streams.copy()
        out, draws = pv.li(rays, st)
        return out, draws, st["end_draw"].copy()

    many_rays = rays[:2].copy()
    many_rays["rng_skip"] = 0
    counts = np.diff(np.minimum(np.concatenate([[0], np.cumsum(streams["n_rays"])]), N_DEV))
    k = int((counts > 0).sum())
    dev_streams = abi.make_streams(streams["seed"][:k], counts[:k], streams["start_draw"][:k])
    d_rays = torch.from_numpy(np.ascontiguousarray(rays[:N_DEV]).view(np.uint8).copy()).cuda()
    d_streams = torch.from_numpy(dev_streams.view(np.uint8).copy()).cuda()
    d_out = torch.zeros((N_DEV, 60), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()   # the uploads above, before anything runs on the side stream

    def device_batch(pv):
        pv.li_device(d_rays.data_ptr(), N_DEV, d_streams.data_ptr(), k, abi.OUT_SPECTRAL, d_out.data_ptr(), 0, side.cuda_stream)

    first = first_many = None
    for cycle in range(CYCLES):
        pv = context()
        try:
            got = li(pv)
            mt = np.stack([mt_seeded(11), mt_seeded(12)])
            Lv, T, mti, status = pv.li_many(many_rays, mt, np.array([624, 624], np.int32))   # the coalescer's stream and pinned staging
            assert (status == abi.PVOL_OK).all()
            many = (Lv, T, mti, mt)
            if first is None:
                first, first_many = got, many
                assert np.abs(first[0][:, :30]).sum() > 0 and first[1].sum() > 0
            for g, w in zip(got + many, first + first_many):
                np.testing.assert_array_equal(g, w)
            pv.kernel_time_ms(reset=True)
            for _ in range(IN_FLIGHT):   # no synchronisation in between: more than 64 pairs in flight
                device_batch(pv)
            avg, launches = pv.kernel_time_ms()
            assert launches == IN_FLIGHT and avg > 0
            assert pv.phase_ms()["march_gather"] > 0
            if cycle == CYCLES - 1:
                device_batch(pv)   # close() synchronises the device; the tensors outlive the context
        finally:
            pv.close()
    torch.cuda.synchronize()
    assert torch.isfinite(d_out).all() and float(d_out[:, :30].abs().sum()) > 0

    pv = context()
    try:
        for g, w in zip(li(pv), first):
            assert g.tobytes() == w.tobytes()
    finally:
        pv.close()
