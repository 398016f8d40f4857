"""Ties tests/single_ref.py to the reference: in its photon-integrator setting (the three statements of single.cpp that differ turned
back into photonvolume.cpp's) it must reproduce Oracle.li_batch, which is pinned to the reference's captures, with no photons: draw
counts and stream ends exactly, Lv and T within the project's 1e-4 relative L2 per ray.  Measured: the largest error over the four
scenes is 7.1e-6 (pf 7.1e-6, vhg 1.3e-6, vh_nomap 1.0e-6, grid16 2.9e-7): the oracle sums radiance in float32, this file in float64."""
import numpy as np
import pytest

import single_ref
from conftest import abi, load_li_case

MAX_RAYS = 96   # per case: whole streams from the front of the golden batch, enough to cross several of them


def front_streams(rays, streams, limit):
    n = 0
    keep = 0
    for st in streams:
        if keep and n + int(st["n_rays"]) > limit:
            break
        n += int(st["n_rays"])
        keep += 1
    return rays[:n].copy(), streams[:keep].copy()


@pytest.mark.parametrize("case", ["vh_nomap", "pf", "vhg", "grid16"])   # one light, two lights, g != 0, a VolumeGrid
def test_photon_setting_reproduces_the_oracle_without_photons(orc, case):
    s, p, rays, streams, _ = load_li_case(case)
    rays, streams = front_streams(rays, streams, MAX_RAYS)
    holder = abi.SceneHolder(s)
    o = orc.Oracle(holder, p)
    ref, rdraws = o.li_batch(rays, streams.copy())
    got, draws, ends, _ = single_ref.li_batch(s, p.step_size, rays, streams, single_ref.oracle_occlusion(o), photon=True)
    np.testing.assert_array_equal(draws, rdraws)
    first = streams["start_draw"].astype(np.uint64)
    for i, st in enumerate(streams):
        a, b = int(st["first_ray"]), int(st["first_ray"]) + int(st["n_rays"])
        assert int(ends[i]) == int(first[i]) + int(rdraws[a:b].sum()) + int(rays["rng_skip"][a:b].sum())
    err = single_ref.row_error(got, ref)
    print("single_ref photon setting vs oracle, %s: %d rays, max rel L2 %.3g" % (case, len(rays), err.max()))
    assert err.max() <= 1e-4
    assert rdraws.max() > 4   # the batch marches


def test_mt19937_is_the_reference_stream():
    """core/rng.cpp seeded with 5489 starts 3499211612, 581869302 (the generator's published first outputs); skip() and the saved state
    continue the same stream."""
    r = single_ref.MT(seed=5489)
    assert [r.uint(), r.uint()] == [3499211612, 581869302]
    a = single_ref.MT(seed=7)
    seq = [a.uint() for _ in range(1500)]
    b = single_ref.MT(seed=7)
    b.skip(700)
    c = single_ref.MT(state=b.state())
    assert [c.uint() for _ in range(800)] == seq[700:]
