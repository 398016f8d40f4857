"""The oracle's specular recursion against the reference's own records at "maxspeculardepth" 1, 2, 3 and 5 (tests/golden/
render_sph_surf_d1 / _d2, render_sphkr_surf_d3 / _d5: oracle/ref_capture `render ... surface ... surfspecdepth N`), the last two on a
glass with a reflective lobe: the samples own trees of spawned rays, not chains.  Bit for bit, as test_specular_recursion_matches_
reference; and every capture is shown, from the oracle's per-sample counts, to hold what it is for."""
import numpy as np
import pytest

from specular_depth_cases import DEPTH_CAPTURES, capture_depth, coverage, load_depth_capture, oracle_render


def _oracle(orc, name, depth=None):
    s, p, cam, film, smp, c = load_depth_capture(name)
    d = capture_depth(c) if depth is None else depth
    r = oracle_render(orc, s, p, cam, film, smp, c["tasks"], int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), d,
                      bool(c["surf.params.i"][1]))
    return r, c


@pytest.mark.parametrize("name", list(DEPTH_CAPTURES))
def test_specular_recursion_at_this_depth_matches_reference(orc, name):
    """integrators/photonmap.cpp:310 (`ray.depth+1 < maxSpecularDepth`) at the depth the capture was made with: draws in front of
    every volume Li(), stream ends, surface radiance, composed radiance and film are the reference's, bit for bit."""
    r, c = _oracle(orc, name)
    assert capture_depth(c) == DEPTH_CAPTURES[name][1]
    assert r["n_samples"] == len(c["samples.time"]) > 0
    np.testing.assert_array_equal(r["rays"]["rng_skip"], c["rays.skip"])
    np.testing.assert_array_equal(r["end_draws"], c["task.end_draw"])
    np.testing.assert_array_equal(r["surf_xyz"].ravel(), c["surf.xyz"])
    np.testing.assert_array_equal(r["xyzT"].ravel(), c["xyzT"])
    np.testing.assert_array_equal(r["pixels"].ravel(), c["film.pixels"])
    assert np.isfinite(c["film.pixels"]).all() and c["film.pixels"].max() > 0


@pytest.mark.parametrize("name", list(DEPTH_CAPTURES))
def test_each_capture_holds_what_it_is_for(orc, name):
    """Depth 1: no sample owns a segment (and a matte hit draws 144 or 145, not 150 or 151: SpecularReflect / SpecularTransmit are
    not entered).  Depth d >= 2: at least 20 samples reach level d - 1.  Reflective glass: at least 20 samples in which one glass hit
    spawned both lobes, and in those the sample owns more segments than its deepest level (a tree, not a chain)."""
    r, c = _oracle(orc, name)
    d = DEPTH_CAPTURES[name][1]
    seg, lvl, both = r["spec_segments"], r["spec_depth"], r["spec_both"]
    n_seg, levels, n_both = coverage(r)
    print(name, "samples with segments", n_seg, "deepest level -> samples", levels, "samples with a two-lobe hit", n_both,
          "segments", int(seg.sum()))
    assert (lvl <= max(d - 1, 0)).all() and (seg >= lvl).all()
    if d == 1:
        assert n_seg == 0 and (seg == 0).all() and (lvl == 0).all()
        assert set(np.unique(c["surf.draws"])) <= {0, 144, 145, 146}     # 2 x rho + one draw per unoccluded light (two lights)
        assert (c["surf.draws"] >= 144).sum() > 500
    else:
        assert levels.get(d - 1, 0) >= 20, levels
    if DEPTH_CAPTURES[name][0] == "sphereroom_kr":
        assert n_both >= 20
        assert (seg[both > 0] > lvl[both > 0]).all()
    else:
        assert n_both == 0 and (seg == lvl).all()                         # Kr = 0: a chain


@pytest.mark.parametrize("name,wrong", [("sph_surf_d1", 2), ("sph_surf_d2", 1), ("sph_surf_d2", 3), ("sphkr_surf_d3", 2), ("sphkr_surf_d3", 4),
                                        ("sphkr_surf_d5", 4)])
def test_a_neighbouring_depth_does_not_pass(orc, name, wrong):
    """The captures tell the depths apart: the oracle at the depth next to the capture's misses its draw counts, its stream ends and
    its surface radiance.  (What keeps a constant in place of the parameter from passing the test above.)"""
    r, c = _oracle(orc, name, depth=wrong)
    assert (r["rays"]["rng_skip"] != c["rays.skip"]).sum() >= 20
    assert (r["end_draws"] != c["task.end_draw"]).any()
    assert (r["surf_xyz"].ravel() != c["surf.xyz"]).any()
