"""The specular recursion on the device (pvol_spec_dev.h, the two walkers of pvol_tile_dev.h, spec_compose_kernel) at every
"maxspeculardepth" the host accepts, on trees as well as chains, and at the edge of its segment pool.

Against the reference's own records at depths 1, 2, 3 and 5 (tests/golden/render_sph_surf_d1 / _d2, render_sphkr_surf_d3 / _d5;
two lights: the FUSED pre-pass and the sliced path) and against the oracle -- which tests/test_specular_depth.py holds to those
records bit for bit -- on the same scene with one light (the COUNT pre-pass and the ray-parallel path) at depths 0 to 5.
Bars: rng_skip and end_draw exact; surf_xyz and T * Ls + Lvi <= 1e-4 relative L2 per sample; film rtol 1e-4, atol 1e-5 max.
No sample is left out of any comparison."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import abi, load_photons
from specular_depth_cases import (DEPTH_CAPTURES, PHOTONS, capture_depth, coverage, load_caustic, load_depth_capture, one_light,
                                  oracle_render)
from test_gpu_render import _check_surface_capture, _pvol, _rel_l2, _render_surface
from test_launch_plan import BatchPlan, Knobs, PlanIn

pytestmark = pytest.mark.gpu

TREE = "sphkr_surf_d5"   # the frame every oracle comparison below renders: 4 tasks, 1 296 camera samples, one batch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        torch.cuda.init()   # raises with the reason
    return torch


def _context(s, p, n_used, max_dist, depth, final_gather=False):
    caustic, n_paths = load_caustic()
    pv = _pvol().PhotonVolume(p)
    try:
        pv.set_scene(abi.SceneHolder(s))
        pv.upload_photons(*load_photons(PHOTONS))
        pv.set_surface_integrator(n_used, max_dist, depth, final_gather, caustic, n_paths)
    except Exception:
        pv.close()
        raise
    return pv


def _capture_context(name):
    s, p, cam, film, smp, c = load_depth_capture(name)
    pv = _context(s, p, int(c["surf.params.i"][0]), float(c["surf.params.f"][0]), capture_depth(c), bool(c["surf.params.i"][1]))
    return pv, cam, film, smp, c


def _check_against_oracle(r, ro):
    np.testing.assert_array_equal(r["xy"], ro["image_xy"])
    np.testing.assert_array_equal(r["rays"]["maxt"], ro["rays"]["maxt"])
    np.testing.assert_array_equal(r["rays"]["rng_skip"], ro["rays"]["rng_skip"])   # sampler draws + the surface integrator's whole tree
    np.testing.assert_array_equal(r["streams"]["end_draw"], ro["end_draws"])
    err = _rel_l2(r["surf_xyz"], ro["surf_xyz"].reshape(-1, 3))
    assert err.max() <= 1e-4, "surface Li per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    err = _rel_l2(r["xyzT"][:, :3], ro["xyzT"].reshape(-1, 4)[:, :3])
    assert err.max() <= 1e-4, "T * Ls + Lvi per-sample rel L2 %.3g at %d" % (err.max(), err.argmax())
    np.testing.assert_allclose(r["pixels"], ro["pixels"], rtol=1e-4, atol=1e-5 * np.abs(ro["pixels"]).max())


# ---------------------------------------------------------------- the reference's records: FUSED pre-pass, sliced path
@pytest.mark.parametrize("name", list(DEPTH_CAPTURES))
def test_depth_captures_match_reference(torch_cuda, name):
    """`D + 1 < maxSpecularDepth` in spec_surface, the +6 draws of a matte hit in surf_count_draws(..., D), specOn at depth <= 1 and the
    acc[] ladder of spec_compose_kernel on trees that stop early, at the depth the reference made the capture with."""
    pv, cam, film, smp, c = _capture_context(name)
    try:
        assert capture_depth(c) == DEPTH_CAPTURES[name][1]
        r = _render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], len(c["samples.time"]))
        assert pv.tile_kernel_name() == "tile_kernel<fused>"   # two lights
        _check_surface_capture(r, c, film)
    finally:
        pv.close()


def test_tree_capture_in_several_slices(torch_cuda, monkeypatch):
    """The same records with slices of 64 rays per task: the pool is emptied in front of every slice and a composed sample's link
    carries SPEC_LINK_DONE, so a later slice that reuses its slots does not fold them in again."""
    pv, cam, film, smp, c = _capture_context(TREE)
    try:
        monkeypatch.setenv("PVOL_SLICE_RAYS", "64")
        r = _render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], len(c["samples.time"]))
        _check_surface_capture(r, c, film)
    finally:
        pv.close()


# ---------------------------------------------------------------- the oracle: COUNT pre-pass, ray-parallel path
_ORACLE = {}


def _frame(two_lights=False, kr=None, kt=None):
    s, p, cam, film, smp, c = load_depth_capture(TREE)
    if not two_lights:
        s = one_light(s, kr, kt)
    return s, p, cam, film, smp, c


def _oracle(orc, depth, two_lights=False, kr=None, kt=None):
    """Computed once per (scene, depth), shared and read-only."""
    key = (depth, two_lights, kr, kt)
    if key not in _ORACLE:
        s, p, cam, film, smp, c = _frame(two_lights, kr, kt)
        n_used, max_dist = (int(c["surf.params.i"][0]), float(c["surf.params.f"][0])) if two_lights else (50, 0.15)
        _ORACLE[key] = oracle_render(orc, s, p, cam, film, smp, c["tasks"], n_used, max_dist, depth)
        _ORACLE[key]["pixels"].setflags(write=False)
    return _ORACLE[key]


def _glass_samples(orc, s, p, rays):
    """Camera samples whose primary ray ends on glass (the oracle's Scene::Intersect)."""
    o = orc.Oracle(abi.SceneHolder(s), p)
    try:
        f, i = o.hits(rays["o"], rays["d"], np.zeros(len(rays), np.float32), np.full(len(rays), np.inf, np.float32))
    finally:
        o.close()
    return (f[:, 1] > 0) & (s["mats.kind"][i[:, 1]] == abi.MATERIAL_GLASS)


def _render_one_light(torch, orc, depth, kr=None, kt=None):
    s, p, cam, film, smp, c = _frame(False, kr, kt)
    ro = _oracle(orc, depth, False, kr, kt)
    pv = _context(s, p, 50, 0.15, depth)
    try:
        r = _render_surface(torch, pv, cam, film, smp, c["tasks"], ro["n_samples"])
        assert pv.march_kernel_name() == "li_group_kernel" and pv.tile_kernel_name() not in ("", "tile_kernel<fused>"), pv.tile_kernel_name()
    finally:
        pv.close()
    return r, ro, (s, p)


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4, 5])
def test_one_light_tree_matches_oracle_at_every_depth(torch_cuda, orc, depth):
    """sphereroom_kr without its point light: one camera sample per lane counts its tree's draws and lays its segments out
    (tile_surface_draws), li_par_kernel marches them, spec_compose_kernel folds them back.  At depth d >= 2 at least 20 samples own
    a tree that reaches level d - 1; at depths 0 and 1 the oracle spawns nothing and glass gives no radiance."""
    r, ro, (s, p) = _render_one_light(torch_cuda, orc, depth)
    n_seg, levels, n_both = coverage(ro)
    if depth >= 2:
        assert levels.get(depth - 1, 0) >= 20 and n_both >= 20, (levels, n_both)
    else:
        assert (ro["spec_segments"] == 0).all() and (ro["spec_depth"] == 0).all()
        glass = _glass_samples(orc, s, p, ro["rays"])
        assert glass.sum() >= 20
        assert (r["surf_xyz"][glass] == 0).all() and (ro["surf_xyz"][glass] == 0).all()
    _check_against_oracle(r, ro)


def test_depths_0_and_1_agree(torch_cuda, orc):
    """Neither enters SpecularReflect / SpecularTransmit (0 + 1 < 0 and 0 + 1 < 1 are both false): the same draws, the same radiance."""
    r0, o0, _ = _render_one_light(torch_cuda, orc, 0)
    r1, o1, _ = _render_one_light(torch_cuda, orc, 1)
    np.testing.assert_array_equal(o0["rays"]["rng_skip"], o1["rays"]["rng_skip"])
    np.testing.assert_array_equal(o0["xyzT"], o1["xyzT"])
    np.testing.assert_array_equal(r0["rays"]["rng_skip"], r1["rays"]["rng_skip"])
    np.testing.assert_array_equal(r0["streams"]["end_draw"], r1["streams"]["end_draw"])
    assert _rel_l2(r0["surf_xyz"], r1["surf_xyz"]).max() <= 1e-4
    assert _rel_l2(r0["xyzT"][:, :3], r1["xyzT"][:, :3]).max() <= 1e-4
    np.testing.assert_allclose(r0["pixels"], r1["pixels"], rtol=1e-4, atol=1e-5 * np.abs(r1["pixels"]).max())


@pytest.mark.parametrize("kr,kt", [(0.25, 0.0), (0.0, None)], ids=["reflection_only", "transmission_only"])
def test_one_lobe_at_a_time_matches_oracle(torch_cuda, orc, kr, kt):
    """Depth 5.  Kt = 0, Kr = 0.25: GlassMaterial adds the reflective lobe alone (glass.cpp:52-57), SpecularTransmit still draws
    its BSDFSample (3 numbers) before Sample_f finds no lobe -- spec_lobe with lobe == 1 and the reflection branch of spec_fresnel on
    their own.  Kr = 0: the chain of the scene file."""
    r, ro, _ = _render_one_light(torch_cuda, orc, 5, kr, kt)
    n_seg, levels, n_both = coverage(ro)
    assert n_seg >= 20 and n_both == 0, (n_seg, n_both)
    if kt == 0.0:
        assert set(levels) == {0, 1}       # the ball is convex: a ray reflected off it meets no glass again
    else:
        assert set(levels) == {0, 2} and levels[2] >= 20   # in through the ball and out again: no internal reflection without Kr
    _check_against_oracle(r, ro)


# ---------------------------------------------------------------- the pool's edge
class _spec_pool:
    """PVOL_SPEC_POOL (pvol_read_knobs reads it at every launch: plan_input) for the length of a with block."""
    def __init__(self, value):
        self.value = str(int(value))

    def __enter__(self):
        self.old = os.environ.get("PVOL_SPEC_POOL")
        os.environ["PVOL_SPEC_POOL"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("PVOL_SPEC_POOL", None)
        else:
            os.environ["PVOL_SPEC_POOL"] = self.old


def _expect_limit(torch, pv, cam, film, smp, tasks, n):
    pvol = _pvol()
    with pytest.raises(pvol.PvolError) as e:
        _render_surface(torch, pv, cam, film, smp, tasks, n)
    assert e.value.status == abi.PVOL_E_LIMIT
    torch.cuda.synchronize()


def test_pool_edge_one_light(torch_cuda, orc):
    """COUNT pre-pass, depth 5, the frame in one batch.  A pool of exactly the batch's S segments serves every sample (`base + n <=
    segCap` at the last slot); one slot less is an error the caller sees (PVOL_E_LIMIT), not a darker film; and the same context
    renders the oracle's frame again once the knob is gone (error counter cleared, no stale link or pool state)."""
    s, p, cam, film, smp, c = _frame()
    ro = _oracle(orc, 5)
    S = int(ro["spec_segments"].sum())
    assert S > 64 and (ro["spec_segments"] > 0).sum() >= 20
    pv = _context(s, p, 50, 0.15, 5)
    try:
        with _spec_pool(S):
            _check_against_oracle(_render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], ro["n_samples"]), ro)
        with _spec_pool(S - 1):
            _expect_limit(torch_cuda, pv, cam, film, smp, c["tasks"], ro["n_samples"])
        assert "PVOL_SPEC_POOL" not in os.environ
        _check_against_oracle(_render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], ro["n_samples"]), ro)
    finally:
        pv.close()


def _fused_slices(pvol, smp, tasks, n, pool):
    """nSlices of the two-light frame's batch (pvol_plan_batch).  maxSteps is set far above the scene's (the record budget only
    shrinks a slice as it grows), the rest as the batch has it."""
    L = pvol.lib()
    L.pvol_plan_batch.argtypes = [C.POINTER(PlanIn), C.POINTER(BatchPlan)]
    L.pvol_plan_batch.restype = None
    i = PlanIn(nLights=2, volKind=1, g=0.0, nPhotons=4000, nUsed=50, candCap=(50 + 63) // 64 * 64 + 192, maxSteps=4096, nTris=6, nCU=256,
               groupWavesPerCU=12, fixWavesPerCU=16, nRays=n, nStreams=len(tasks), maxRays=max(pvol.render_sample_count(smp, [t]) for t in tasks),
               hasTile=1, spp=smp.pixel_samples, specOn=1, hasTauOut=1)
    i.knobs = Knobs(groupGuess=1.15, specPool=pool)
    out = BatchPlan()
    L.pvol_plan_batch(C.byref(i), C.byref(out))
    assert out.rc == abi.PVOL_OK and out.tile == 3 and out.specCap == pool   # PVOL_TILE_FUSED
    return out.nSlices


def test_pool_edge_two_lights(torch_cuda, orc):
    """The same pair through the FUSED pre-pass (the whole wave on one camera sample, SpecWalkPol): the frame is one slice, so S is
    the slice's count.  With S slots the reference's records; with S - 1 the status alone; then the records again."""
    pv, cam, film, smp, c = _capture_context(TREE)
    try:
        n = len(c["samples.time"])
        ro = _oracle(orc, 5, two_lights=True)
        S = int(ro["spec_segments"].sum())
        assert S > 64 and (ro["spec_segments"] > 0).sum() >= 20
        assert _fused_slices(_pvol(), smp, c["tasks"], n, S) == 1
        with _spec_pool(S):
            _check_surface_capture(_render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], n), c, film)
        with _spec_pool(S - 1):
            _expect_limit(torch_cuda, pv, cam, film, smp, c["tasks"], n)
        _check_surface_capture(_render_surface(torch_cuda, pv, cam, film, smp, c["tasks"], n), c, film)
    finally:
        pv.close()
