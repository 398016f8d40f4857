"""The moment form of li_group_kernel, host side: the gate pvol_moment_gate (how many Taylor terms of
exp(-delta_b L) carry an XYZ result below rounding, or none), the moment formula itself restated in float64 against the direct
30-bin sum on the committed map, and the plan's choice of the form.  Pure host arithmetic: needs no GPU."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_photons, load_scene

HOMOGENEOUS, GRID = 1, 2
MOMENTS = 3   # BatchPlan.groupForm, GRP_FORM_MOMENTS
EPS = 2.0 ** -25


class Knobs(C.Structure):
    _fields_ = [("sliceRays", C.c_int64), ("specPool", C.c_int64), ("tileBatchRays", C.c_int64), ("groupGuess", C.c_float),
                ("fxgWiden", C.c_float), ("fxgAim", C.c_float), ("fixExact", C.c_int32)]


class PlanIn(C.Structure):   # pvol_host.h; the three moment fields sit in what was padding in front of the knobs
    _fields_ = [("nLights", C.c_int32), ("volKind", C.c_int32), ("g", C.c_float), ("nPhotons", C.c_uint32), ("nUsed", C.c_int32),
                ("candCap", C.c_int32), ("maxSteps", C.c_int32), ("nTris", C.c_int32), ("roulette", C.c_int32), ("distant", C.c_int32),
                ("forceSeq", C.c_int32), ("noGroup", C.c_int32), ("noLite", C.c_int32), ("statsOn", C.c_int32),
                ("nCU", C.c_int32), ("groupWavesPerCU", C.c_int32), ("fixWavesPerCU", C.c_int32), ("tileWaves", C.c_int32),
                ("nRays", C.c_uint32), ("nStreams", C.c_uint32), ("maxRays", C.c_uint32), ("hasInit", C.c_int32), ("transOnly", C.c_int32),
                ("hasTile", C.c_int32), ("spp", C.c_uint32), ("specOn", C.c_int32), ("hasTauOut", C.c_int32),
                ("momentTerms", C.c_int16), ("outXYZ", C.c_int8), ("noMoments", C.c_int8), ("knobs", Knobs)]


class BatchPlan(C.Structure):
    _fields_ = [("rc", C.c_int32), ("path", C.c_int32), ("tile", C.c_int32), ("groupForm", C.c_int32), ("fixGroup", C.c_int32),
                ("liteResolve", C.c_int32), ("resolve", C.c_int32), ("recStride", C.c_uint32), ("sliceM", C.c_uint32), ("nSlices", C.c_uint32),
                ("nWaves", C.c_uint32), ("gWaves", C.c_uint32), ("fixWaves", C.c_uint32), ("tileWavesPerTask", C.c_int32),
                ("recBytes", C.c_uint64), ("stateBytes", C.c_uint64), ("deferWant", C.c_uint64), ("specCap", C.c_uint64),
                ("ldsSeq", C.c_uint64), ("ldsPar", C.c_uint64), ("ldsResolve", C.c_uint64), ("ldsGroup", C.c_uint64), ("ldsTile", C.c_uint64),
                ("kernel", C.c_char_p)]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    L = importlib.import_module("cs348b-pbrt_amd.pvol").lib()
    f32p = C.POINTER(C.c_float)
    L.pvol_moment_gate.argtypes = [f32p, f32p, C.c_double]
    L.pvol_moment_gate.restype = C.c_int
    L.pvol_plan_batch.argtypes = [C.POINTER(PlanIn), C.POINTER(BatchPlan)]
    L.pvol_plan_batch.restype = None
    return L


def gate(lib, sig_a, sig_s, bound):
    a, s = np.ascontiguousarray(sig_a, np.float32), np.ascontiguousarray(sig_s, np.float32)
    f32p = C.POINTER(C.c_float)
    return lib.pvol_moment_gate(a.ctypes.data_as(f32p), s.ctypes.data_as(f32p), float(bound))


@pytest.fixture(scope="module")
def c2():
    """The committed C2 scene's spectra and the diagonal of its medium's extent (15 x 5 x 10, v2w a translation): 18.7."""
    s = load_scene("volumescene_h")
    ext = s["vol.extent"].astype(np.float64)
    diag = float(np.linalg.norm(ext[3:] - ext[:3]))
    assert abs(diag - 18.708) < 1e-3
    return s, s["vol.sigma_a"].copy(), s["vol.sigma_s"].copy(), diag


def bound(x, n):
    return x ** n / math.factorial(n) * math.exp(x)


def sig_bar(sig_a, sig_s):
    """sigma_t's midrange as the float the kernels multiply by, and max |delta| (pvol_api.hip moment_sig_bar)."""
    t = (sig_a.astype(np.float32) + sig_s.astype(np.float32)).astype(np.float64)
    bar = float(np.float32(0.5 * (t.min() + t.max())))
    return bar, t - bar


def test_gate_on_the_c2_scene_is_three_terms(lib, c2):
    _, a, s, diag = c2
    _, delta = sig_bar(a, s)
    x = np.abs(delta).max() * diag
    assert bound(x, 2) > EPS > bound(x, 3)   # the issue's table: 5.5e-6 seen at two terms, bound 8.2e-9 at three
    assert gate(lib, a, s, diag) == 3


def test_gate_grey_medium_is_one_term(lib, c2):
    _, a, s, diag = c2
    grey_a, grey_s = np.full(30, a.mean(), np.float32), np.full(30, s.mean(), np.float32)   # delta scaled to zero
    assert np.ptp(grey_a + grey_s) == 0
    assert gate(lib, grey_a, grey_s, diag) == 1
    assert gate(lib, grey_a, grey_s, 1e9) == 1


def test_gate_refuses_a_coloured_medium(lib, c2):
    _, a, s, diag = c2
    f = np.linspace(0.8, 1.2, 30).astype(np.float32)   # sigma_t varying +-20 % over the bins
    assert gate(lib, a * f, s * f, diag) == 0
    assert gate(lib, a, s, float("inf")) == 0 and gate(lib, a, s, float("nan")) == 0 and gate(lib, a, s, -1.0) == 0


def test_gate_is_monotone_in_the_path_bound(lib, c2):
    _, a, s, diag = c2
    as_if = lambda n: 4 if n == 0 else n   # "none" is beyond three terms
    ns = [as_if(gate(lib, a, s, diag * k)) for k in (0.0, 1e-4, 1e-3, 1e-2, 0.1, 0.3, 1.0, 1.5, 2.0, 5.0, 30.0, 1e3, 1e6)]
    assert ns == sorted(ns)
    assert ns[0] == 1 and ns[-1] == 4
    assert set(ns) == {1, 2, 3, 4}


def test_moment_formula_matches_the_30_bin_sum(lib, c2):
    """Float64 restatement of what the kernel sums: X = stepD liiScale E sum_n kappa^n sum_members M_n[m], with M_n[m] = sum_b cie_b
    albedo_b (ln2 delta_b)^n / n! alpha[m][b], against sum_b cie_b albedo_b exp2(sigma_t_b kappa) sum_members alpha[m][b], over
    50-photon sums of the committed map and path lengths up to the bound: the relative error stays below the gate's own bound."""
    s, a, sg, diag = c2
    n_terms = gate(lib, a, sg, diag)
    assert n_terms == 3
    bar, delta = sig_bar(a, sg)
    x = np.abs(delta).max() * diag
    _, _, alpha = load_photons("vh")
    alpha = alpha.astype(np.float64)
    t = (a.astype(np.float32) + sg.astype(np.float32)).astype(np.float64)
    albedo = sg.astype(np.float64) / t
    cie = np.stack([s["cie.x"], s["cie.y"], s["cie.z"]]).astype(np.float64)              # [3][30]
    ln2d = math.log(2.0) * delta
    W = np.stack([cie * albedo * ln2d ** n / math.factorial(n) for n in range(n_terms)])   # [n][3][30]
    M = np.einsum("ncb,mb->mnc", W, alpha)                                                 # the photons' moment rows
    rng = np.random.default_rng(348)
    worst = 0.0
    for _ in range(2000):
        members = rng.choice(len(alpha), 50, replace=False)
        length = diag * rng.random() if rng.random() < 0.9 else diag
        kappa = -length / math.log(2.0)                                                    # exp(-sigma_t L) = exp2(sigma_t kappa)
        direct = (cie * albedo * np.exp2(t * kappa)) @ alpha[members].sum(0)
        S = M[members].sum(0)                                                              # [n][3]
        moment = np.exp2(bar * kappa) * sum(S[n] * kappa ** n for n in range(n_terms))
        worst = max(worst, float(np.abs(moment / direct - 1).max()))
    print("moment form vs 30 bins: worst relative error %.3g, bound %.3g" % (worst, bound(x, n_terms)))
    assert worst <= bound(x, n_terms)
    assert worst > 1e-12   # the comparison is not vacuous: two terms would sit four orders above
    two = np.exp2(bar * -diag / math.log(2.0)) * (M[:50].sum(0)[0] + M[:50].sum(0)[1] * (-diag / math.log(2.0)))
    ref = (cie * albedo * np.exp2(t * -diag / math.log(2.0))) @ alpha[:50].sum(0)
    assert np.abs(two / ref - 1).max() > bound(x, 3)


def plan(lib, **kw):
    """The flagship batch: homogeneous, one distant light, g 0, nused 50, an XYZ result, a scene that passes the gate."""
    v = dict(nLights=1, volKind=HOMOGENEOUS, g=0.0, nPhotons=100000, nUsed=50, candCap=256, maxSteps=100, nTris=0, roulette=0, distant=1,
             nCU=256, groupWavesPerCU=12, fixWavesPerCU=16, nRays=4000, nStreams=4, maxRays=1000, spp=0, momentTerms=3, outXYZ=1)
    v.update(kw)
    if v.get("hasTile"):
        v["spp"] = v["spp"] or 4
    i = PlanIn(**v)
    i.knobs = Knobs(groupGuess=1.15)
    out = BatchPlan()
    lib.pvol_plan_batch(C.byref(i), C.byref(out))
    return out


def test_plan_struct_sizes(lib):
    assert C.sizeof(PlanIn) == 152 and C.sizeof(BatchPlan) == 136   # pvol_host.h's static_assert: the new fields took padding


@pytest.mark.parametrize("kw,form", [
    ({}, MOMENTS),
    (dict(hasTile=1), MOMENTS),                   # the render driver's batch (COUNT pre-pass, PAR)
    (dict(momentTerms=1), MOMENTS), (dict(momentTerms=2), MOMENTS),
    (dict(momentTerms=0), 1),                     # the gate refused the scene (or the map has no moment rows)
    (dict(outXYZ=0), 1),                          # spectral output
    (dict(noMoments=1), 1),                       # PVOL_NO_MOMENTS=1
    (dict(statsOn=1), 1),                         # the counters' launch keeps the 30 bins
    (dict(volKind=GRID), 2),                      # a density region: SLICED, its own form
    (dict(nLights=2, hasTile=1), 1),              # REPLAY (several lights) stays on 30 bins
    (dict(hasInit=1), 1),                         # REPLAY again
    (dict(noGroup=1), 0), (dict(g=0.6), 0), (dict(nUsed=500), 0), (dict(nPhotons=0), 0),   # form 1 would not have run
    (dict(forceSeq=1), 0),
])
def test_plan_takes_the_moment_form_exactly_under_its_conditions(lib, kw, form):
    p = plan(lib, **kw)
    assert p.rc == 0
    assert p.groupForm == form
    if form:
        assert p.kernel == b"li_group_kernel"
        base = plan(lib, **dict(kw, noMoments=1))   # everything else about the batch is what the 30-bin form gets
        assert (base.path, base.tile, base.gWaves, base.fixWaves, base.deferWant, base.ldsGroup) == \
               (p.path, p.tile, p.gWaves, p.fixWaves, p.deferWant, p.ldsGroup)
