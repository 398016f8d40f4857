"""Per-vertex normals of triangle meshes (`"normal N"`) in the scene front end and the argument checks of
pvol_set_triangle_normals, without a device.

The front end takes every vertex normal to world space as Transform::operator()(const Normal&) does (core/transform.h:232-237: the
transposed inverse, fp32, products summed left to right, not normalised) and emits `tris.n`, [n_triangles, 9]; a mesh whose N count
differs from P's loses it (CreateTriangleMeshShape, shapes/trianglemesh.cpp:397-401)."""
import ctypes as C
import importlib
import os

import numpy as np

from conftest import GOLD, abi

F = np.float32
pbrt_scene = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
pvol = importlib.import_module("cs348b-pbrt_amd.pvol")

HEAD = """Film "image" "integer xresolution" [16] "integer yresolution" [16]
Sampler "lowdiscrepancy" "integer pixelsamples" [4]
PixelFilter "gaussian"
SurfaceIntegrator "photonmap" "integer indirectphotons" [0]
VolumeIntegrator "photonvolume"
Camera "perspective" "float fov" [60]
WorldBegin
LightSource "point" "point from" [0 3 0] "color I" [10 10 10]
Material "matte" "color Kd" [.5 .5 .5]
"""
QUAD_P = [-1, 0, -1, 1, 0, -1, 1, 0, 1, -1, 0, 1]
QUAD_N = [.3, 1, .1, -.2, 1, .4, .1, .9, -.5, -.4, 1.1, -.2]
QUAD_IDX = [0, 1, 2, 2, 3, 0]


def _nums(v):
    return " ".join(repr(float(x)) for x in v)


def _mesh(P=QUAD_P, N=None, idx=QUAD_IDX):
    s = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]' % (" ".join(str(i) for i in idx), _nums(P))
    if N is not None:
        s += ' "normal N" [%s]' % _nums(N)
    return s + "\n"


def _load(tmp_path, body):
    path = tmp_path / "scene.pbrt"
    path.write_text(HEAD + body + "WorldEnd\n")
    return pbrt_scene.load(str(path))


def _inverse_transpose(minv, n):
    """core/transform.h:232-237 restated: (mInv[0][i] * x + mInv[1][i] * y) + mInv[2][i] * z in fp32."""
    x, y, z = (F(c) for c in n)
    return np.array([F(F(F(minv[0, i] * x) + F(minv[1, i] * y)) + F(minv[2, i] * z)) for i in range(3)], F)


def test_normals_go_to_world_space_by_the_transposed_inverse(tmp_path):
    xf = "Scale 2 1 1\nRotate 35 0.3 1 0.2\nScale -1 1 1\n"
    d = _load(tmp_path, "AttributeBegin\n" + xf + _mesh(N=QUAD_N) + "AttributeEnd\n")
    ctm = pbrt_scene.scale(2, 1, 1) * pbrt_scene.rotate(F(35), [F(0.3), F(1), F(0.2)]) * pbrt_scene.scale(-1, 1, 1)
    minv = np.asarray(ctm.minv, F)
    N = np.array(QUAD_N, F).reshape(4, 3)
    want = np.array([np.concatenate([_inverse_transpose(minv, N[v]) for v in QUAD_IDX[3 * t:3 * t + 3]]) for t in range(2)], F)
    assert d["tris.n"].dtype == F and d["tris.n"].shape == (2, 9)
    assert d["tris.n"].tobytes() == want.tobytes()   # bit for bit
    assert not np.allclose(np.linalg.norm(d["tris.n"].reshape(-1, 3), axis=1), 1.0)   # not normalised
    # the transform mirrors: flip is as it is without N
    flat = _load(tmp_path, "AttributeBegin\n" + xf + _mesh() + "AttributeEnd\n")
    np.testing.assert_array_equal(d["tris.flip"], [1, 1])
    np.testing.assert_array_equal(d["tris.flip"], flat["tris.flip"])
    assert d["tris.p"].tobytes() == flat["tris.p"].tobytes()


def test_a_file_without_normals_has_no_key(tmp_path):
    assert "tris.n" not in _load(tmp_path, _mesh())
    assert abi.SceneHolder(_load(tmp_path, _mesh())).tri_normals is None


def test_a_wrong_normal_count_is_dropped(tmp_path):
    assert "tris.n" not in _load(tmp_path, _mesh(N=QUAD_N[:9]))
    assert "tris.n" not in _load(tmp_path, _mesh(N=QUAD_N + [0, 1, 0]))
    # only the type "normal" is FindNormal's
    assert "tris.n" not in _load(tmp_path, _mesh().rstrip("\n") + ' "vector N" [%s]\n' % _nums(QUAD_N))


def test_two_meshes_one_with_normals(tmp_path):
    other = [c + 3 for c in QUAD_P]
    d = _load(tmp_path, _mesh() + _mesh(P=other, N=QUAD_N) + _mesh(P=[c - 3 for c in QUAD_P]))
    assert d["tris.n"].shape == (6, 9)
    assert not d["tris.n"][:2].any() and not d["tris.n"][4:].any()
    N = np.array(QUAD_N, F).reshape(4, 3)
    np.testing.assert_array_equal(d["tris.n"][2], N[[0, 1, 2]].reshape(-1))   # identity transform: the file's values
    np.testing.assert_array_equal(d["tris.n"][3], N[[2, 3, 0]].reshape(-1))
    h = abi.SceneHolder(d)
    assert h.tri_normals.shape == (6, 9) and h.tri_normals.dtype == F


def _check(holder, n, count):
    L = pvol.lib()
    ptr = None if n is None else np.ascontiguousarray(n, F).ctypes.data_as(C.POINTER(C.c_float))
    return L.pvol_check_triangle_normals(C.byref(holder.scene), ptr, count)


def test_argument_checks_without_a_device(tmp_path):
    d = _load(tmp_path, _mesh(N=QUAD_N))
    h = abi.SceneHolder(d)
    n = h.tri_normals
    assert _check(h, n, 2) == abi.PVOL_OK
    assert _check(h, None, 0) == abi.PVOL_OK                     # clearing
    assert _check(h, n, 1) == abi.PVOL_E_INVALID                 # a count that differs from the scene's
    assert _check(h, np.zeros((3, 9), F), 3) == abi.PVOL_E_INVALID
    assert _check(h, None, 2) == abi.PVOL_E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        m = n.copy()
        m[1, 4] = bad
        assert _check(h, m, 2) == abi.PVOL_E_INVALID
    assert pvol.lib().pvol_check_triangle_normals(None, None, 0) == abi.PVOL_E_INVALID
    # a test entry like pvol_check_scene, not ABI; the entry point itself is ABI
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "pvol.h")).read()
    assert "pvol_check_triangle_normals" not in text and "pvol_set_triangle_normals" in text
    assert "pvol_set_triangle_normals" in pvol.EXPORTS


def test_the_committed_fixture_parses_and_passes_the_scene_check():
    path = os.path.join(GOLD, "smooth", "glassball_smooth.pbrt")
    assert os.path.getsize(path) < 100 * 1024
    d = pbrt_scene.load(path)
    nt = len(d["tris.material"])
    assert d["tris.n"].shape == (nt, 9) and nt == 224 + 6
    ball = d["tris.n"][:224].reshape(-1, 3, 3)
    assert np.abs(ball).sum(axis=(1, 2)).min() > 0 and not d["tris.n"][224:].any()   # the ball has normals, the walls none
    # the normals lie on the side of the winding's own normal (the reference uses N as written, it never face-forwards it)
    P = d["tris.p"].reshape(-1, 3, 3)[:224].astype(np.float64)
    ng = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 1])
    assert (np.einsum("tk,tvk->tv", ng, ball.astype(np.float64)) > 0).all()
    assert (d["tris.flip"][:224] == 0).all()
    h = abi.SceneHolder(d)
    p = abi.params_from_blob(d)
    assert pvol.lib().pvol_check_scene(C.byref(p), C.byref(h.scene)) == abi.PVOL_OK
    assert _check(h, h.tri_normals, nt) == abi.PVOL_OK
