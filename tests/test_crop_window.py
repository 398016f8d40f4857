"""Host side of the crop window (Film "image" `"float cropwindow"`): pvol_film_window_from_crop and pvol_film_sample_extent
against a numpy restatement of ImageFilm's constructor and GetSampleExtent (film/image.cpp:48-51, :157-166), the scene-file
front end reading the parameter, and -- the argument the GPU tests of the windowed film rest on -- that a film clamped to the
window (image.cpp:86-89, :121) holds exactly the window's slice of a full-resolution film fed the same samples.  No GPU."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, abi, load_render_case

F = np.float32


@pytest.fixture(scope="module")
def pvol():
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "cs348b-pbrt_amd", "csrc")])
    return importlib.import_module("cs348b-pbrt_amd.pvol")


@pytest.fixture(scope="module")
def ps():
    return importlib.import_module("cs348b-pbrt_amd.pbrt_scene")


def _film(xres, yres, xw=2.0, yw=2.0):
    return abi.make_film(xres, yres, np.zeros(256, np.float32), xw, yw)


def ref_window(xres, yres, crop):
    """film/image.cpp:48-51 in the reference's arithmetic: int * float is a float product, Ceil2Int = (int)ceilf."""
    c = [F(v) for v in crop]
    x0 = int(np.ceil(F(F(xres) * c[0])))
    nx = max(1, int(np.ceil(F(F(xres) * c[1]))) - x0)
    y0 = int(np.ceil(F(F(yres) * c[2])))
    ny = max(1, int(np.ceil(F(F(yres) * c[3]))) - y0)
    return x0, y0, nx, ny


def ref_extent(win, xw, yw):
    """film/image.cpp:157-166: sums left to right in float."""
    x0, y0, nx, ny = win
    return [int(np.floor(F(F(F(x0) + F(0.5)) - F(xw)))), int(np.ceil(F(F(F(F(x0) + F(0.5)) + F(nx)) + F(xw)))),
            int(np.floor(F(F(F(y0) + F(0.5)) - F(yw)))), int(np.ceil(F(F(F(F(y0) + F(0.5)) + F(ny)) + F(yw))))]


CROPS = [(0, 1, 0, 1),                    # the whole frame
         (0.25, 0.75, 0.25, 0.75),        # interior
         (0, 0.5, 0, 0.5), (0.5, 1, 0.5, 1), (0, 0.3, 0.6, 1), (0.7, 1, 0, 0.2),   # touching every edge and corner
         (0.5, 0.5, 0.5, 0.5),            # empty crop: max(1, .) makes it one pixel
         (0.31, 0.32, 0.4, 0.41),         # between pixels at small resolutions: one pixel again
         (0.1, 0.9, 0.33, 0.34), (1 / 3, 2 / 3, 1 / 7, 6 / 7), (0.999, 1, 0, 0.001), (0, 0.001, 0.999, 1), (0.05, 0.95, 0, 1)]
SIZES = [(16, 12), (96, 54), (1, 1), (7, 3), (640, 480), (1280, 720), (1920, 1080), (333, 77)]


def test_window_and_extent_match_the_reference_formulas(pvol):
    seen_one_pixel = seen_between = 0
    for xres, yres in SIZES:
        for xw, yw in [(2.0, 2.0), (0.5, 0.5), (1.5, 3.0)]:
            film = _film(xres, yres, xw, yw)
            for crop in CROPS:
                want = ref_window(xres, yres, crop)
                inside = want[0] + want[2] <= xres and want[1] + want[3] <= yres
                w = abi.FilmWindow()
                rc = pvol.lib().pvol_film_window_from_crop(C.byref(film), np.asarray(crop, F).ctypes.data_as(C.POINTER(C.c_float)), C.byref(w))
                if not inside:      # a crop whose start rounds up to the resolution: the reference's pixel past the frame, refused
                    assert rc == abi.PVOL_E_INVALID, (xres, yres, crop)
                    continue
                assert rc == abi.PVOL_OK, (xres, yres, crop)
                got = (w.x_pixel_start, w.y_pixel_start, w.x_pixel_count, w.y_pixel_count)
                assert got == want, (xres, yres, crop)
                assert pvol.film_sample_extent(film, w) == ref_extent(want, xw, yw), (xres, yres, crop, xw, yw)
                seen_one_pixel += want[2] == 1 and want[3] == 1
                seen_between += crop[0] != crop[1] and int(np.ceil(F(xres) * F(crop[1]))) == want[0]
    assert seen_one_pixel > 10 and seen_between >= 3


def test_full_crop_is_the_whole_frame_and_the_reference_captures_extent(pvol):
    """crop 0 1 0 1, and no window at all, give the sample extent the reference's own Film::GetSampleExtent wrote into the
    captures (tests/golden/render_*.bin: reference-written fixtures)."""
    for name in ("vh", "grid16", "sph", "pf_surf"):
        s, p, cam, film, smp, c = load_render_case(name)
        w = pvol.film_window_from_crop(film, (0, 1, 0, 1))
        assert (w.x_pixel_start, w.y_pixel_start, w.x_pixel_count, w.y_pixel_count) == (0, 0, film.x_resolution, film.y_resolution)
        want = [smp.x_start, smp.x_end, smp.y_start, smp.y_end]
        assert pvol.film_sample_extent(film, w) == want
        assert pvol.film_sample_extent(film, None) == want
        # ... and the sub-windows the reference's Sampler::ComputeSubWindow wrote come out of that extent
        abi.set_sample_extent(smp, [0, 0, 0, 0])
        abi.set_sample_extent(smp, pvol.film_sample_extent(film, w))
        for i, t in enumerate(c["tasks"]):
            assert pvol.sub_window(smp, int(t)) == list(c["task.window"][4 * i:4 * i + 4])


def test_invalid_crops_and_windows_are_refused(pvol):
    L = pvol.lib()
    film = _film(40, 30)
    w = abi.FilmWindow()
    fp = C.POINTER(C.c_float)
    for crop in [(-0.1, 1, 0, 1), (0, 1.5, 0, 1), (0, 1, -1, 1), (0, 1, 0, 2), (0.6, 0.4, 0, 1), (0, 1, 0.9, 0.1), (np.nan, 1, 0, 1),
                 (1, 1, 0, 1), (0, 1, 1, 1)]:
        assert L.pvol_film_window_from_crop(C.byref(film), np.asarray(crop, F).ctypes.data_as(fp), C.byref(w)) == abi.PVOL_E_INVALID, crop
    ok = np.asarray((0, 1, 0, 1), F).ctypes.data_as(fp)
    assert L.pvol_film_window_from_crop(None, ok, C.byref(w)) == abi.PVOL_E_INVALID
    assert L.pvol_film_window_from_crop(C.byref(film), None, C.byref(w)) == abi.PVOL_E_INVALID
    assert L.pvol_film_window_from_crop(C.byref(film), ok, None) == abi.PVOL_E_INVALID
    e = (C.c_int32 * 4)()
    for bad in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, -2), (38, 0, 3, 4), (0, 28, 4, 3), (40, 0, 1, 1), (0, 0, 41, 30),
                (2 ** 31 - 1, 0, 2, 2)]:
        assert L.pvol_film_sample_extent(C.byref(film), C.byref(abi.make_window(*bad)), e) == abi.PVOL_E_INVALID, bad
    assert L.pvol_film_sample_extent(C.byref(film), C.byref(abi.make_window(38, 28, 2, 2)), e) == abi.PVOL_OK
    assert L.pvol_film_sample_extent(None, None, e) == abi.PVOL_E_INVALID
    assert L.pvol_film_sample_extent(C.byref(film), None, None) == abi.PVOL_E_INVALID
    # the device entry points look at the window before they look for a device
    cam, smp = abi.Camera(), abi.make_sampler(40, 30, 4, 8)
    bad = abi.make_window(38, 0, 3, 4)
    assert L.pvol_render_tasks_window_device(None, C.byref(cam), C.byref(film), C.byref(bad), C.byref(smp), None, 0, None, None, None) == abi.PVOL_E_INVALID
    assert L.pvol_film_resolve_window_device(None, C.byref(film), C.byref(bad), None, None, None) == abi.PVOL_E_INVALID
    with pytest.raises(ValueError):
        pvol.film_window_from_crop(film, (0, 1, 0))


def test_python_restatement_of_the_front_end_agrees_with_the_library(pvol, ps):
    for xres, yres in SIZES:
        film = _film(xres, yres)
        for crop in CROPS:
            want = ref_window(xres, yres, crop)
            if want[0] + want[2] > xres or want[1] + want[3] > yres:
                with pytest.raises(ValueError):
                    ps.film_window(xres, yres, crop)
                continue
            win = ps.film_window(xres, yres, crop)
            assert tuple(int(v) for v in win) == want
            assert list(ps.sample_extent(win)) == pvol.film_sample_extent(film, abi.make_window(*want))


SCENE = """
LookAt 0 0 -5  0 0 0  0 1 0
Camera "perspective" "float fov" [40]
Film "image" "integer xresolution" [200] "integer yresolution" [100] %s
Sampler "lowdiscrepancy" "integer pixelsamples" [4]
WorldBegin
LightSource "point" "point from" [0 2 0]
WorldEnd
"""


def _load(ps, tmp_path, film_params):
    f = tmp_path / "s.pbrt"
    f.write_text(SCENE % film_params)
    return ps.load(str(f))


def test_front_end_reads_the_crop_window(ps, tmp_path):
    d = _load(ps, tmp_path, '"float cropwindow" [0.25 0.75 0.125 0.625]')
    np.testing.assert_array_equal(d["film.cropwindow"], np.array([0.25, 0.75, 0.125, 0.625], F))
    assert list(d["film"][:2]) == [200, 100]                                   # the resolution stays the frame's
    want = ref_window(200, 100, (0.25, 0.75, 0.125, 0.625))
    assert want == (50, 13, 100, 50)                                           # Ceil2Int(12.5), Ceil2Int(62.5) - 13
    assert tuple(int(v) for v in d["film.window"]) == want
    assert list(d["film.sample_extent"]) == ref_extent(want, 2.0, 2.0) == [48, 153, 11, 66]
    # CreateImageFilm orders and clamps each pair (film/image.cpp:258-261)
    d = _load(ps, tmp_path, '"float cropwindow" [0.75 0.25 -1 0.5]')
    np.testing.assert_array_equal(d["film.cropwindow"], np.array([0.25, 0.75, 0, 0.5], F))
    assert tuple(int(v) for v in d["film.window"]) == (50, 0, 100, 50)


def test_front_end_without_a_crop_window_is_the_whole_frame(ps, tmp_path):
    d = _load(ps, tmp_path, "")
    np.testing.assert_array_equal(d["film.cropwindow"], np.array([0, 1, 0, 1], F))
    assert tuple(int(v) for v in d["film.window"]) == (0, 0, 200, 100)
    assert list(d["film.sample_extent"]) == [-2, 203, -2, 103]
    smp = abi.make_sampler(200, 100, 4, 8)
    assert list(d["film.sample_extent"]) == [smp.x_start, smp.x_end, smp.y_start, smp.y_end]


@pytest.mark.parametrize("film_params", ['"float cropwindow" [0.25 0.75 0.1]',            # three numbers
                                         '"float cropwindow" [0.25 0.75 0.1 0.6 0.9]',    # five
                                         '"float cropwindow" [0.25 0.75 0.1 nan]',
                                         '"integer cropwindow" [0 1 0 1]',                # ParamSet would not find it as a float
                                         '"float cropwindow" [1 1 0 1]'])                 # the reference's pixel past the frame
def test_front_end_refuses_a_malformed_crop_window(ps, tmp_path, film_params):
    with pytest.raises(ValueError):
        _load(ps, tmp_path, film_params)


def _splat(film, xy, xyz, window=None):
    """ImageFilm::AddSample (film/image.cpp:78-137) in numpy, sample by sample in order, float32 accumulation; `window`
    (x0, y0, nx, ny) clamps the footprint and addresses the pixel relative to it (:86-89, :121)."""
    x0w, y0w, nx, ny = window if window is not None else (0, 0, film.x_resolution, film.y_resolution)
    pix = np.zeros((ny, nx, 4), F)
    table = np.asarray(film.filter_table[:], F).reshape(16, 16)
    xw, yw = F(film.filter_xwidth), F(film.filter_ywidth)
    inv_x, inv_y = F(1) / xw, F(1) / yw
    for (ix_, iy_), v in zip(xy, xyz):
        dx, dy = F(ix_ - F(0.5)), F(iy_ - F(0.5))
        x0, x1 = int(np.ceil(F(dx - xw))), int(np.floor(F(dx + xw)))
        y0, y1 = int(np.ceil(F(dy - yw))), int(np.floor(F(dy + yw)))
        x0, x1, y0, y1 = max(x0, x0w), min(x1, x0w + nx - 1), max(y0, y0w), min(y1, y0w + ny - 1)
        if x1 - x0 < 0 or y1 - y0 < 0:
            continue
        for y in range(y0, y1 + 1):
            fy = min(int(np.floor(np.abs(F(F(F(y) - dy) * inv_y) * F(16)))), 15)
            for x in range(x0, x1 + 1):
                fx = min(int(np.floor(np.abs(F(F(F(x) - dx) * inv_x) * F(16)))), 15)
                wt = table[fy, fx]
                p = pix[y - y0w, x - x0w]
                p[0] += wt * v[0]; p[1] += wt * v[1]; p[2] += wt * v[2]; p[3] += wt   # noqa: E702
    return pix


def test_windowed_film_is_the_slice_of_the_full_resolution_film(pvol, orc):
    """What the GPU tests lean on: feed the same samples, in the same order, to a full-resolution film and to a film clamped
    to the window -- the window's pixels get the same additions in the same order, so the slice is equal bit for bit.  The
    full-resolution film is the oracle's (orc.film_add_samples), the windowed one the numpy restatement above."""
    rng = np.random.default_rng(11)
    xres, yres = 24, 18
    film = abi.make_film(xres, yres, pvol.gaussian_filter_table())
    for win in [(6, 5, 9, 7), (0, 0, 8, 6), (16, 12, 8, 6), (11, 3, 1, 1)]:
        ext = ref_extent(win, 2.0, 2.0)
        n = 3000
        xy = np.stack([rng.uniform(ext[0], ext[1], n), rng.uniform(ext[2], ext[3], n)], 1).astype(F)
        xyz = rng.random((n, 4)).astype(F)
        full = orc.film_add_samples(film, xy, xyz)
        np.testing.assert_array_equal(_splat(film, xy, xyz), full)            # the restatement is the oracle's film
        got = _splat(film, xy, xyz, win)
        x0, y0, nx, ny = win
        np.testing.assert_array_equal(got, full[y0:y0 + ny, x0:x0 + nx])
        assert got[..., 3].min() > 0                                           # the apron's samples reach the border pixels
