"""The scene-file front end and VolumeIntegrator "single": the authored fog room, the default stepsize, "emission" still refused by
name, and every scene file's dictionary keeping its key set."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLD, ROOT

ps = importlib.import_module("cs348b-pbrt_amd.pbrt_scene")
SCENES = os.path.join(GOLD, "scenes")
FOG_ROOM = os.path.join(SCENES, "single", "fog_room_single.pbrt")   # a folder of its own: test_scene_image.py counts the files of scenes/
HEAD = 'Camera "perspective"\n%s\nWorldBegin\nVolume "homogeneous" "color sigma_a" [.1 .1 .1] "color sigma_s" [.2 .2 .2] "point p0" [0 0 0] "point p1" [1 1 1]\nWorldEnd\n'


def test_fog_room_names_the_single_integrator():
    d = ps.load(FOG_ROOM)
    assert d["vol.integrator"] == "single"
    assert float(d["params.f"][0]) == 1.0   # "stepsize" left out: CreateSingleScatteringIntegrator's default (single.cpp:143)
    assert int(d["vol.kind"][0]) == 1 and d["lights.kind"].tolist() == [2]   # a homogeneous extent, one distant light
    np.testing.assert_array_equal(d["vol.extent"], np.array([-2, 0, -2, 2, 3, 2], np.float32))
    # the render driver's limit under this integrator: diagonal x sigma_t stays far below 6.8
    diag = float(np.linalg.norm(d["vol.extent"][3:] - d["vol.extent"][:3]))
    assert diag * float((d["vol.sigma_a"] + d["vol.sigma_s"]).max()) < 2.0
    assert len(d["tris.material"]) == 6 and d["film"].tolist() == [48, 48, 4]


def test_stepsize_is_read_and_defaults_to_one(tmp_path):
    f = tmp_path / "a.pbrt"
    f.write_text(HEAD % 'VolumeIntegrator "single" "float stepsize" [.25]')
    d = ps.load(str(f))
    assert d["vol.integrator"] == "single" and float(d["params.f"][0]) == 0.25
    f.write_text(HEAD % 'VolumeIntegrator "single"')
    assert float(ps.load(str(f))["params.f"][0]) == 1.0


def test_emission_stays_refused_by_name(tmp_path):
    f = tmp_path / "e.pbrt"
    f.write_text(HEAD % 'VolumeIntegrator "emission"')
    with pytest.raises(ps.Unsupported) as e:
        ps.load(str(f))
    assert 'VolumeIntegrator "emission"' in str(e.value)


# what a scene dictionary may hold besides the keys every scene has (abi.SceneHolder reads each where it is present)
OPTIONAL = {"tris.n", "spheres.o2w", "spheres.w2o", "spheres.f", "spheres.material", "spheres.flip", "vol.density", "vol.exp", "vol.updir"}


def test_other_scenes_keep_their_key_sets(tmp_path):
    """The integrator's key is present only when the file names "single": every other scene file of tests/golden, in every folder,
    has the keys of a plain scene and optional ones that were there before."""
    f = tmp_path / "p.pbrt"
    f.write_text(HEAD % 'VolumeIntegrator "photonvolume"')
    plain = ps.load(str(f))
    assert "vol.integrator" not in plain
    f.write_text(HEAD % 'VolumeIntegrator "single"')
    single = ps.load(str(f))
    assert set(single) == set(plain) | {"vol.integrator"}
    for k in plain:   # and nothing else about the dictionary moves with the integrator's name
        np.testing.assert_array_equal(np.asarray(single[k]), np.asarray(plain[k]), err_msg=k)
    loaded = 0
    for dp, _, names in sorted(os.walk(GOLD)):
        for n in sorted(names):
            path = os.path.join(dp, n)
            if not n.endswith(".pbrt") or path == FOG_ROOM:
                continue
            try:
                d = ps.load(path)
            except (ValueError, ps.Unsupported):   # a fragment meant for Include; the two textured files the front end refuses
                continue
            loaded += 1
            assert set(plain) <= set(d) <= set(plain) | OPTIONAL, (path, sorted(set(d) ^ set(plain)))
    assert loaded >= 14


def test_render_tool_takes_the_integrator():
    text = open(os.path.join(ROOT, "tools", "render_pbrt.py")).read()
    assert "--volume-integrator" in text and "set_volume_integrator" in text
