"""The C++ class's Exposure and HemisphereDirections (include/RayTracer/RayTracer.h), driven by tests/cpp/exposure_driver.cpp and
compared bit for bit with the Python class's answers."""
import os
import subprocess

import numpy as np
import pytest

import exposure_expect as ee

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cpp_methods_give_the_python_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import api
    exe = str(tmp_path / "exposure_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "exposure_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    rows = ee.open_box()
    pts = ee.open_box_points()
    dirs = ee.as_dirs4(api.hemisphere_directions(64))
    for name, a in (("scene.f4", rows), ("points.f4", pts), ("dirs.f4", dirs)):
        a.astype("<f4").tofile(str(tmp_path / name))
    g = R.RayTracer((32, 24), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=1)
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        local, world, own = g.Exposure(pts, dirs), g.Exposure(pts, dirs, world=True), g.Exposure(pts, api.hemisphere_directions(48))
        assert len(set(local.tolist())) > 10 and not np.array_equal(local, world)
        want = ["LOCAL %016x" % int(m) for m in local] + ["WORLD %016x" % int(m) for m in world] + ["OWN %016x" % int(m) for m in own]
        out = subprocess.run([exe] + [str(tmp_path / f) for f in ("scene.f4", "points.f4", "dirs.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert out.stdout.splitlines() == want
    g.close()
