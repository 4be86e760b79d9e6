"""The C++ class's TriangleDistance (include/RayTracer/RayTracer.h), driven by tests/cpp/tridistance_driver.cpp on the Cornell box
and compared bit for bit with the Python class's answers."""
import os
import subprocess

import numpy as np
import pytest

import tridistance_expect as td
import trioverlap_expect as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cpp_methods_give_the_python_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    exe = str(tmp_path / "tridistance_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tridistance_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    rows = scenes.cornell32()
    tris = td.mixed_queries(rows, 81, 5)
    tris = np.concatenate([tris, td.with_radius(te.bad_queries(tris[0])[::3], np.inf)])      # and nine with a NaN coordinate
    tris[::3, 3] = np.float32(0.01)                                      # every third one with a small radius
    rows.astype("<f4").tofile(str(tmp_path / "scene.f4"))
    tris.astype("<f4").tofile(str(tmp_path / "tris.f4"))
    g = R.RayTracer((32, 24), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=1)
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        hits, wit = g.TriangleDistance(tris)
        assert (hits["prim"] < 0).any() and (hits["prim"] >= 0).any() and not np.isfinite(te.corners_of(tris)).all()
        assert td.same((hits, wit), td.expected(tris, rows))
        hx = lambda a: tuple(int(x) for x in np.ascontiguousarray(a).view(np.uint32))
        want = ["DISTANCE %d %08x %08x %08x %d %08x %08x %08x" % ((h["prim"],) + hx(np.float32([h["t"], h["u"], h["v"]])) + (w["where"],) +
                                                                   hx(np.float32([w["x"], w["y"], w["z"]]))) for h, w in zip(hits, wit)]
        out = subprocess.run([exe, str(tmp_path / "scene.f4"), str(tmp_path / "tris.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert out.stdout.splitlines() == want
    g.close()
