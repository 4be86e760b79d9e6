"""The C++ class's SignedDistance and ClosestSides (include/RayTracer/RayTracer.h), driven by tests/cpp/signed_driver.cpp and
compared bit for bit with the Python class's answers."""
import os
import subprocess

import numpy as np
import pytest

import closest_expect as ce
import signed_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def _hex(x):
    return float(np.float32(x)).hex()


def test_cpp_methods_give_the_python_answers(tmp_path):
    import raytracertest_amd as R
    exe = str(tmp_path / "signed_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "signed_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    rows = se.l_prism()
    pts = ce.with_radius(se.probe_points(rows, n_random=200)[::7], np.float32(0.3))
    rows.astype("<f4").tofile(str(tmp_path / "scene.f4"))
    pts.astype("<f4").tofile(str(tmp_path / "points.f4"))
    g = R.RayTracer((32, 24), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=1)
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        hits, sides = g.SignedDistance(pts)
        assert (hits["prim"] >= 0).any() and (hits["prim"] == -1).any() and (sides["s"] < 0).any() and (sides["s"] > 0).any()
        rows4, _ = g.ClosestAll(pts, 4)
        sides4 = g.ClosestSides(pts, rows4)
        want = ["SIGNED %d %s %s %s %d %s" % (h["prim"], _hex(h["t"]), _hex(h["u"]), _hex(h["v"]), s["feature"], _hex(s["s"]))
                for h, s in zip(hits, sides)]
        want += ["SIDE %d %d %s" % (h["prim"], s["feature"], _hex(s["s"])) for h, s in zip(rows4.reshape(-1), sides4.reshape(-1))]
        out = subprocess.run([exe, str(tmp_path / "scene.f4"), str(tmp_path / "points.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr

        def parse(line):                                                 # (C's %a and Python's hex() spell a float differently)
            f = line.split()
            return tuple(x if i == 0 or x.lstrip("-").isdigit() else float.fromhex(x) for i, x in enumerate(f))
        assert [parse(x) for x in out.stdout.splitlines()] == [parse(x) for x in want]
    g.close()
