"""The C++ class's SphereCast (include/RayTracer/RayTracer.h), driven by tests/cpp/spherecast_driver.cpp on the Cornell box and
compared with the Python class's answers bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import spherecast_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cpp_methods_give_the_python_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    exe = str(tmp_path / "spherecast_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "spherecast_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    rows = scenes.cornell32()
    sweeps = np.concatenate([se.random_sweeps(rows, 60, 5), se.start_sweeps(rows, 10, 6), se.bad_sweeps(se.random_sweeps(rows, 1, 7)[0])])
    rows.astype("<f4").tofile(str(tmp_path / "scene.f4"))
    sweeps.astype("<f4").tofile(str(tmp_path / "sweeps.f4"))
    g = R.RayTracer((32, 24), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=1)
    assert g.UploadScene(rows)
    exp = se.expected(sweeps, rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        hits = g.SphereCast(sweeps)
        assert se.same_hits(hits, exp) and (hits["prim"] >= 0).sum() > 30 and (hits["prim"] < 0).sum() > 5 and (hits["t"][hits["prim"] >= 0] == 0).any()
        want = ["SWEEP %d %08x %08x %08x" % (h["prim"], h["t"].view(np.uint32), h["u"].view(np.uint32), h["v"].view(np.uint32)) for h in hits]
        out = subprocess.run([exe, str(tmp_path / "scene.f4"), str(tmp_path / "sweeps.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert out.stdout.splitlines() == want
    g.close()
