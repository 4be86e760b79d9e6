"""--nearest X,Y,Z[,R[,K]] of both command lines: the point through ClosestAll, one line `prim distance u v` per stored record,
the same lines from tools/rt_cli.cpp and raytracertest_amd.cli, with and without --accel, equal to the API's answer; and
--nearest alone is still the hit rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cli_nearest_cpp_and_python_print_what_the_api_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    exe = str(tmp_path / "rt_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread",
                    "-o", exe], check=True)
    scene_file = str(tmp_path / "cornell.f4")
    scenes.cornell32().astype("<f4").tofile(scene_file)
    common = ["-w", "96", "-h", "54", "-s", "1", "-i", "1", "-u", "0", "-f", "70", "-l", "3", "--aperture", "0.05", "--seed", "7",
              "--scene", scene_file, "-q"]
    g = R.RayTracer((96, 54), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=7)
    assert g.UploadScene(scenes.cornell32())
    pt = np.float32([[0.25, 0.5, 2.0]])
    everything = g.ClosestAll(pt, 16)
    assert everything[1][0] == 16
    r = float(np.float32(np.sqrt(everything[0]["t"][0, 5]) * np.float32(1.001)))     # a radius that holds a few of them (an fp32 number)
    # (each run is two processes)
    for spec, k, dist, modes in (("0.25,0.5,2", 8, np.inf, (False, True)), ("0.25,0.5,2,%.9g" % r, 8, r, (True,)),
                                 ("0.25,0.5,2,%.9g,3" % r, 3, r, (False,)), ("0.25,0.5,2,inf,16", 16, np.inf, (True,))):
        for accel in modes:
            g.SetQueryAcceleration(accel)
            hits, counts = g.ClosestAll(pt, k, max_distance=np.float32(dist))
            assert counts[0] == k if dist == np.inf else 3 <= counts[0] < 16
            want = ["%d %.9g %.9g %.9g" % (h["prim"], np.sqrt(h["t"]), h["u"], h["v"]) for h in hits[0, :counts[0]]]
            flags = common + ["--nearest", spec] + (["--accel"] if accel else [])
            c = subprocess.run([exe] + flags + ["-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
            p = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + flags + ["-o", str(tmp_path / "p.bmp")],
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert c.returncode == 0 and p.returncode == 0, (c.stderr, p.stderr)
            assert c.stdout.splitlines() == want and p.stdout.splitlines() == want, (spec, accel, want, c.stdout, p.stdout)
    g.close()
    out = subprocess.run([exe] + common + ["--nearest", "1,1,1,2,17", "-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--nearest" in out.stderr
    out = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + common + ["--nearest", "1,1,1,2,17", "-o", str(tmp_path / "p.bmp")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and "--nearest" in out.stderr
