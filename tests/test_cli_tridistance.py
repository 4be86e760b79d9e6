"""--tri-distance X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,R] of both command lines: the triangle through TriangleDistance, one line
`tri-distance prim distance where xq yq zq xs ys zs` (or `tri-distance -1`), the same line from tools/rt_cli.cpp and
raytracertest_amd.cli, with and without --accel, equal to the API's answer for the Cornell box."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cli_tri_distance_cpp_and_python_print_what_the_api_answers(tmp_path):
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
    floating = "-0.25,-0.25,-3.5,0.25,0.25,-2.5,0,0.5,-3"                # a triangle inside the box
    nothing = 0
    # (each run is two processes)
    far = "50,50,50,51,50,50,50,51,50,0.5"                              # far outside the box, within half a unit: nothing
    for spec, modes in ((floating, (False, True)), (far, (False,)), ("-10,-10,-3,10,-10,-3.5,0,10,-2.5,2", (True,))):
        v = [float(x) for x in spec.split(",")]
        for accel in modes:
            g.SetQueryAcceleration(accel)
            h, w = g.TriangleDistance(np.float32([v[:9]]), v[9] if len(v) == 10 else np.inf)
            a, b = g.TriangleDistancePositions(h, w)
            if h["prim"][0] < 0:
                want, nothing = ["tri-distance -1"], nothing + 1
            else:
                want = ["tri-distance %d %.9g %d %.9g %.9g %.9g %.9g %.9g %.9g" % ((h["prim"][0], np.sqrt(h["t"][0]), w["where"][0]) + tuple(a[0]) + tuple(b[0]))]
            flags = common + ["--tri-distance=" + spec] + (["--accel"] if accel else [])
            c = subprocess.run([exe] + common + ["--tri-distance", spec] + (["--accel"] if accel else []) + ["-o", str(tmp_path / "c.bmp")],
                               capture_output=True, text=True, timeout=120)
            p = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + flags + ["-o", str(tmp_path / "p.bmp")],
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert c.returncode == 0 and p.returncode == 0, (c.stderr, p.stderr)
            assert c.stdout.splitlines() == want and p.stdout.splitlines() == want, (spec, accel, want, c.stdout, p.stdout)
    assert nothing == 1                                                  # the small radius finds nothing, the others something
    g.close()
