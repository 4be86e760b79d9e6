"""--spherecast X,Y,Z,DX,DY,DZ,R[,TMAX] of both command lines: the sweep through SphereCast, `spherecast prim t u v x y z` with the
contact point, the same line from tools/rt_cli.cpp and raytracertest_amd.cli, with and without --accel, equal to the API's answer
for the Cornell box."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cli_spherecast_cpp_and_python_print_what_the_api_answers(tmp_path):
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
    # (each run is two processes)
    kinds = set()
    for spec, modes in (("0,0,0,0.25,0.125,-1,0.25", (False, True)), ("0,0,0,0,0,-1,0.125,0.5", (False,)), ("0,0,0,0,-1,0,50", (True,))):
        v = [float(x) for x in spec.split(",")]
        sw = np.float32([v + [np.inf] * (8 - len(v))])
        for accel in modes:
            g.SetQueryAcceleration(accel)
            h = g.SphereCast(sw)
            if h["prim"][0] < 0:
                want = ["spherecast -1"]
            else:
                q = g.SphereCastContacts(sw, h)[1][0]
                want = ["spherecast %d %.9g %.9g %.9g %.9g %.9g %.9g" % (h["prim"][0], h["t"][0], h["u"][0], h["v"][0], q[0], q[1], q[2])]
            kinds.add("none" if h["prim"][0] < 0 else "start" if h["t"][0] == 0 else "moving")
            flags = common + ["--spherecast=" + spec] + (["--accel"] if accel else [])
            c = subprocess.run([exe] + common + ["--spherecast", spec] + (["--accel"] if accel else []) + ["-o", str(tmp_path / "c.bmp")],
                               capture_output=True, text=True, timeout=120)
            p = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + flags + ["-o", str(tmp_path / "p.bmp")],
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert c.returncode == 0 and p.returncode == 0, (c.stderr, p.stderr)
            assert c.stdout.splitlines() == want and p.stdout.splitlines() == want, (spec, accel, want, c.stdout, p.stdout)
    assert kinds == {"none", "start", "moving"}
    g.close()
