"""--overlap-hexa X0,Y0,Z0,...,X7,Y7,Z7[,K] and --select X0,Y0,X1,Y1,FAR[,NEAR] of both command lines: `overlap-hexa count` and one
line per stored prim, `select count` and one line per prim, the same lines from tools/rt_cli.cpp and raytracertest_amd.cli, with
and without --accel, equal to the API's answers for the Cornell box."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cli_overlap_hexa_and_select_cpp_and_python_print_what_the_api_answers(tmp_path):
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

    def both(option, spec, accel):
        flags = [option, spec] + (["--accel"] if accel else [])
        c = subprocess.run([exe] + common + flags + ["-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
        p = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + common + [option + "=" + spec] + flags[2:] + ["-o", str(tmp_path / "p.bmp")],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        return c, p

    slab = R.RayTracer.box_corners([-10, -10, -3.25], [10, 10, -2.75])[0]              # a slab through the whole box
    skew = R.RayTracer.oriented_box_corners([0, -0.5, -2.5], [[0.25, 0.25, 0], [-0.125, 0.125, 0], [0, 0.125, 0.5]])[0]
    text = lambda c: ",".join("%.9g" % v for v in c.reshape(-1))
    # (each run is two processes)
    for corners, k, accel in ((slab, 8, False), (slab, 0, True), (skew, 3, True)):
        g.SetQueryAcceleration(accel)
        prims, counts = g.OverlapHexahedra(corners[None], k)
        want = ["overlap-hexa %d" % counts[0]] + ["%d" % p for p in prims[0, :min(int(counts[0]), k)]]
        c, p = both("--overlap-hexa", text(corners) + ",%d" % k, accel)
        assert c.returncode == 0 and p.returncode == 0, (c.stderr, p.stderr)
        assert c.stdout.splitlines() == want and p.stdout.splitlines() == want, (k, accel, want, c.stdout, p.stdout)
    assert g.OverlapHexahedra(slab[None], 16)[1][0] >= 8                              # the slab cuts the walls
    for spec, accel in (("0,0,95,53,10", False), ("30,20,60,40,2.5,0.5", True)):
        v = spec.split(",")
        g.SetQueryAcceleration(accel)
        sel = g.SelectRect(*(int(x) for x in v[:4]), near=float(v[5]) if len(v) == 6 else 0.0, far=float(v[4]))
        want = ["select %d" % sel.shape[0]] + ["%d" % p for p in sel]
        c, p = both("--select", spec, accel)
        assert c.returncode == 0 and p.returncode == 0, (c.stderr, p.stderr)
        assert c.stdout.splitlines() == want and p.stdout.splitlines() == want, (spec, accel, want, c.stdout, p.stdout)
        assert sel.shape[0] > 16 or accel                                # the whole image needs the cursor
    g.close()
    bad = ",".join(["0"] * 24) + ",17"
    out = subprocess.run([exe] + common + ["--overlap-hexa", bad, "-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--overlap-hexa" in out.stderr
    out = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + common + ["--overlap-hexa", bad, "-o", str(tmp_path / "p.bmp")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and "--overlap-hexa" in out.stderr
    out = subprocess.run([exe] + common + ["--select", "0,0,96,10,5", "-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--select" in out.stderr            # a pixel outside the image
