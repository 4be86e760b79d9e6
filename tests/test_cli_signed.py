"""--signed X,Y,Z[,R] of both command lines: --closest's line plus feature, s and the signed distance; the same line from
tools/rt_cli.cpp and raytracertest_amd.cli, with and without --accel, equal to the API's answer."""
import os
import subprocess
import sys

import numpy as np
import pytest

import signed_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "rt_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread",
                    "-o", exe], check=True)
    return exe


def test_both_command_lines_know_signed(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--signed X,Y,Z[,R]" in out.stdout
    for bad in ("3", "3,4", "3,4,5,", "3,4,x", "1,2,3,4,5"):
        out = subprocess.run([exe, "--signed", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X,Y,Z[,R]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--signed X,Y,Z[,R]" in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--signed", "0.5,-1,2"]).signed_query == (0.5, -1.0, 2.0, float("inf"))
    assert build_parser().parse_args(["--signed", "0.5,-1,2,0.25"]).signed_query == (0.5, -1.0, 2.0, 0.25)
    assert build_parser().parse_args([]).signed_query is None


@pytest.mark.gpu
def test_cli_signed_cpp_and_python_print_what_the_api_answers(tmp_path):
    import raytracertest_amd as R
    exe = _build(tmp_path)
    rows = se.l_prism()
    scene_file = str(tmp_path / "l.f4")
    rows.astype("<f4").tofile(scene_file)
    common = ["-w", "96", "-h", "54", "-s", "1", "-i", "1", "-u", "0", "-f", "70", "-l", "3", "--aperture", "0.05", "--seed", "7",
              "--scene", scene_file, "-q"]
    g = R.RayTracer((96, 54), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=7)
    assert g.UploadScene(rows)
    # inside next to the concave edge, outside in the notch, outside within reach, outside out of reach (each run is two processes)
    for spec, pt, dist, accel, side in (("0.95,0.9,0.25", (0.95, 0.9, 0.25), np.inf, False, -1), ("1.5,1.25,0.25", (1.5, 1.25, 0.25), np.inf, True, 1),
                                        ("2.5,0.5,0.25,1", (2.5, 0.5, 0.25), 1.0, True, 1), ("2.5,0.5,0.25,0.25", (2.5, 0.5, 0.25), 0.25, False, 0)):
        g.SetQueryAcceleration(accel)
        p = np.float32([pt])
        h, s = g.SignedDistance(p, dist)
        q = g.ClosestPositions(p, h)[0]
        d = np.sqrt(h["t"][0])
        want = "signed -1" if h["prim"][0] < 0 else "signed %d %.9g %.9g %.9g %.9g %d %.9g %.9g" % (
            h["prim"][0], d, q[0], q[1], q[2], s["feature"][0], s["s"][0], np.copysign(d, s["s"][0]))
        assert (h["prim"][0] < 0) == (side == 0) and (side == 0 or np.sign(s["s"][0]) == side), (spec, h, s)
        flags = common + ["--signed", spec] + (["--accel"] if accel else [])
        c = subprocess.run([exe] + flags + ["-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
        y = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + flags + ["-o", str(tmp_path / "p.bmp")],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert c.returncode == 0 and y.returncode == 0, (c.stderr, y.stderr)
        assert c.stdout.splitlines() == [want] and y.stdout.splitlines() == [want], (spec, accel, want, c.stdout, y.stdout)
    g.close()
