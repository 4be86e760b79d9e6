"""--exposure X,Y,Z,NX,NY,NZ[,R[,K]] of both command lines: the mask in hex and the open count of K hemisphere directions over
[1e-3, R]; the same line from tools/rt_cli.cpp and raytracertest_amd.cli, with and without --accel, equal to the API's bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exposure_expect as ee

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "rt_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread",
                    "-o", exe], check=True)
    return exe


def _cpp_directions(tmp_path, k):
    """rt::RayTracer::HemisphereDirections(k) as (k, 4) float32: the set tools/rt_cli.cpp traces."""
    exe = str(tmp_path / "d")
    if not os.path.exists(exe):
        src = tmp_path / "d.cpp"
        src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "RayTracer/RayTracer.h"\n'
                       'int main(int, char** v) { for (float f : rt::RayTracer::HemisphereDirections(std::atoi(v[1]))) std::printf("%a\\n", f); return 0; }\n')
        subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + LIBDIR, "-lrt_mi355x",
                        "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, str(k)], capture_output=True, text=True, check=True).stdout.split()
    return np.float32([float.fromhex(x) for x in out]).reshape(k, 4)


def test_both_command_lines_know_exposure(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--exposure X,Y,Z,NX,NY,NZ[,R[,K]]" in out.stdout
    for bad in ("3", "1,2,3,0,0", "1,2,3,0,0,1,", "1,2,3,0,0,x", "1,2,3,0,0,1,5,0", "1,2,3,0,0,1,5,65", "1,2,3,0,0,1,5,-3", "1,2,3,0,0,1,5,8,9"):
        out = subprocess.run([exe, "--exposure", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X,Y,Z,NX,NY,NZ[,R[,K]]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--exposure X,Y,Z,NX,NY,NZ[,R[,K]]" in py.stdout
    from raytracertest_amd.cli import build_parser
    inf = float("inf")
    assert build_parser().parse_args(["--exposure", "0.5,-1,2,0,0,1"]).exposure == (0.5, -1.0, 2.0, 0.0, 0.0, 1.0, inf, 64)
    assert build_parser().parse_args(["--exposure", "0.5,-1,2,0,0,1,0.25"]).exposure == (0.5, -1.0, 2.0, 0.0, 0.0, 1.0, 0.25, 64)
    assert build_parser().parse_args(["--exposure", "0.5,-1,2,0,0,1,0.25,7"]).exposure == (0.5, -1.0, 2.0, 0.0, 0.0, 1.0, 0.25, 7)
    assert build_parser().parse_args([]).exposure is None
    for bad in ("1,2,3,0,0", "1,2,3,0,0,1,5,0", "1,2,3,0,0,1,5,65"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--exposure", bad])
    # the C++ class's direction set is the Python one to one ulp (two libm's round the same float64 formula once each)
    from raytracertest_amd import api
    got, want = _cpp_directions(tmp_path, 64), ee.as_dirs4(api.hemisphere_directions(64))
    assert got.shape == want.shape and np.abs(got.view(np.int32) - want.view(np.int32)).max() <= 1


@pytest.mark.gpu
def test_cli_exposure_cpp_and_python_print_what_the_api_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import api
    exe = _build(tmp_path)
    rows = ee.open_box()
    scene_file = str(tmp_path / "box.f4")
    rows.astype("<f4").tofile(scene_file)
    common = ["-w", "96", "-h", "54", "-s", "1", "-i", "1", "-u", "0", "-f", "70", "-l", "3", "--aperture", "0.05", "--seed", "7",
              "--scene", scene_file, "-q"]
    g = R.RayTracer((96, 54), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=7)
    assert g.UploadScene(rows)
    # on the floor looking up, inside looking sideways with a short reach, inside with few directions (each run is two processes)
    for spec, pt, r, k, accel in (("0.5,0.5,0,0,0,1", (0.5, 0.5, 0, 0, 0, 1), np.inf, 64, False),
                                  ("0.25,0.5,0.5,1,0,0,0.9", (0.25, 0.5, 0.5, 1, 0, 0), 0.9, 64, True),
                                  ("0.3,0.6,0.2,0,0.6,0.8,100,7", (0.3, 0.6, 0.2, 0, 0.6, 0.8), 100.0, 7, True)):
        g.SetQueryAcceleration(accel)
        # each command line against the API's bits for ITS direction set (the two sets agree to one ulp, so a grazing ray may differ)
        want = []
        for dirs in (_cpp_directions(tmp_path, k), api.hemisphere_directions(k)):
            mask = int(g.Exposure(np.float32([pt + (1e-3, r)]), dirs)[0])
            want.append("exposure %016x %d %d" % (mask, bin(mask).count("1"), k))
            assert 0 < bin(mask).count("1") < k, (spec, want)
        flags = common + ["--exposure", spec] + (["--accel"] if accel else [])
        c = subprocess.run([exe] + flags + ["-o", str(tmp_path / "c.bmp")], capture_output=True, text=True, timeout=120)
        y = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli"] + flags + ["-o", str(tmp_path / "p.bmp")],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert c.returncode == 0 and y.returncode == 0, (c.stderr, y.stderr)
        assert c.stdout.splitlines() == [want[0]] and y.stdout.splitlines() == [want[1]], (spec, accel, want, c.stdout, y.stdout)
    g.close()
