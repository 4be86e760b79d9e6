"""The C++ class's Section and SectionSegments (include/RayTracer/RayTracer.h), driven by tests/cpp/section_driver.cpp on the
Cornell box and compared with the restatement of section_expect: rows, counts, the next page and the cut records bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import section_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
COMPILE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "section_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread"]


def planes_for(rows):
    """Planes and slabs through the Cornell box, its back wall's own plane, a slab that holds it, a plane beside it, bad planes."""
    good = np.concatenate([se.random_planes(rows, 40, 5), se.random_planes(rows, 20, 6, thick=0.3)])
    special = se.planes_of([(0, 0, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)], [-3.0, -se.INF, 50.0, 0.0], [-3.0, se.INF, 60.0, 0.0])
    return np.concatenate([good, special, se.bad_planes(good[0])])


def expected_lines(planes, rows):
    prims, counts = se.expected(planes, rows, 4)
    want = ["SECTION %d %d %d %d %d" % ((c,) + tuple(p)) for p, c in zip(prims, counts)]
    for side in (0, 1):
        for c in se.cuts(planes, prims, rows, side=side).reshape(-1):
            want.append("CUT %d %d %d " % (side, c["kind"], c["features"]) + " ".join("%08x" % w for w in np.r_[c["p0"], c["p1"]].view(np.uint32)))
    page, left = se.expected(planes, rows, 2, after=prims[:, 3])
    return want + ["PAGE %d %d %d" % ((c,) + tuple(p)) for p, c in zip(page, left)], counts


def test_the_driver_compiles_against_the_header_and_the_expected_lines_reach_every_kind(tmp_path):
    """Without a device: the class's two methods and rt_cut compile from a caller's side, and the lines the device test will
    compare hold sections, cuts of several kinds and pages."""
    from raytracertest_amd import scenes
    subprocess.run(COMPILE + ["-o", str(tmp_path / "section_driver")], check=True)
    hdr = open(os.path.join(ROOT, "include", "RayTracer", "RayTracer.h")).read()
    assert "bool Section(const std::vector<float>& planes, uint32_t maxHits" in hdr and "bool SectionSegments(" in hdr
    rows = scenes.cornell32()
    planes = planes_for(rows)
    lines, counts = expected_lines(planes, rows)
    n = planes.shape[0]
    assert len(lines) == n + 2 * 4 * n + n and (counts == 0).any() and (counts > 4).any() and counts.max() == 32
    kinds = {int(x.split()[2]) for x in lines if x.startswith("CUT")}
    assert kinds >= {se.CUT_NONE, se.CUT_SEGMENT, se.CUT_COPLANAR, se.CUT_TOUCH}


@pytest.mark.gpu
def test_cpp_methods_give_the_restated_answers(tmp_path):
    from raytracertest_amd import scenes
    exe = str(tmp_path / "section_driver")
    subprocess.run(COMPILE + ["-o", exe], check=True)
    rows = scenes.cornell32()
    planes = planes_for(rows)
    rows.astype("<f4").tofile(str(tmp_path / "scene.f4"))
    planes.astype("<f4").tofile(str(tmp_path / "planes.f4"))
    want, _ = expected_lines(planes, rows)
    for accel in (False, True):
        out = subprocess.run([exe, str(tmp_path / "scene.f4"), str(tmp_path / "planes.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert out.stdout.splitlines() == want
