"""The C++ class's Overlap (include/RayTracer/RayTracer.h), driven by tests/cpp/overlap_driver.cpp on the Cornell box and
compared with the Python class's answers."""
import os
import subprocess

import numpy as np
import pytest

import overlap_expect as oe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")

pytestmark = pytest.mark.gpu


def test_cpp_methods_give_the_python_answers(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    exe = str(tmp_path / "overlap_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "overlap_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    rows = scenes.cornell32()
    boxes = np.concatenate([oe.random_boxes(rows, 60, 5, width=1.5), oe.whole_box(rows), oe.bad_boxes(oe.whole_box(rows)[0])])
    rows.astype("<f4").tofile(str(tmp_path / "scene.f4"))
    boxes.astype("<f4").tofile(str(tmp_path / "boxes.f4"))
    g = R.RayTracer((32, 24), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=1)
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        prims, counts = g.Overlap(boxes, 4)
        assert (counts == 0).any() and (counts > 4).any() and counts.max() == rows.shape[0] // 3
        _assert = oe.expected(boxes, rows, 4)
        assert np.array_equal(prims, _assert[0]) and np.array_equal(counts, _assert[1])
        page, left = g.Overlap(boxes, 2, after=prims[:, 3])
        want = ["OVERLAP %d %d %d %d %d" % ((c,) + tuple(p)) for p, c in zip(prims, counts)]
        want += ["PAGE %d %d %d" % ((c,) + tuple(p)) for p, c in zip(page, left)]
        out = subprocess.run([exe, str(tmp_path / "scene.f4"), str(tmp_path / "boxes.f4")] + (["accel"] if accel else []),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert out.stdout.splitlines() == want
    g.close()
