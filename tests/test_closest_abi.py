"""CPU checks of the point query's boundary (rt_tracer_closest_point / _device): declared, exported, argument checks that need
no device, the Python and C++ classes and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from query_expect import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_closest_point", "rt_tracer_closest_point_device")


def test_symbols_are_declared_exported_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert hdr.index("rt_tracer_intersect_all_device(") < hdr.index("rt_tracer_closest_point(") < hdr.index("rt_tracer_create_multi(")
    pts = np.zeros((4, 4), np.float32)
    out = np.zeros(4, HIT_DTYPE)
    assert L.rt_tracer_closest_point(None, pts.ctypes.data, 4, out.ctypes.data) == 1
    assert L.rt_tracer_closest_point_device(None, pts.ctypes.data, 4, out.ctypes.data, None) == 1
    assert L.rt_tracer_closest_point(None, None, 0, None) == 1
    assert L.rt_tracer_closest_point_device(None, None, 4, None, None) == 1


def test_python_class_has_the_methods():
    from raytracertest_amd import api
    for m in ("ClosestPoint", "_closest_point_tensor", "ClosestPositions"):
        assert callable(getattr(api.RayTracer, m))
    d = api.RayTracer._d2max
    assert d(np.inf) == np.inf and d(3.0) == np.float32(9.0) and d(-2.0) == np.float32(-4.0) and np.isnan(d(np.nan))
    assert d(np.float32(1.1)) == np.float32(1.1) * np.float32(1.1)      # squared in fp32


@pytest.mark.parametrize("max_distance", [np.inf, 2.0, -2.0, 1e30])    # (1e30 squared overflows fp32: +inf)
def test_points_array_fills_the_radius_column_of_three_column_points(max_distance):
    from raytracertest_amd import api
    f, d2 = api.RayTracer._points_array, api.RayTracer._d2max(max_distance)
    assert d2 == {np.inf: np.inf, 2.0: 4.0, -2.0: -4.0, 1e30: np.inf}[max_distance]
    one = f("ClosestPoint", (1.0, 2.0, 3.0), max_distance)                # a single (3,) point
    assert one.dtype == np.float32 and one.shape == (1, 4) and one.flags.c_contiguous
    assert one.tobytes() == np.array([[1, 2, 3, d2]], np.float32).tobytes()
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    got = f("ClosestAll", pts, max_distance)
    assert got.dtype == np.float32 and got.shape == (5, 4) and got.flags.c_contiguous
    assert np.array_equal(got[:, :3], pts) and got[:, 3].tobytes() == np.full(5, d2, np.float32).tobytes()


def test_points_array_keeps_four_column_points_and_names_its_caller():
    from raytracertest_amd import api
    f = api.RayTracer._points_array
    base = np.arange(40, dtype=np.float32).reshape(5, 8)
    base[2, 3] = np.nan
    view = base[:, :4]                                                    # not contiguous
    got = f("SignedDistance", view, 2.0)                                  # the radius column is the caller's: max_distance plays no part
    assert got.shape == (5, 4) and got.dtype == np.float32 and got.flags.c_contiguous
    assert got.tobytes() == np.ascontiguousarray(view).tobytes()
    assert f("ClosestPoint", np.zeros((0, 4), np.float32), np.inf).shape == (0, 4)
    for who in ("ClosestPoint", "ClosestAll", "ClosestWithin", "SignedDistance", "ClosestSides"):
        with pytest.raises(ValueError, match=r"^%s: expected \(n, 3\) or \(n, 4\) float32 points, got shape \(2, 5\)$" % who):
            f(who, np.zeros((2, 5), np.float32), np.inf)
        with pytest.raises(ValueError, match=r"^%s: expected .* got shape \(\)$" % who):
            f(who, 1.0, np.inf)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float p[4] = {0}; rt_hit h;\n'
                   '  h.prim = RT_PRIM_NONE;\n'
                   '  return rt_tracer_closest_point(NULL, p, 1, &h) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_closest_point_device(NULL, p, 1, &h, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_closest_point_and_rejects_a_vector_of_five_floats(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> pts(8, 0.0f), five(5, 0.0f); std::vector<rt_hit> hits(3);\n'
                   '  if (r.ClosestPoint(five, hits) || hits.size() != 3) return 1;\n'
                   '  if (!r.ClosestPoint(five).empty()) return 2;\n'
                   '  const bool ok = r.ClosestPoint(pts, hits);\n'
                   '  if (ok != r.Valid()) return 3;\n'
                   '  if (ok && (hits.size() != 2 || hits[0].prim != RT_PRIM_NONE || r.ClosestPoint(pts).size() != 2)) return 4;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_closest(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--closest X,Y,Z[,R]" in out.stdout
    for bad in ("3", "3,4", "3,4,5,", "3,4,x", "1,2,3,4,5"):
        out = subprocess.run([exe, "--closest", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X,Y,Z[,R]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--closest X,Y,Z[,R]" in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--closest", "0.5,-1,2"]).closest == (0.5, -1.0, 2.0, float("inf"))
    assert build_parser().parse_args(["--closest", "0.5,-1,2,0.25"]).closest == (0.5, -1.0, 2.0, 0.25)
    assert build_parser().parse_args([]).closest is None
