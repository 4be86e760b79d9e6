"""CPU checks of the k-nearest point query's boundary (rt_tracer_closest_all / _device): declared, exported, argument checks
that need no device, the Python and C++ classes and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from query_expect import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_closest_all", "rt_tracer_closest_all_device")


def test_symbols_are_declared_exported_in_header_order_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert (hdr.index("rt_tracer_closest_point_device(") < hdr.index("rt_tracer_closest_all(") < hdr.index("rt_tracer_closest_all_device(")
            < hdr.index("rt_tracer_create_multi("))
    s = api.ABI_SYMBOLS
    assert s.index("rt_tracer_closest_point_device") < s.index(NEW[0]) < s.index(NEW[1]) and len(set(s)) == len(s)
    pts = np.zeros((4, 4), np.float32)
    after = np.zeros(4, HIT_DTYPE)
    out = np.zeros((4, 4), HIT_DTYPE)
    counts = np.zeros(4, np.uint32)
    a = (pts.ctypes.data, after.ctypes.data, 4, 4, out.ctypes.data, counts.ctypes.data)
    assert L.rt_tracer_closest_all(None, *a) == 1
    assert L.rt_tracer_closest_all_device(None, *a, None) == 1
    assert L.rt_tracer_closest_all(None, None, None, 0, 4, None, None) == 1
    assert L.rt_tracer_closest_all_device(None, None, None, 4, 4, None, None, None) == 1


def test_python_class_has_the_methods_and_checks_max_hits():
    from raytracertest_amd import api
    for m in ("ClosestAll", "_closest_all_tensor", "ClosestWithin"):
        assert callable(getattr(api.RayTracer, m))
    def k(max_hits):                                                   # ClosestAll, ClosestWithin and ClosestSides report as ClosestAll
        return api.RayTracer._max_hits("ClosestAll", max_hits)
    assert k(1) == 1 and k(16) == 16 and k(4.0) == 4 and api.RT_MAX_HITS == 16
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="max_hits"):
            k(bad)
    with pytest.raises(ValueError, match=r"^ClosestAll: max_hits = 17 \(1 to 16\)$"):
        k(17)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float p[4] = {0}; rt_hit h[RT_MAX_HITS]; rt_hit after; uint32_t c;\n'
                   '  after.t = 0; after.u = 0; after.v = 0; after.prim = RT_PRIM_NONE;\n'
                   '  return rt_tracer_closest_all(NULL, p, &after, 1, RT_MAX_HITS, h, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_closest_all_device(NULL, p, NULL, 1, 1, h, &c, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_closest_all_and_rejects_bad_vectors_and_counts(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> pts(8, 0.0f), five(5, 0.0f); std::vector<rt_hit> hits(3), after(3); std::vector<uint32_t> counts(5);\n'
                   '  if (r.ClosestAll(five, 4, hits, counts) || hits.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.ClosestAll(pts, 0, hits, counts) || r.ClosestAll(pts, RT_MAX_HITS + 1, hits, counts) || hits.size() != 3) return 2;\n'
                   '  if (r.ClosestAll(pts, 4, hits, counts, after) || hits.size() != 3) return 3;       // a cursor of another length\n'
                   '  if (!r.ClosestAll(five, 4).empty() || !r.ClosestAll(pts, 17).empty()) return 4;\n'
                   '  const bool ok = r.ClosestAll(pts, 3, hits, counts);\n'
                   '  if (ok != r.Valid()) return 5;\n'
                   '  if (ok && (hits.size() != 6 || counts.size() != 2 || counts[0] != 0 || hits[0].prim != RT_PRIM_NONE ||\n'
                   '             r.ClosestAll(pts, 3).size() != 6)) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_the_nearest_query_and_keep_the_hit_rule_flag(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--nearest X,Y,Z[,R[,K]]" in out.stdout
    for bad in ("3", "3,4", "3,4,5,", "3,4,x", "1,2,3,4,5,6", "1,2,3,4,x", "1,2,3,4,-1"):
        out = subprocess.run([exe, "--nearest", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X,Y,Z[,R[,K]]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "X,Y,Z[,R[,K]]" in py.stdout
    from raytracertest_amd.cli import build_parser
    a = build_parser().parse_args(["--nearest", "0.5,1,2"])
    assert a.nearest_query == (0.5, 1.0, 2.0, float("inf"), 8) and a.nearest is False
    assert build_parser().parse_args(["--nearest", "0.5,1,2,0.25"]).nearest_query == (0.5, 1.0, 2.0, 0.25, 8)
    assert build_parser().parse_args(["--nearest=-0.5,1,2,0.25,3"]).nearest_query == (-0.5, 1.0, 2.0, 0.25, 3)
    # alone it is the hit rule it always was
    a = build_parser().parse_args(["--edges", "--nearest", "-o", "x.bmp"])
    assert a.nearest is True and not hasattr(a, "nearest_query") and a.out == "x.bmp"
    assert build_parser().parse_args([]).nearest is False
    a = build_parser().parse_args(["--nearest", "--nearest", "1,2,3"])
    assert a.nearest is True and a.nearest_query == (1.0, 2.0, 3.0, float("inf"), 8)
    for bad in ("3,4", "1,2,3,4,5,6", "1,2,3,4,x"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--nearest", bad])
