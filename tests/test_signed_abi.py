"""CPU checks of the signed point queries' boundary (rt_tracer_signed_distance, rt_tracer_closest_sides and their _device forms,
rt_dbg_feature_normals): declared, exported, the size of rt_side, argument checks that need no device, and the Python and C++
classes."""
import ctypes as C
import os
import subprocess

import numpy as np

from query_expect import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_signed_distance", "rt_tracer_signed_distance_device", "rt_tracer_closest_sides", "rt_tracer_closest_sides_device",
       "rt_dbg_feature_normals")


def test_symbols_are_declared_exported_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert hdr.index("rt_tracer_closest_all_device(") < hdr.index("rt_tracer_signed_distance(") < hdr.index("rt_tracer_create_multi(")
    assert api.SIDE_DTYPE.itemsize == 8 and api.SIDE_DTYPE.names == ("s", "feature")
    pts = np.zeros((4, 4), np.float32)
    hits = np.zeros(4, HIT_DTYPE)
    sides = np.zeros(4, api.SIDE_DTYPE)
    p, h, s = pts.ctypes.data, hits.ctypes.data, sides.ctypes.data
    assert L.rt_tracer_signed_distance(None, p, 4, h, s) == 1
    assert L.rt_tracer_signed_distance_device(None, p, 4, h, s, None) == 1
    assert L.rt_tracer_signed_distance(None, None, 0, None, None) == 1
    assert L.rt_tracer_closest_sides(None, p, h, 4, 1, s) == 1
    assert L.rt_tracer_closest_sides_device(None, p, h, 4, 1, s, None) == 1
    assert L.rt_tracer_closest_sides(None, None, None, 0, 1, None) == 1


def test_feature_normals_argument_table():
    from raytracertest_amd import api
    L = api.load_library()
    rows = np.zeros((6, 4), np.float32)
    rows[:, :3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0], [-1, 0, 0]]
    info = (C.c_uint64 * 8)()
    out = np.full((2, 7, 4), 9.0, np.float32)
    r = rows.ctypes.data
    assert L.rt_dbg_feature_normals(None, 6, 0, out.ctypes.data, out.nbytes, info) == 1
    assert L.rt_dbg_feature_normals(r, 6, 0, out.ctypes.data, out.nbytes, None) == 1
    for bad in (0, 2, 4, 5):                                             # no triangle, or no multiple of three rows
        assert L.rt_dbg_feature_normals(r, bad, 0, out.ctypes.data, out.nbytes, info) == 1
    assert L.rt_dbg_feature_normals(r, 6, 0, None, 0, info) == 0         # sizes only
    assert list(info)[:4] == [2, 4, 5, 2] and info[5] == 224
    assert L.rt_dbg_feature_normals(r, 6, 0, out.ctypes.data, 223, info) != 0 and "224" in L.rt_last_error().decode()
    assert L.rt_dbg_feature_normals(r, 6, 0, None, 224, info) != 0
    assert (out == 9.0).all()                                            # nothing was written by the rejected calls
    assert L.rt_dbg_feature_normals(r, 6, 0, out.ctypes.data, out.nbytes, info) == 0
    assert (out[:, :, :3] == np.float32([0, 0, 1])).all() and (out[:, :, 3] == 0).all()
    assert np.array_equal(api.feature_normals(rows), out)


def test_python_class_has_the_methods():
    from raytracertest_amd import api
    for m in ("SignedDistance", "ClosestSides", "Contains", "SignedDistances", "DistanceField"):
        assert callable(getattr(api.RayTracer, m))
    assert callable(api.feature_normals)
    assert (api.FEATURE_NONE, api.FEATURE_FACE, api.FEATURE_SPHERE) == (-1, 0, 7)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'typedef char side_is_8_bytes[sizeof(rt_side) == 8 ? 1 : -1];\n'
                   'int main(void) { float p[4] = {0}; rt_hit h; rt_side s;\n'
                   '  h.prim = RT_PRIM_NONE; s.feature = RT_FEATURE_NONE; s.s = 0.0f;\n'
                   '  return rt_tracer_signed_distance(NULL, p, 1, &h, &s) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_signed_distance_device(NULL, p, 1, &h, &s, NULL) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_closest_sides(NULL, p, &h, 1, 1, &s) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_closest_sides_device(NULL, p, &h, 1, 1, &s, NULL) == RT_ERR_INVALID &&\n'
                   '         RT_FEATURE_FACE == 0 && RT_FEATURE_SPHERE == 7 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_the_signed_queries_and_rejects_vectors_that_do_not_fit(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> pts(8, 0.0f), five(5, 0.0f); std::vector<rt_hit> hits(3); std::vector<rt_side> sides(3);\n'
                   '  if (r.SignedDistance(five, hits, sides) || hits.size() != 3 || sides.size() != 3) return 1;\n'
                   '  if (!r.SignedDistance(five).empty()) return 2;\n'
                   '  if (r.ClosestSides(pts, hits, sides) || sides.size() != 3) return 3;      // 3 records for 2 points\n'
                   '  const bool ok = r.SignedDistance(pts, hits, sides);\n'
                   '  if (ok != r.Valid()) return 4;\n'
                   '  if (ok && (hits.size() != 2 || sides.size() != 2 || hits[0].prim != RT_PRIM_NONE ||\n'
                   '             sides[0].feature != RT_FEATURE_NONE || sides[0].s != 0.0f || r.SignedDistance(pts).size() != 2)) return 5;\n'
                   '  if (ok && (!r.ClosestSides(pts, hits, sides) || sides.size() != 2 || sides[1].feature != RT_FEATURE_NONE)) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
