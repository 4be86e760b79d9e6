"""CPU checks of the triangle-shaped region query's boundary (rt_tracer_overlap_triangles / _device): declared, exported,
argument checks that need no device, the struct-free signature and the rule in the header, the Python and C++ classes and both
command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_overlap_triangles", "rt_tracer_overlap_triangles_device")


def test_symbols_are_declared_exported_in_header_order_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert (hdr.index("---- region queries") < hdr.index("rt_tracer_overlap_device(") < hdr.index("rt_tracer_overlap_triangles(")
            < hdr.index("rt_tracer_overlap_triangles_device(") < hdr.index("---- one frame sharded") < hdr.index("---- swept queries")
            < hdr.index("rt_tracer_create_multi("))
    s = api.ABI_SYMBOLS
    assert s.index("rt_tracer_overlap_device") < s.index(NEW[0]) < s.index(NEW[1]) < s.index("rt_tracer_sphere_cast") and len(set(s)) == len(s)
    tris = np.zeros((4, 12), np.float32)
    after = np.full(4, -1, np.int32)
    prims = np.zeros((4, 4), np.int32)
    counts = np.zeros(4, np.uint32)
    a = (tris.ctypes.data, after.ctypes.data, 4, 4, prims.ctypes.data, counts.ctypes.data)
    assert L.rt_tracer_overlap_triangles(None, *a) == 1
    assert L.rt_tracer_overlap_triangles_device(None, *a, None) == 1
    assert L.rt_tracer_overlap_triangles(None, None, None, 0, 4, None, None) == 1
    assert L.rt_tracer_overlap_triangles(None, tris.ctypes.data, None, 4, 17, prims.ctypes.data, counts.ctypes.data) == 1
    assert L.rt_tracer_overlap_triangles_device(None, None, None, 4, 0, None, None, None) == 1


def test_the_signature_is_struct_free_and_the_rule_is_written_out():
    """Plain float / int32 / uint32 arrays: a caller needs no type of the header to call it.  The header states the rule
    operation by operation, the shared-corner guarantee, the sphere rule, and why scan and tree agree."""
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    sec = hdr[hdr.index("rt_tracer_overlap_device("):hdr.index("---- one frame sharded")]
    assert ("int  rt_tracer_overlap_triangles(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                                 uint32_t* counts);") in sec
    assert ("int  rt_tracer_overlap_triangles_device(rt_tracer* t, const float* tris, const int32_t* after, size_t n, uint32_t max_hits,\n"
            "                                        int32_t* prims, uint32_t* counts, void* stream);") in sec
    assert "rt_hit" not in sec and "typedef" not in sec
    for text in ("n x 12 floats", "three 16-byte loads", "1. Box step", "2. Move by -P0", "3. Seventeen axes", "f = {e1, c - b, a - c}",
                 "g = {p1, p2 - p1, p2}", "the nine f_i x g_j", "the three n x f_i", "the three m x g_j", "0, x.p1, x.p2",
                 "EVERY record\n *                    projection is > EVERY query projection", "the axis never separates",
                 "bit-equal to A, B or C of a record makes that record accepted", "All nine query coordinates are finite",
                 "accepts NOTHING, spheres included", "d2min <= r*r && r*r <= d2max", "v0 = P0, e1 = p1, e2 = p2", "NO inflation",
                 "restarting the list and the count", "no rho, no slack and no conditioning clause", "0 .. RT_MAX_HITS",
                 "tris must be 16-byte aligned"):
        assert text in sec, text


def test_python_class_has_the_methods_and_checks_triangles_and_max_hits():
    from raytracertest_amd import api
    R = api.RayTracer
    for m in ("OverlapTriangles", "_overlap_triangles_tensor", "OverlapTrianglesAll", "SelfIntersections", "self_pairs", "scene_corners"):
        assert callable(getattr(R, m))
    assert "fold between neighbours" in R.SelfIntersections.__doc__.lower()
    c = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    want = np.zeros((2, 3, 4), np.float32)
    want[:, :, :3] = c
    want = want.reshape(2, 12)
    for form in (c, c.reshape(2, 9), want, list(range(9))):
        got = R._triangles_array("OverlapTriangles", form)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want[:got.shape[0]])
    for bad in (np.zeros((3, 5)), 1.0, np.zeros((3, 8)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match="OverlapTriangles"):
            R._triangles_array("OverlapTriangles", bad)
    # the corners SelfIntersections compares: the uploaded vertices, or A, fl(v0 + e1), fl(v0 + e2) of the edge layout
    rows = np.zeros((1, 3, 4), np.float32)
    rows[0, :, :3] = [[1, 2, 3], [0.1, 0.2, 0.3], [4, 5, 6]]
    assert np.array_equal(R.scene_corners(rows.reshape(-1, 4)), rows[:, :, :3])
    e = R.scene_corners(rows.reshape(-1, 4), True)
    assert np.array_equal(e[0, 0], rows[0, 0, :3]) and np.array_equal(e[0, 1], rows[0, 0, :3] + rows[0, 1, :3]) and e.dtype == np.float32
    # pairs: i < j, accepted, no corner in common; a NaN corner equals nothing
    corners = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [5, 5, 5], [6, 6, 6]], [[7, 7, 7], [8, 8, 8], [9, 9, np.nan]],
                          [[9, 9, np.nan], [2, 2, 2], [3, 3, 3]]])
    prims = np.int32([0, 1, 2, 4, 0, 1, 0, 2, 3, 2, 3])
    offsets = np.int64([0, 4, 6, 9, 11])
    assert R.self_pairs(corners, prims, offsets).tolist() == [[0, 2], [2, 3]]
    assert R.self_pairs(corners, np.zeros(0, np.int32), np.zeros(5, np.int64)).shape == (0, 2)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float t[12] = {0}; int32_t prims[RT_MAX_HITS]; int32_t after = RT_PRIM_NONE; uint32_t c;\n'
                   '  return rt_tracer_overlap_triangles(NULL, t, &after, 1, RT_MAX_HITS, prims, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_overlap_triangles_device(NULL, t, NULL, 1, 0, NULL, &c, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_overlap_triangles_and_rejects_bad_vectors_and_counts(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> tris(24, 0.0f), nine(9, 0.0f); std::vector<int32_t> prims(3), after(3); std::vector<uint32_t> counts(5);\n'
                   '  if (r.OverlapTriangles(nine, 4, prims, counts) || prims.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.OverlapTriangles(tris, RT_MAX_HITS + 1, prims, counts) || prims.size() != 3) return 2;\n'
                   '  if (r.OverlapTriangles(tris, 4, prims, counts, after) || prims.size() != 3) return 3;       // a cursor of another length\n'
                   '  if (!r.OverlapTriangles(nine, 4).empty() || !r.OverlapTriangles(tris, 17).empty()) return 4;\n'
                   '  const bool ok = r.OverlapTriangles(tris, 3, prims, counts);\n'
                   '  if (ok != r.Valid()) return 5;\n'
                   '  if (ok && (prims.size() != 6 || counts.size() != 2 || counts[0] != 0 || prims[0] != RT_PRIM_NONE ||\n'
                   '             r.OverlapTriangles(tris).size() != 2 || !r.OverlapTriangles(tris, 0, prims, counts) || !prims.empty())) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_the_triangle_query(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    form = "X0,Y0,Z0,X1,Y1,Z1,X2,Y2,Z2[,K]"
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--overlap-tri " + form in out.stdout
    for bad in ("3", "1,2,3,4,5,6", "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,7,8,", "1,2,3,4,5,6,7,8,x", "1,2,3,4,5,6,7,8,9,-1",
                "1,2,3,4,5,6,7,8,9,10,11", "1,2,3,4,5,6,7,8,9,x"):
        out = subprocess.run([exe, "--overlap-tri", bad], capture_output=True, text=True)
        assert out.returncode == 2 and form in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and form in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--overlap-tri", "0.5,1,2,3,4,5,6,7,8"]).overlap_tri == (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 8)
    assert build_parser().parse_args(["--overlap-tri=-0.5,1,2,3,4,5,6,7,8,0"]).overlap_tri == (-0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 0)
    a = build_parser().parse_args(["--overlap", "0,0,0,1,1,1"])                       # the box option still stands alone
    assert a.overlap_tri is None and a.overlap == (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 8)
    for bad in ("1,2,3,4,5,6", "1,2,3,4,5,6,7,8,9,10,11", "1,2,3,4,5,6,7,8,9,x", "1,2,3,4,5,6,7,8,9,-1"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--overlap-tri", bad])
