"""CPU checks of the section queries' boundary (rt_tracer_section / rt_tracer_section_segments and their _device forms):
declared, exported, argument checks that need no device, the signatures, rt_cut and the rule in the header, the Python helpers
that build the planes, the C++ class and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import section_expect as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_section", "rt_tracer_section_device", "rt_tracer_section_segments", "rt_tracer_section_segments_device")


def test_symbols_are_declared_exported_in_header_order_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert (hdr.index("---- section queries") < hdr.index(NEW[0] + "(") < hdr.index(NEW[1] + "(") < hdr.index("typedef struct rt_cut")
            < hdr.index(NEW[2] + "(") < hdr.index(NEW[3] + "(") < hdr.index("rt_tracer_create_multi("))
    s = api.ABI_SYMBOLS
    assert s.index("rt_tracer_overlap_hexahedra_device") < s.index(NEW[0]) < s.index(NEW[3]) < s.index("rt_tracer_sphere_cast") and len(set(s)) == len(s)
    planes = np.zeros((4, 8), np.float32)
    after = np.full(4, -1, np.int32)
    prims = np.full((4, 4), 77, np.int32)
    counts = np.full(4, 99, np.uint32)
    cuts = np.full((4, 4, 8), 5.0, np.float32)
    a = (planes.ctypes.data, after.ctypes.data, 4, 4, prims.ctypes.data, counts.ctypes.data)
    assert L.rt_tracer_section(None, *a) == 1                            # RT_ERR_INVALID
    assert L.rt_tracer_section_device(None, *a, None) == 1
    assert L.rt_tracer_section(None, None, None, 0, 4, None, None) == 1
    assert L.rt_tracer_section(None, planes.ctypes.data, None, 4, 17, prims.ctypes.data, counts.ctypes.data) == 1
    assert L.rt_tracer_section_device(None, None, None, 4, 0, None, None, None) == 1
    b = (planes.ctypes.data, prims.ctypes.data, 4)
    for per, side in ((4, 0), (0, 0), (17, 0), (4, 2)):
        assert L.rt_tracer_section_segments(None, *b, per, side, cuts.ctypes.data) == 1
        assert L.rt_tracer_section_segments_device(None, *b, per, side, cuts.ctypes.data, None) == 1
    assert (prims == 77).all() and (counts == 99).all() and (cuts == 5.0).all()        # the outputs are untouched


def test_the_signatures_rt_cut_and_the_rule_are_written_out():
    from raytracertest_amd import api
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    sec = hdr[hdr.index("---- section queries"):hdr.index("---- one frame sharded over several GPUs, continued")]
    assert ("int  rt_tracer_section(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                       uint32_t* counts);") in sec
    assert ("int  rt_tracer_section_device(rt_tracer* t, const float* planes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                              uint32_t* counts, void* stream);") in sec
    assert ("int  rt_tracer_section_segments(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane, uint32_t side,\n"
            "                                rt_cut* cuts);") in sec
    assert ("int  rt_tracer_section_segments_device(rt_tracer* t, const float* planes, const int32_t* prims, size_t n, uint32_t per_plane,\n"
            "                                       uint32_t side, rt_cut* cuts, void* stream);") in sec
    assert "typedef struct rt_cut { float p0[3]; int32_t kind; float p1[3]; int32_t features; } rt_cut;" in sec
    for text in ("n x 8 floats: nx ny nz d0 d1 _ _ _", "two 16-byte loads", "accepts NOTHING, spheres included", "n = 0 is not special",
                 "p(X) = (nx*X.x + ny*X.y) + nz*X.z", "none of p(A), p(B), p(C) is a NaN", "closed: touching counts",
                 "rn = r * sqrt((nx*nx + ny*ny) + nz*nz)", "pc - rn <= d1 and pc + rn >= d0", "xlo = (n_axis >= 0 ? lo : hi)",
                 "pmin > d1 or pmax < d0", "a NaN never skips", "rounding is monotone", "NO\n * inflation",
                 "rt_dbg_query_accel_slack has no effect", "0 .. RT_MAX_HITS", "planes must be 16-byte aligned",
                 "t = sL / (sL - sU)", "X = L + t*(U - L)", "below end L towards the above end U", "bit-equal points",
                 "leaves the\n *                      above side", "n x (e1 x e2)", "counter-clockwise seen from the tip of n",
                 "f0 | f1 << 8", "0 / 1 / 2 the edge AB / BC / CA, 4 / 5 / 6 the corner A / B / C", "|pc - d| <= rn",
                 "per_plane 1 .. RT_MAX_HITS and side 0 or 1", "never cancels or joins a running Trace", "answers from its first band"):
        assert text in sec, text
    for name, value in (("NONE", 0), ("SEGMENT", 1), ("TOUCH", 2), ("COPLANAR", 3), ("CIRCLE", 4)):
        assert "#define RT_CUT_%-8s %d\n" % (name, value) in sec
        assert getattr(api, "CUT_" + name) == value == getattr(se, "CUT_" + name)
    assert api.CUT_DTYPE == se.CUT_DTYPE and api.CUT_DTYPE.itemsize == 32
    old = hdr[hdr.index("---- region queries"):hdr.index("---- one frame sharded")]
    assert "a cut plane" not in old and "rt_tracer_section" in old       # the advice of two triangles for a cut plane is gone
    kern = open(os.path.join(ROOT, "raytracertest_amd", "csrc", "rt_section.hpp")).read()
    for text in ("Rounding is monotone", "pmin = p(xlo) <= p(P) <= p(xhi) = pmax", "b.rho is not read", "a forwarding layer changes"):
        assert text in kern, text


def test_python_class_has_the_methods_and_the_plane_helpers():
    from raytracertest_amd import api
    R = api.RayTracer
    for m in ("Section", "SectionAll", "SectionSegments", "Slice", "plane_rows", "_planes_array"):
        assert callable(getattr(R, m))
    p = R.plane_rows((1, 2, 3), [4, 5])
    assert p.dtype == np.float32 and p.tolist() == [[1, 2, 3, 4, 4, 0, 0, 0], [1, 2, 3, 5, 5, 0, 0, 0]]
    p = R.plane_rows([[1, 0, 0], [0, 1, 0]], -np.inf, [1.0, 2.0])
    assert p.tolist() == [[1, 0, 0, -np.inf, 1, 0, 0, 0], [0, 1, 0, -np.inf, 2, 0, 0, 0]]
    assert np.array_equal(p, se.planes_of([[1, 0, 0], [0, 1, 0]], -np.inf, [1.0, 2.0]))
    assert R.plane_rows((0, 0, 1), []).shape == (0, 8) and R.plane_rows((0, 0, 1), 0.5).shape == (1, 8)
    want = np.float32([[1, 2, 3, 4, 5, 0, 0, 0]])
    for form in (want, want[:, :5], want[0], [1, 2, 3, 4, 5]):
        got = R._planes_array("Section", form)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)
    assert R._planes_array("Section", [1, 2, 3, 4]).tolist() == [[1, 2, 3, 4, 4, 0, 0, 0]]
    for bad in (np.zeros((3, 6)), 1.0, np.zeros((3, 3)), np.zeros((2, 7))):
        with pytest.raises(ValueError, match="Section"):
            R._planes_array("Section", bad)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float p[8] = {0}; int32_t prims[RT_MAX_HITS]; int32_t after = RT_PRIM_NONE; uint32_t c; rt_cut cut[RT_MAX_HITS];\n'
                   '  return sizeof(rt_cut) == 32 && RT_CUT_NONE == 0 && RT_CUT_CIRCLE == 4 &&\n'
                   '         rt_tracer_section(NULL, p, &after, 1, RT_MAX_HITS, prims, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_section_device(NULL, p, NULL, 1, 0, NULL, &c, NULL) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_section_segments(NULL, p, prims, 1, RT_MAX_HITS, 0, cut) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_section_segments_device(NULL, p, prims, 1, 1, 1, cut, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_section_and_rejects_bad_vectors_and_counts(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> planes(16, 0.0f), odd(12, 0.0f); std::vector<int32_t> prims(3), after(3); std::vector<uint32_t> counts(5);\n'
                   '  std::vector<rt_cut> cuts(7);\n'
                   '  if (r.Section(odd, 4, prims, counts) || prims.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.Section(planes, RT_MAX_HITS + 1, prims, counts) || prims.size() != 3) return 2;\n'
                   '  if (r.Section(planes, 4, prims, counts, after) || prims.size() != 3) return 3;       // a cursor of another length\n'
                   '  if (!r.Section(odd, 4).empty() || !r.Section(planes, 17).empty()) return 4;\n'
                   '  if (r.SectionSegments(planes, prims, 4, 0, cuts) || r.SectionSegments(planes, prims, 0, 0, cuts) || cuts.size() != 7) return 7;\n'
                   '  const bool ok = r.Section(planes, 3, prims, counts);\n'
                   '  if (ok != r.Valid()) return 5;\n'
                   '  if (ok && (prims.size() != 6 || counts.size() != 2 || counts[0] != 0 || prims[0] != RT_PRIM_NONE || r.Section(planes).size() != 2 ||\n'
                   '             !r.SectionSegments(planes, prims, 3, 1, cuts) || cuts.size() != 6 || cuts[0].kind != RT_CUT_NONE ||\n'
                   '             r.SectionSegments(planes, prims, 3, 2, cuts) || r.SectionSegments(planes, prims, 17, 0, cuts) || cuts.size() != 6 ||\n'
                   '             !r.Section(planes, 0, prims, counts) || !prims.empty())) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_the_section_query(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    form = "NX,NY,NZ,D0[,D1[,K]]"
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--section " + form in out.stdout and "prim kind features x0 y0 z0 x1 y1 z1" in out.stdout
    for bad in ("3", "1,2,3", "1,2,3,", "1,2,3,4,", "1,2,3,4,5,", "1,2,3,4,5,x", "1,2,3,4,5,-1", "1,2,3,4,5,6,7", "1,2,3,x"):
        out = subprocess.run([exe, "--section", bad], capture_output=True, text=True)
        assert out.returncode == 2 and form in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and form in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--section", "0,0,1,-3"]).section == (0.0, 0.0, 1.0, -3.0, -3.0, 8)
    assert build_parser().parse_args(["--section=0,0,1,-3,-2.5"]).section == (0.0, 0.0, 1.0, -3.0, -2.5, 8)
    assert build_parser().parse_args(["--section=0,0,1,-inf,-2.5,0"]).section == (0.0, 0.0, 1.0, -np.inf, -2.5, 0)
    assert build_parser().parse_args(["--overlap", "0,0,0,1,1,1"]).section is None
    for bad in ("1,2,3", "1,2,3,4,5,-1", "1,2,3,4,5,x", "1,2,3,4,5,6,7"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--section", bad])
