"""CPU checks of the region query's boundary (rt_tracer_overlap / _device): declared, exported, argument checks that need no
device, the struct-free signature, the Python and C++ classes and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_overlap", "rt_tracer_overlap_device")


def test_symbols_are_declared_exported_in_header_order_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert (hdr.index("rt_tracer_closest_sides_device(") < hdr.index("---- region queries") < hdr.index("rt_tracer_overlap(")
            < hdr.index("rt_tracer_overlap_device(") < hdr.index("rt_tracer_create_multi("))
    s = api.ABI_SYMBOLS
    assert s.index("rt_tracer_closest_sides_device") < s.index(NEW[0]) < s.index(NEW[1]) and len(set(s)) == len(s)
    boxes = np.zeros((4, 8), np.float32)
    after = np.full(4, -1, np.int32)
    prims = np.zeros((4, 4), np.int32)
    counts = np.zeros(4, np.uint32)
    a = (boxes.ctypes.data, after.ctypes.data, 4, 4, prims.ctypes.data, counts.ctypes.data)
    assert L.rt_tracer_overlap(None, *a) == 1
    assert L.rt_tracer_overlap_device(None, *a, None) == 1
    assert L.rt_tracer_overlap(None, None, None, 0, 4, None, None) == 1
    assert L.rt_tracer_overlap(None, boxes.ctypes.data, None, 4, 17, prims.ctypes.data, counts.ctypes.data) == 1
    assert L.rt_tracer_overlap_device(None, None, None, 4, 0, None, None, None) == 1


def test_the_signature_is_struct_free_and_the_rule_is_written_out():
    """Plain float / int32 / uint32 arrays: a caller needs no type of the header to call it.  The header states the rule
    operation by operation, why scan and tree agree, and that the slack has no effect."""
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    sec = hdr[hdr.index("---- region queries"):hdr.index("---- one frame sharded")]
    assert ("int  rt_tracer_overlap(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                       uint32_t* counts);") in sec
    assert ("int  rt_tracer_overlap_device(rt_tracer* t, const float* boxes, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                              uint32_t* counts, void* stream);") in sec
    assert "rt_hit" not in sec and "typedef" not in sec
    for text in ("1. Box step", "2. Plane step", "3. The nine axes", "c = 0.5*lo + 0.5*hi", "rt_dbg_query_accel_slack has no effect",
                 "Why scan and tree agree", "rounded outward", "restarting the list and the count", "0 .. RT_MAX_HITS"):
        assert text in sec, text


def test_python_class_has_the_methods_and_checks_boxes_and_max_hits():
    from raytracertest_amd import api
    R = api.RayTracer
    for m in ("Overlap", "_overlap_tensor", "OverlapAll", "Voxelize", "voxel_boxes"):
        assert callable(getattr(R, m))
    k = R._overlap_hits
    assert k(0) == 0 and k(16) == 16 and k(4.0) == 4
    for bad in (17, -1, 2.5):
        with pytest.raises(ValueError, match="max_hits"):
            k(bad)
    with pytest.raises(ValueError, match=r"^Overlap: max_hits = 17 \(0 to 16\)$"):
        k(17)
    lo, hi = np.float32([[0, 1, 2], [3, 4, 5]]), np.float32([[6, 7, 8], [9, 10, 11]])
    want = np.float32([[0, 1, 2, 0, 6, 7, 8, 0], [3, 4, 5, 0, 9, 10, 11, 0]])
    for form in ((lo, hi), np.c_[lo, hi], want, [0, 1, 2, 6, 7, 8]):
        got = R._boxes_array("Overlap", form)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want[:got.shape[0]])
    for bad in (np.zeros((3, 5)), 1.0, (lo, hi[:1])):
        with pytest.raises(ValueError, match="Overlap"):
            R._boxes_array("Overlap", bad)


def test_voxel_boxes_share_their_faces_bit_for_bit():
    from raytracertest_amd import api
    b = api.RayTracer.voxel_boxes((-0.3, 0.1, 7.0), (0.1, 0.25, 1.0 / 3.0), (5, 2, 3)).reshape(5, 2, 3, 8)
    assert b.dtype == np.float32
    for a in range(3):
        lo, hi = np.moveaxis(b[..., a], a, 0), np.moveaxis(b[..., 4 + a], a, 0)
        assert np.array_equal(hi[:-1], lo[1:])                           # neighbours share the face
        o, s = np.float32((-0.3, 0.1, 7.0)[a]), np.float32((0.1, 0.25, 1.0 / 3.0)[a])
        i = np.arange(lo.shape[0], dtype=np.float32).reshape((-1, 1, 1))
        assert np.array_equal(lo, np.broadcast_to(o + s * i, lo.shape)) and np.array_equal(hi, np.broadcast_to(o + s * (i + np.float32(1)), hi.shape))
    assert api.RayTracer.voxel_boxes((0, 0, 0), 1.0, (0, 2, 2)).shape == (0, 8)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float b[8] = {0}; int32_t prims[RT_MAX_HITS]; int32_t after = RT_PRIM_NONE; uint32_t c;\n'
                   '  return rt_tracer_overlap(NULL, b, &after, 1, RT_MAX_HITS, prims, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_overlap_device(NULL, b, NULL, 1, 0, NULL, &c, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_overlap_and_rejects_bad_vectors_and_counts(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> boxes(16, 0.0f), nine(9, 0.0f); std::vector<int32_t> prims(3), after(3); std::vector<uint32_t> counts(5);\n'
                   '  if (r.Overlap(nine, 4, prims, counts) || prims.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.Overlap(boxes, RT_MAX_HITS + 1, prims, counts) || prims.size() != 3) return 2;\n'
                   '  if (r.Overlap(boxes, 4, prims, counts, after) || prims.size() != 3) return 3;       // a cursor of another length\n'
                   '  if (!r.Overlap(nine, 4).empty() || !r.Overlap(boxes, 17).empty()) return 4;\n'
                   '  const bool ok = r.Overlap(boxes, 3, prims, counts);\n'
                   '  if (ok != r.Valid()) return 5;\n'
                   '  if (ok && (prims.size() != 6 || counts.size() != 2 || counts[0] != 0 || prims[0] != RT_PRIM_NONE ||\n'
                   '             r.Overlap(boxes).size() != 2 || !r.Overlap(boxes, 0, prims, counts) || !prims.empty())) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_the_overlap_query(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--overlap X0,Y0,Z0,X1,Y1,Z1[,K]" in out.stdout
    for bad in ("3", "1,2,3,4,5", "1,2,3,4,5,", "1,2,3,4,5,x", "1,2,3,4,5,6,-1", "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,x"):
        out = subprocess.run([exe, "--overlap", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X0,Y0,Z0,X1,Y1,Z1[,K]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "X0,Y0,Z0,X1,Y1,Z1[,K]" in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--overlap", "0.5,1,2,3,4,5"]).overlap == (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 8)
    assert build_parser().parse_args(["--overlap=-0.5,1,2,3,4,5,0"]).overlap == (-0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 0)
    assert build_parser().parse_args([]).overlap is None
    for bad in ("1,2,3,4,5", "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,x", "1,2,3,4,5,6,-1"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--overlap", bad])
