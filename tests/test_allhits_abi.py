"""CPU checks of the all-hits query's boundary (rt_tracer_intersect_all / _device): declared, exported, argument checks that
need no device, the Python and C++ classes and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from query_expect import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_intersect_all", "rt_tracer_intersect_all_device")


def test_symbols_are_declared_exported_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "#define RT_MAX_HITS 16u" in hdr and api.RT_MAX_HITS == 16
    segs = np.zeros((4, 8), np.float32)
    hits = np.zeros((4, 16), HIT_DTYPE)
    counts = np.zeros(4, np.uint32)
    assert L.rt_tracer_intersect_all(None, segs.ctypes.data, 4, 16, hits.ctypes.data, counts.ctypes.data) == 1
    assert L.rt_tracer_intersect_all_device(None, segs.ctypes.data, 4, 16, hits.ctypes.data, counts.ctypes.data, None) == 1
    assert L.rt_tracer_intersect_all(None, None, 0, 1, None, None) == 1
    assert L.rt_tracer_intersect_all_device(None, None, 4, 1, None, None, None) == 1


def test_python_class_has_intersect_all():
    from raytracertest_amd import api
    for m in ("IntersectAll", "_intersect_all_tensor"):
        assert callable(getattr(api.RayTracer, m))
    k = api.RayTracer._max_hits
    assert k("IntersectAll", 1) == 1 and k("IntersectAll", 16) == 16 and k("IntersectAll", 4.0) == 4
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="max_hits"):
            k("IntersectAll", bad)
    with pytest.raises(ValueError, match=r"^IntersectAll: max_hits = 0 \(1 to 16\)$"):
        k("IntersectAll", 0)


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float s[8] = {0}; rt_hit h[RT_MAX_HITS]; uint32_t c = 0;\n'
                   '  h[0].prim = RT_PRIM_NONE;\n'
                   '  return rt_tracer_intersect_all(NULL, s, 1, RT_MAX_HITS, h, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_intersect_all_device(NULL, s, 1, RT_MAX_HITS, h, &c, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_intersect_all_and_rejects_an_odd_segment_vector(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> segs(16, 0.0f), odd(9, 0.0f); std::vector<rt_hit> hits(3); std::vector<uint32_t> counts(5);\n'
                   '  if (r.IntersectAll(odd, 4, hits, counts) || hits.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.IntersectAll(segs, 0, hits, counts) || r.IntersectAll(segs, RT_MAX_HITS + 1, hits, counts)) return 2;\n'
                   '  const bool ok = r.IntersectAll(segs, 4, hits, counts);\n'
                   '  return ok == r.Valid() ? 0 : 3;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_hits(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--hits X,Y[,K]" in out.stdout
    for bad in ("3", "3,4,", "3,4,x", "a,b,2"):
        out = subprocess.run([exe, "--hits", bad], capture_output=True, text=True)
        assert out.returncode == 2 and "X,Y[,K]" in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--hits X,Y[,K]" in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--hits", "12,34"]).hits == (12, 34, 8)
    assert build_parser().parse_args(["--hits", "12,34,3"]).hits == (12, 34, 3)
    assert build_parser().parse_args([]).hits is None
