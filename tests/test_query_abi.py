"""CPU checks of the ray-query boundary (rt_tracer_intersect / _device, rt_tracer_pick, rt_tracer_focus_at): the rt_hit
layout, argument checks that need no device, the C++ class and both command lines, and the test-side expected-hit scan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from query_expect import HIT_DTYPE, expected_hits, edge_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")


def test_rt_hit_layout():
    from raytracertest_amd import api
    assert api.HIT_DTYPE == HIT_DTYPE and api.HIT_DTYPE.itemsize == 16
    assert [api.HIT_DTYPE.fields[k][1] for k in ("t", "u", "v", "prim")] == [0, 4, 8, 12]
    assert api.PRIM_NONE == -1
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "typedef struct rt_hit { float t, u, v; int32_t prim; } rt_hit;" in hdr and "#define RT_PRIM_NONE (-1)" in hdr


def test_rt_hit_layout_in_c(tmp_path):
    src = tmp_path / "hit.c"
    src.write_text('#include <stddef.h>\n#include "rt_mi355x.h"\n'
                   'typedef char size_ok[sizeof(rt_hit) == 16 ? 1 : -1];\n'
                   'typedef char off_ok[offsetof(rt_hit, t) == 0 && offsetof(rt_hit, u) == 4 && offsetof(rt_hit, v) == 8 && '
                   'offsetof(rt_hit, prim) == 12 ? 1 : -1];\n'
                   'int main(void) { rt_hit h; h.prim = RT_PRIM_NONE; return rt_tracer_pick(NULL, NULL, 0, &h, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hit.o")], check=True)


def test_query_exports_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    rays = np.zeros((4, 6), np.float32)
    hits = np.zeros(4, HIT_DTYPE)
    pix = np.zeros((4, 2), np.uint32)
    f = ctypes.c_float()
    assert L.rt_tracer_intersect(None, rays.ctypes.data, 4, hits.ctypes.data) == 1
    assert L.rt_tracer_intersect_device(None, rays.ctypes.data, 4, hits.ctypes.data, None) == 1
    assert L.rt_tracer_pick(None, pix.ctypes.data, 4, hits.ctypes.data, None) == 1
    assert L.rt_tracer_focus_at(None, 0, 0, ctypes.byref(f)) == 1
    for name in ("rt_tracer_intersect", "rt_tracer_intersect_device", "rt_tracer_pick", "rt_tracer_focus_at"):
        assert name in api.ABI_SYMBOLS and hasattr(L, name)


def test_cpp_header_with_queries_compiles_strict(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<math::vec3> rays(2); std::vector<rt_hit> hits; rt_hit h; math::vec3 ray[2]; float f = 0;\n'
                   '  const bool ok = r.Intersect(rays, hits) | r.Pick(math::uvec2(1, 1), h) | r.Pick(math::uvec2(1, 1), h, ray) |\n'
                   '                  r.FocusAt(math::uvec2(1, 1)) | r.FocusAt(math::uvec2(1, 1), &f);\n'
                   '  return ok ? 0 : 1;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", str(tmp_path / "q")], check=True)


def test_cpp_query_driver_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "query_driver.cpp"), "-L" + LIBDIR, "-lrt_mi355x",
                    "-Wl,-rpath," + LIBDIR, "-pthread", "-o", str(tmp_path / "qd")], check=True)


def test_cli_help_lists_pick_and_focus(tmp_path):
    exe = os.path.join(LIBDIR, "rt_cli")
    if not os.path.exists(exe):
        exe = str(tmp_path / "rt_cli")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                        "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--pick X,Y" in out.stdout and "--focus X,Y" in out.stdout
    out = subprocess.run([exe, "--pick", "3"], capture_output=True, text=True)
    assert out.returncode == 2 and "X,Y" in out.stderr
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--pick X,Y" in py.stdout and "--focus X,Y" in py.stdout
    from raytracertest_amd.cli import build_parser
    a = build_parser().parse_args(["--pick", "12,34", "--focus", "5,6"])
    assert a.pick == (12, 34) and a.focus == (5, 6)
    a = build_parser().parse_args([])
    assert a.pick is None and a.focus is None


@pytest.mark.parametrize("contract", [0, 1])
def test_expected_hit_helper_reproduces_the_triangle_kats(orc, kats, contract):
    for c in kats:
        ray = orc.ray_make(c["origin"], c["dir"], True, contract)
        rows = np.zeros((3, 4), np.float32)
        rows[:, :3] = [c["a"], c["b"], c["c"]]
        h = expected_hits(orc, ray[None], rows, contract=contract)[0]
        assert (h["prim"] == 0) == c["hit"], c["name"]
        if c["hit"]:
            assert int(h["t"].view(np.uint32)) == int(c["t_bits"], 16), c["name"]
            assert h["u"] == np.float32(c["u"]) and h["v"] == np.float32(c["v"]), c["name"]
        else:
            assert (h["t"], h["u"], h["v"]) == (0, 0, 0)


def test_expected_hit_helper_rules(orc):
    """Two copies of one triangle and one behind the origin: the lower index wins ties under both rules; the farthest rule
    keeps the negative t of a hit behind the origin, the nearest rule does not."""
    tri = np.array([[0, 0, -10, 0], [1, 0, -10, 0], [0, 1, -10, 0]], np.float32)
    back = tri.copy()
    back[:, 2] = 10.0
    back = back[[0, 2, 1]]                                   # facing the ray coming from the other side
    rows = np.concatenate([tri, tri, back])
    ray = np.array([[0.2, 0.2, 0, 0, 0, -1], [0.2, 0.2, 20, 0, 0, 1]], np.float32)
    far = expected_hits(orc, ray, rows)
    near = expected_hits(orc, ray, rows, nearest=True)
    assert far["prim"][0] == 0 and near["prim"][0] == 0 and far["t"][0] == 10.0
    assert far["prim"][1] == 2 and far["t"][1] == -10.0 and near["prim"][1] == -1 and near["t"][1] == 0
    e = edge_rows(rows)
    assert np.array_equal(e[1::3, :3] + e[0::3, :3], rows[1::3, :3])
