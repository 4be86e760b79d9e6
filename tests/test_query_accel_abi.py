"""CPU checks of the query-acceleration boundary: rt_tracer_set_query_accel, rt_tracer_query_accel_info and the two rt_dbg_*
entry points are declared and exported and reject null handles; the C++ class, the Python class and both command lines know
the switch."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_set_query_accel", "rt_tracer_query_accel_info", "rt_dbg_bvh_build", "rt_dbg_query_accel_slack",
       "rt_dbg_query_stack_cap")


def test_new_symbols_are_declared_exported_and_reject_null_handles():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "#define RT_QUERY_SCAN 0u" in hdr and "#define RT_QUERY_BVH  1u" in hdr
    assert "well" in hdr.lower() and "2^-10" in hdr                      # the contract's condition is stated
    assert "struct rt_options" in hdr and "query_accel" not in hdr.split("} rt_options;")[0]   # rt_options did not grow
    out = (ctypes.c_uint64 * 8)()
    assert L.rt_tracer_set_query_accel(None, 1) == 1
    assert L.rt_tracer_query_accel_info(None, out) == 1
    assert L.rt_dbg_query_accel_slack(None, 1000) == 1
    assert L.rt_dbg_query_stack_cap(None, 0) == 1
    assert "test-only" in hdr.split("rt_dbg_query_stack_cap(")[0][-700:].lower()       # documented as what it is
    assert L.rt_dbg_bvh_build(None, 0, 0, None, 0, None, 0, out) == 1
    assert (api.QUERY_SCAN, api.QUERY_BVH) == (0, 1)
    assert api.BVH_NODE_DTYPE.itemsize == 128 and api.BVH_RECORD_DTYPE.itemsize == 48
    assert [api.BVH_NODE_DTYPE.fields[k][1] for k in ("lo", "hi", "child", "cmax")] == [0, 48, 96, 112]
    assert [api.BVH_RECORD_DTYPE.fields[k][1] for k in ("e2", "e1", "v0", "index")] == [0, 12, 24, 36]
    for m in ("SetQueryAcceleration", "QueryAccelInfo", "DebugQueryStackCap"):
        assert callable(getattr(api.RayTracer, m))


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { uint64_t info[8]; return rt_tracer_set_query_accel(NULL, RT_QUERY_BVH) == RT_ERR_INVALID &&\n'
                   '  rt_tracer_query_accel_info(NULL, info) == RT_ERR_INVALID && RT_QUERY_SCAN == 0u ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_the_switch(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  const bool ok = r.SetQueryAcceleration(true);\n'
                   '  const rt::RayTracer::QueryAccel a = r.QueryAccelInfo();\n'
                   '  return ok && a.bvh && !a.valid && a.nodes == 0 ? 0 : 1;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", str(tmp_path / "q")], check=True)


def test_command_lines_list_accel(tmp_path):
    exe = os.path.join(LIBDIR, "rt_cli")
    if not os.path.exists(exe):
        exe = str(tmp_path / "rt_cli")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                        "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--accel" in out.stdout
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and "--accel" in py.stdout
    from raytracertest_amd.cli import build_parser
    assert build_parser().parse_args(["--pick", "1,2", "--accel"]).accel is True
    assert build_parser().parse_args([]).accel is False


def test_documents_name_the_mode():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md", os.path.join("tools", "README.md")):
        assert "RT_QUERY_BVH" in open(os.path.join(ROOT, doc)).read() or "SetQueryAcceleration" in open(os.path.join(ROOT, doc)).read(), doc
