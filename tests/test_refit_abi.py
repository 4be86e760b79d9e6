"""CPU checks of the refit boundary: the three entry points of the update policy and the debug entry points are declared and
exported and reject null handles and an unknown policy; the C++ class and the Python class know them; rt_options did not grow."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_set_query_accel_update", "rt_tracer_query_accel_rebuild", "rt_tracer_query_accel_update_info",
       "rt_dbg_bvh_refit", "rt_dbg_query_tree_read")


def test_new_symbols_are_declared_exported_and_reject_bad_arguments():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW + ("rt_dbg_bvh_tree_cost",):
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "#define RT_ACCEL_REBUILD 0u" in hdr and "#define RT_ACCEL_REFIT   1u" in hdr
    assert "struct rt_options" in hdr and "accel" not in hdr.split("} rt_options;")[0]        # rt_options did not grow
    assert hdr.index("single-function device harnesses") < hdr.index("rt_dbg_bvh_refit(") < hdr.index("rt_dbg_query_tree_read(")
    out = (ctypes.c_uint64 * 8)()
    assert L.rt_tracer_set_query_accel_update(None, 1) == 1
    assert L.rt_tracer_set_query_accel_update(None, 2) == 1
    assert L.rt_tracer_query_accel_rebuild(None) == 1
    assert L.rt_tracer_query_accel_update_info(None, out) == 1
    assert L.rt_dbg_bvh_refit(None, 0, 0, None, 0, None, 0, out) == 1
    assert L.rt_dbg_query_tree_read(None, None, 0, None, 0, out) == 1
    assert L.rt_dbg_bvh_tree_cost(None, 0) == 0.0
    assert (api.ACCEL_REBUILD, api.ACCEL_REFIT) == (0, 1)
    for m in ("SetQueryAccelUpdate", "RebuildQueryAccel", "QueryAccelUpdateInfo", "query_tree"):
        assert callable(getattr(api.RayTracer, m))
    assert callable(api.bvh_refit) and callable(api.tree_cost)


def test_unknown_policy_is_rejected_before_anything_else():
    """The policy is checked on a handle as well; 2 is no policy.  (A handle needs a device: the source states the order.)"""
    src = open(os.path.join(ROOT, "raytracertest_amd", "csrc", "rt_query_api.hpp")).read()
    body = src.split("int rt_tracer_set_query_accel_update(rt_tracer* t, uint32_t policy) {")[1].split("\n}\n")[0]
    assert body.index("RT_ERR_INVALID") < body.index("policy != RT_ACCEL_REBUILD && policy != RT_ACCEL_REFIT") < body.index("api_mu")


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { uint64_t info[8]; return rt_tracer_set_query_accel_update(NULL, RT_ACCEL_REFIT) == RT_ERR_INVALID &&\n'
                   '  rt_tracer_query_accel_rebuild(NULL) == RT_ERR_INVALID && rt_tracer_query_accel_update_info(NULL, info) == RT_ERR_INVALID &&\n'
                   '  rt_dbg_bvh_refit(NULL, 0, 0, NULL, 0, NULL, 0, info) == RT_ERR_INVALID &&\n'
                   '  rt_dbg_query_tree_read(NULL, NULL, 0, NULL, 0, info) == RT_ERR_INVALID && RT_ACCEL_REBUILD == 0u ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_the_three_methods(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  const bool ok = r.SetQueryAccelUpdate(true) && r.RebuildQueryAccel();\n'
                   '  const rt::RayTracer::QueryAccelUpdate u = r.QueryAccelUpdateInfo();\n'
                   '  return ok && u.refit && u.refits == 0 && u.fallbacks == 0 && u.cost == 0.0 && u.costBuilt == 0.0 ? 0 : 1;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", str(tmp_path / "q")], check=True)


def test_documents_name_the_policy():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md", os.path.join("tools", "README.md")):
        assert "RT_ACCEL_REFIT" in open(os.path.join(ROOT, doc)).read() or "SetQueryAccelUpdate" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.3e" in design and "refit_level_kernel" in design
