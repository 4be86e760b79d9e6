"""CPU checks of the exposure query's boundary (rt_tracer_exposure, rt_tracer_exposure_device, rt_dbg_exposure_rays): declared,
exported, RT_MAX_DIRS, argument checks that need no device, the header as C99, and the Python and C++ classes."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_exposure", "rt_tracer_exposure_device", "rt_dbg_exposure_rays")


def test_symbols_are_declared_exported_and_reject_null_handles():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert hdr.index("rt_tracer_occluded_device(") < hdr.index("rt_tracer_exposure(") < hdr.index("rt_tracer_exposure_device(") \
        < hdr.index("rt_tracer_intersect_all(")
    assert hdr.index("single-function device harnesses") < hdr.index("rt_dbg_exposure_rays(")
    assert "#define RT_MAX_DIRS 64u" in hdr and api.RT_MAX_DIRS == 64
    assert "#define RT_EXPOSURE_LOCAL 0u" in hdr and "#define RT_EXPOSURE_WORLD 1u" in hdr
    assert (api.EXPOSURE_LOCAL, api.EXPOSURE_WORLD) == (0, 1)
    pts = np.zeros((4, 8), np.float32)
    dirs = np.zeros((4, 4), np.float32)
    masks = np.zeros(4, np.uint64)
    p, d, m = pts.ctypes.data, dirs.ctypes.data, masks.ctypes.data
    assert L.rt_tracer_exposure(None, p, 4, d, 4, 0, m) == 1
    assert L.rt_tracer_exposure_device(None, p, 4, d, 4, 0, m, None) == 1
    assert L.rt_tracer_exposure(None, None, 0, None, 1, 0, None) == 1


def test_exposure_rays_argument_table():
    from raytracertest_amd import api
    L = api.load_library()
    pts = np.zeros((3, 8), np.float32)
    pts[:, 3:6] = [0, 0, 1]
    pts[:, 6:] = [0.25, 4.0]
    dirs = np.zeros((64, 4), np.float32)
    dirs[:, :3] = [1, 2, 3]
    out = np.full((3, 64, 8), 9.0, np.float32)
    p, d, o = pts.ctypes.data, dirs.ctypes.data, out.ctypes.data
    for n_dirs in (0, 65, 1 << 20):
        assert L.rt_dbg_exposure_rays(None, p, 3, d, n_dirs, 0, o) == 1 and "n_dirs" in L.rt_last_error().decode()
    for flags in (2, 3, 4, 0x80000000):
        assert L.rt_dbg_exposure_rays(None, p, 3, d, 64, flags, o) == 1 and "flags" in L.rt_last_error().decode()
    for args in ((None, 3, d, o), (p, 3, None, o), (p, 3, d, None)):
        assert L.rt_dbg_exposure_rays(None, args[0], args[1], args[2], 64, 0, args[3]) == 1
    assert (out == 9.0).all()                                            # nothing was written by the rejected calls
    assert L.rt_dbg_exposure_rays(None, None, 0, None, 1, 0, None) == 0  # n = 0 is a no-op
    assert L.rt_dbg_exposure_rays(None, None, 0, None, 0, 0, None) == 1  # ... but n_dirs is checked whatever n is
    assert L.rt_dbg_exposure_rays(None, p, 3, d, 2, 0, o) == 0           # writes n * n_dirs segments, no more
    flat = out.reshape(-1, 8)
    assert (flat[6:] == 9.0).all()
    assert np.array_equal(flat[:6], np.float32([[0, 0, 0, 1, 2, 3, 0.25, 4.0]] * 6))    # normal +z: the frame is the identity
    assert L.rt_dbg_exposure_rays(None, p, 3, d, 64, 1, o) == 0
    assert np.array_equal(out[:, :, 3:6], np.broadcast_to(np.float32([1, 2, 3]), (3, 64, 3)))


def test_python_class_has_the_methods_and_checks_its_arguments():
    from raytracertest_amd import api
    for m in ("Exposure", "AmbientOcclusion", "DebugExposureRays"):
        assert callable(getattr(api.RayTracer, m))
    assert callable(api.hemisphere_directions) and callable(api.exposure_rays)
    pts = np.zeros((2, 8), np.float32)
    for bad_dirs in (np.zeros((0, 3), np.float32), np.zeros((65, 3), np.float32), np.zeros((4, 2), np.float32), np.zeros(3, np.float32)):
        try:
            api.exposure_rays(pts, bad_dirs)
        except ValueError:
            continue
        raise AssertionError(bad_dirs.shape)
    for bad_pts in (np.zeros((2, 7), np.float32), np.float32(1.0)):
        try:
            api.exposure_rays(bad_pts, np.zeros((4, 3), np.float32))
        except ValueError:
            continue
        raise AssertionError(bad_pts.shape)
    six = api._exposure_points_array("Exposure", np.zeros((2, 6), np.float32), 1e-3, 2.0)   # (n, 6): the scalar bounds are filled in
    assert six.shape == (2, 8) and (six[:, 6] == np.float32(1e-3)).all() and (six[:, 7] == 2.0).all()
    six = api._exposure_points_array("Exposure", np.zeros((2, 6), np.float32), None, None)
    assert (six[:, 6] == 0.0).all() and np.isposinf(six[:, 7]).all()


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'typedef char max_dirs_is_64[RT_MAX_DIRS == 64u ? 1 : -1];\n'
                   'int main(void) { float p[8] = {0}, d[4] = {0}, s[8]; uint64_t m = 0;\n'
                   '  return rt_tracer_exposure(NULL, p, 1, d, 1, RT_EXPOSURE_LOCAL, &m) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_exposure_device(NULL, p, 1, d, 1, RT_EXPOSURE_WORLD, &m, NULL) == RT_ERR_INVALID &&\n'
                   '         rt_dbg_exposure_rays(NULL, p, 1, d, 0, 0, s) == RT_ERR_INVALID &&\n'
                   '         RT_EXPOSURE_LOCAL == 0 && RT_EXPOSURE_WORLD == 1 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_exposure_and_rejects_vectors_that_do_not_fit(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  const std::vector<float> dirs = rt::RayTracer::HemisphereDirections(64);\n'
                   '  if (dirs.size() != 256 || dirs[3] != 0.0f || !(dirs[2] > 0.99f) || !(dirs[254] > 0.0f)) return 1;\n'
                   '  std::vector<float> pts(16, 0.0f), seven(7, 0.0f); std::vector<uint64_t> masks(3, 5u);\n'
                   '  pts[5] = pts[13] = 1.0f; pts[7] = pts[15] = 2.0f;\n'
                   '  if (r.Exposure(seven, dirs, masks) || masks.size() != 3 || masks[0] != 5u) return 2;\n'
                   '  if (r.Exposure(pts, std::vector<float>(), masks) || r.Exposure(pts, std::vector<float>(5, 0.0f), masks)) return 3;\n'
                   '  if (r.Exposure(pts, rt::RayTracer::HemisphereDirections(65), masks) || masks.size() != 3) return 4;\n'
                   '  if (!r.Exposure(seven, dirs).empty()) return 5;\n'
                   '  const bool ok = r.Exposure(pts, dirs, masks);\n'
                   '  if (ok != r.Valid()) return 6;\n'
                   '  if (ok && (masks.size() != 2 || masks[0] != ~0ull || masks[1] != ~0ull)) return 7;       // no scene: all open\n'
                   '  if (ok && r.Exposure(pts, rt::RayTracer::HemisphereDirections(3), true) != std::vector<uint64_t>(2, 7u)) return 8;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
