"""CPU checks of the hexahedron-shaped region query's boundary (rt_tracer_overlap_hexahedra / _device): declared, exported,
argument checks that need no device, the struct-free signature and the rule in the header, the Python helpers that build the
corners, the C++ class and both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
NEW = ("rt_tracer_overlap_hexahedra", "rt_tracer_overlap_hexahedra_device")


def test_symbols_are_declared_exported_in_header_order_and_reject_null_handles_and_arrays():
    from raytracertest_amd import api
    L = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in NEW:
        assert name in api.ABI_SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert (hdr.index("rt_tracer_overlap_triangles_device(") < hdr.index("rt_tracer_overlap_hexahedra(")
            < hdr.index("rt_tracer_overlap_hexahedra_device(") < hdr.index("---- one frame sharded"))
    s = api.ABI_SYMBOLS
    assert s.index("rt_tracer_overlap_triangles_device") < s.index(NEW[0]) < s.index(NEW[1]) < s.index("rt_tracer_sphere_cast") and len(set(s)) == len(s)
    hexa = np.zeros((4, 32), np.float32)
    after = np.full(4, -1, np.int32)
    prims = np.full((4, 4), 77, np.int32)
    counts = np.full(4, 99, np.uint32)
    a = (hexa.ctypes.data, after.ctypes.data, 4, 4, prims.ctypes.data, counts.ctypes.data)
    assert L.rt_tracer_overlap_hexahedra(None, *a) == 1                  # RT_ERR_INVALID
    assert L.rt_tracer_overlap_hexahedra_device(None, *a, None) == 1
    assert L.rt_tracer_overlap_hexahedra(None, None, None, 0, 4, None, None) == 1
    assert L.rt_tracer_overlap_hexahedra(None, hexa.ctypes.data, None, 4, 17, prims.ctypes.data, counts.ctypes.data) == 1
    assert L.rt_tracer_overlap_hexahedra_device(None, None, None, 4, 0, None, None, None) == 1
    assert (prims == 77).all() and (counts == 99).all()                  # the outputs are untouched


def test_the_signature_is_struct_free_and_the_rule_is_written_out():
    hdr = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    sec = hdr[hdr.index("rt_tracer_overlap_triangles_device("):hdr.index("---- one frame sharded")]
    assert ("int  rt_tracer_overlap_hexahedra(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits, int32_t* prims,\n"
            "                                 uint32_t* counts);") in sec
    assert ("int  rt_tracer_overlap_hexahedra_device(rt_tracer* t, const float* hexa, const int32_t* after, size_t n, uint32_t max_hits,\n"
            "                                        int32_t* prims, uint32_t* counts, void* stream);") in sec
    assert "rt_hit" not in sec and "typedef" not in sec
    for text in ("n x 32 floats", "eight 16-byte loads", "bit 0 of k", "1. Box step", "All 24 corner coordinates are finite",
                 "accepts NOTHING, spheres included", "2. Move by -C0", "3. Forty-three axes", "f = {e1, c - b, a - c}",
                 "(h_d - h_a) x (h_c - h_b)", "(0,2,4,6), (1,3,5,7), (0,1,4,5), (2,3,6,7), (0,1,2,3), (4,5,6,7)",
                 "(0,1), (2,3), (4,5), (6,7),", "(0,2), (1,3), (4,6), (5,7), (0,4), (1,5), (2,6), (3,7)", "0, x.h_1 .. x.h_7",
                 "a NaN projection never separates", "may be accepted though the two are apart", "d2min <= r*r && r*r <= d2max",
                 "every centre counts as inside", "NO inflation", "restarting the list and the count",
                 "no rho, no slack and no conditioning clause", "0 .. RT_MAX_HITS", "hexa must be 16-byte aligned"):
        assert text in sec, text


def test_python_class_has_the_methods_and_the_corner_helpers_are_float32_as_stated():
    from raytracertest_amd import api
    R = api.RayTracer
    for m in ("OverlapHexahedra", "_overlap_hexahedra_tensor", "OverlapHexahedraAll", "box_corners", "oriented_box_corners",
              "frustum_corners", "PixelFrustum", "SelectRect"):
        assert callable(getattr(R, m))
    c = np.arange(48, dtype=np.float32).reshape(2, 8, 3)
    want = np.zeros((2, 8, 4), np.float32)
    want[:, :, :3] = c
    for form in (c, want, want.reshape(2, 32), c[0]):
        got = R._hexahedra_array("OverlapHexahedra", form)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want.reshape(2, 32)[:got.shape[0]])
    for bad in (np.zeros((3, 5)), 1.0, np.zeros((3, 24)), np.zeros((2, 3, 4)), np.zeros((2, 12))):
        with pytest.raises(ValueError, match="OverlapHexahedra"):
            R._hexahedra_array("OverlapHexahedra", bad)
    # box_corners: no arithmetic, bit 0 / 1 / 2 of k picks hi's x / y / z
    b = R.box_corners([1, 2, 3], [4, 5, 6])
    assert b.shape == (1, 8, 3) and b.dtype == np.float32
    assert b[0].tolist() == [[1, 2, 3], [4, 2, 3], [1, 5, 3], [4, 5, 3], [1, 2, 6], [4, 2, 6], [1, 5, 6], [4, 5, 6]]
    # oriented_box_corners: ((centre +- a0) +- a1) +- a2 in float32
    rng = np.random.default_rng(1)
    centre, axes = rng.normal(size=(5, 3)).astype(np.float32), rng.normal(size=(5, 3, 3)).astype(np.float32)
    o = R.oriented_box_corners(centre, axes)
    assert o.shape == (5, 8, 3) and o.dtype == np.float32
    for k in range(8):
        s = [np.float32(1 if (k >> j) & 1 else -1) for j in range(3)]
        assert np.array_equal(o[:, k], ((centre + s[0] * axes[:, 0]) + s[1] * axes[:, 1]) + s[2] * axes[:, 2])
    assert np.array_equal(R.oriented_box_corners([0, 0, 0], np.eye(3))[0], R.box_corners([-1, -1, -1], [1, 1, 1])[0])
    # frustum_corners: o + near*d and o + far*d, each operation rounded to float32
    rays = rng.normal(size=(3, 4, 6)).astype(np.float32)
    f = R.frustum_corners(rays, 0.25, np.float32([2.0, 3.0, 0.7]))
    assert f.shape == (3, 8, 3) and f.dtype == np.float32
    assert np.array_equal(f[:, :4], rays[:, :, :3] + np.float32(0.25) * rays[:, :, 3:])
    assert np.array_equal(f[:, 4:], rays[:, :, :3] + np.float32([2.0, 3.0, 0.7])[:, None, None] * rays[:, :, 3:])
    assert np.array_equal(R.frustum_corners(rays[0], 0.0, 1.0)[0, :4], rays[0, :, :3])      # near = 0: the origins bit for bit
    per_ray = np.float32([[0.5, 1.0, 1.5, 2.0]])
    assert np.array_equal(R.frustum_corners(rays[0], 0.25, per_ray)[0, 4:], rays[0, :, :3] + per_ray[0][:, None] * rays[0, :, 3:])


def test_cap_parameters_enclose_everything_between_near_and_far():
    """PixelFrustum's caps: flat, perpendicular to the sum of the four unit directions, and beyond every point at parameter near
    resp. far of every unit direction between the four -- checked in float64 on a wide, off-centre rectangle of directions."""
    from raytracertest_amd.api import RayTracer as R
    tx, ty = (-0.9, 0.5), (-0.7, -0.1)
    d = np.array([[tx[i], ty[j], -1.0] for j in (0, 1) for i in (0, 1)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.c_[np.full((4, 3), 0.25), d].astype(np.float32)
    near_k, far_k = R.cap_parameters(rays, 0.5, 2.0)
    assert near_k.shape == (1, 4) and far_k.dtype == np.float32 and (near_k <= 0.5).all() and (far_k >= 2.0).all()
    C = R.frustum_corners(rays, near_k, far_k)[0].astype(np.float64) - 0.25
    w = rays[:, 3:].astype(np.float64).sum(axis=0)
    depth = C @ w
    assert np.ptp(depth[:4]) < 1e-5 and np.ptp(depth[4:]) < 1e-5            # both caps are flat
    u, v = np.meshgrid(np.linspace(0, 1, 101), np.linspace(0, 1, 101))
    inner = np.stack([tx[0] + u * (tx[1] - tx[0]), ty[0] + v * (ty[1] - ty[0]), -np.ones_like(u)], axis=-1).reshape(-1, 3)
    inner /= np.linalg.norm(inner, axis=1, keepdims=True)
    assert (2.0 * inner @ w <= depth[4:].max() + 1e-5).all() and (0.5 * inner @ w >= depth[:4].min() - 1e-5).all()
    assert (2.0 * inner @ w).max() > depth[4:].max() - 1e-3                  # and no farther out than that needs


def test_header_compiles_as_c99_with_the_new_entries(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include "rt_mi355x.h"\n'
                   'int main(void) { float h[32] = {0}; int32_t prims[RT_MAX_HITS]; int32_t after = RT_PRIM_NONE; uint32_t c;\n'
                   '  return rt_tracer_overlap_hexahedra(NULL, h, &after, 1, RT_MAX_HITS, prims, &c) == RT_ERR_INVALID &&\n'
                   '         rt_tracer_overlap_hexahedra_device(NULL, h, NULL, 1, 0, NULL, &c, NULL) == RT_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "a.o")], check=True)


def test_cpp_class_has_overlap_hexahedra_and_rejects_bad_vectors_and_counts(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include "RayTracer/RayTracer.h"\n'
                   'int main() {\n'
                   '  rt::RayTracer r(math::uvec2(8, 8), math::vec3(0, 0, 0), math::vec2(0, 0), 70.0f, 10.0f, 4.0f);\n'
                   '  std::vector<float> hexa(64, 0.0f), odd(24, 0.0f); std::vector<int32_t> prims(3), after(3); std::vector<uint32_t> counts(5);\n'
                   '  if (r.OverlapHexahedra(odd, 4, prims, counts) || prims.size() != 3 || counts.size() != 5) return 1;\n'
                   '  if (r.OverlapHexahedra(hexa, RT_MAX_HITS + 1, prims, counts) || prims.size() != 3) return 2;\n'
                   '  if (r.OverlapHexahedra(hexa, 4, prims, counts, after) || prims.size() != 3) return 3;       // a cursor of another length\n'
                   '  if (!r.OverlapHexahedra(odd, 4).empty() || !r.OverlapHexahedra(hexa, 17).empty()) return 4;\n'
                   '  const bool ok = r.OverlapHexahedra(hexa, 3, prims, counts);\n'
                   '  if (ok != r.Valid()) return 5;\n'
                   '  if (ok && (prims.size() != 6 || counts.size() != 2 || counts[0] != 0 || prims[0] != RT_PRIM_NONE ||\n'
                   '             r.OverlapHexahedra(hexa).size() != 2 || !r.OverlapHexahedra(hexa, 0, prims, counts) || !prims.empty())) return 6;\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "a")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_both_command_lines_know_the_hexahedron_query_and_the_selection(tmp_path):
    exe = str(tmp_path / "rt_cli")                                   # (from the source of this tree, whatever lib/ holds)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "rt_cli.cpp"), "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR,
                    "-pthread", "-o", exe], check=True)
    form, sel = "X0,Y0,Z0,...,X7,Y7,Z7[,K]", "X0,Y0,X1,Y1,FAR[,NEAR]"
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--overlap-hexa " + form in out.stdout and "--select " + sel in out.stdout
    c24 = ",".join(str(v) for v in range(24))
    for bad in ("3", "1,2,3,4,5,6", c24[:-3], c24 + ",", c24 + ",x", c24 + ",-1", c24 + ",4,5"):
        out = subprocess.run([exe, "--overlap-hexa", bad], capture_output=True, text=True)
        assert out.returncode == 2 and form in out.stderr, bad
    for bad in ("3", "1,2,3,4", "1,2,3,4,inf", "1,2,3,4,5,nan", "-1,2,3,4,5", "1,2,3,4,5,6,7", "1,2,3,4,x"):
        out = subprocess.run([exe, "--select", bad], capture_output=True, text=True)
        assert out.returncode == 2 and sel in out.stderr, bad
    py = subprocess.run([sys.executable, "-m", "raytracertest_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert py.returncode == 0 and form in py.stdout and sel in py.stdout
    from raytracertest_amd.cli import build_parser
    a = build_parser().parse_args(["--overlap-hexa", c24])
    assert a.overlap_hexa == tuple(float(v) for v in range(24)) + (8,) and a.select is None and a.overlap_tri is None
    assert build_parser().parse_args(["--overlap-hexa=" + c24 + ",0"]).overlap_hexa[24] == 0
    assert build_parser().parse_args(["--select", "1,2,30,20,9.5"]).select == (1, 2, 30, 20, 9.5, 0.0)
    assert build_parser().parse_args(["--select", "1,2,30,20,9.5,0.25"]).select == (1, 2, 30, 20, 9.5, 0.25)
    for opt, bad in (("--overlap-hexa", "1,2,3"), ("--overlap-hexa", c24 + ",-1"), ("--overlap-hexa", c24 + ",x"),
                     ("--select", "1,2,3,4"), ("--select", "1,2,3,4,inf"), ("--select", "-1,2,3,4,5"), ("--select", "1,2,3,4,5,6,7")):
        with pytest.raises(SystemExit):
            build_parser().parse_args([opt, bad])
