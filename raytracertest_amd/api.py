"""Host-side mirror of rt::RayTracer (RayTracer/RayTracer.h:14-41) over the C ABI
(include/rt_mi355x.h).  Same method names, argument order, units and error behaviour as
the reference class, so that the parity tests read like a caller of the reference
(OpenGLView/MainFrame.cpp:45,219-256).

There is NO fallback: if librt_mi355x.so is missing or no HIP device is usable this
module raises.  PyTorch is not involved here, except that RayTracer.Intersect also takes a torch tensor on the
tracer's device (torch is imported only then).
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_MI355X_LIB selects another build of the same library (kernel A/B experiments only)
_LIB_PATH = os.environ.get("RT_MI355X_LIB") or os.path.join(_HERE, "lib", "librt_mi355x.so")

MATH_FMA, MATH_STRICT = 0, 1
FLAG_NO_FILTER = 1
FLAG_NO_BINNING = 2
FLAG_NEAREST_HIT = 4
FLAG_SMOOTH_NORMALS = 8
FLAG_NO_MACRO_BINS = 16
FLAG_NO_SUPER_BINS = 64
FLAG_NO_SURE_HIT = 32
BUF_RENDER, BUF_COUNTS, BUF_IMAGE, BUF_RNG, BUF_FRAME = 0, 1, 2, 3, 4
GROUP_ID_BYTES = 128
TRANSPORT_RCCL, TRANSPORT_PEER = 0, 1

# every symbol include/rt_mi355x.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "rt_tracer_create", "rt_tracer_create_ex", "rt_tracer_destroy", "rt_tracer_trace",
    "rt_tracer_stop", "rt_tracer_resize", "rt_tracer_set_camera_parameters",
    "rt_tracer_rotate_camera", "rt_tracer_upload_scene", "rt_tracer_set_update_callback",
    "rt_tracer_set_finished_callback", "rt_tracer_wait", "rt_tracer_set_seed",
    "rt_tracer_upload_spheres", "rt_tracer_trace_enqueue", "rt_tracer_trace_enqueue_n", "rt_tracer_sync", "rt_tracer_trace_stats", "rt_tracer_launch", "rt_tracer_launch_iterations", "rt_tracer_fused_iterations", "rt_tracer_set_image_mirror", "rt_tracer_set_list_reuse", "rt_tracer_stream_b", "rt_tracer_upload_scene_edges", "rt_pack_normal",
    "rt_unpack_normal",
    "rt_tracer_kernel_time", "rt_tracer_launch_time", "rt_tracer_read_buffer", "rt_tracer_copy_buffer_to_device", "rt_tracer_copy_buffer_to_device_async",
    "rt_tracer_stream",
    "rt_tracer_device_pointer", "rt_tracer_buffer_bytes", "rt_tracer_info",
    "rt_tracer_last_error", "rt_last_error", "rt_device_count", "rt_version",
    "rt_dbg_hit_triangle", "rt_dbg_sincos", "rt_dbg_valu_peak", "rt_dbg_check_midrange", "rt_dbg_trace_occupancy", "rt_dbg_uniform", "rt_dbg_get_ray",
    "rt_dbg_rng_init_host", "rt_dbg_rng_advance_host", "rt_dbg_rng_advance_host_n", "rt_dbg_owed_state", "rt_dbg_enqueue_calls", "rt_dbg_list_builds",
    "rt_tracer_create_multi", "rt_group_unique_id", "rt_tracer_join_group", "rt_tracer_leave_group",
    "rt_tracer_gather_time", "rt_tracer_band_count", "rt_tracer_band_info",
    "rt_tracer_join_group_bands", "rt_balance_rows", "rt_tracer_rebalance", "rt_tracer_set_band", "rt_dbg_read_tile_lists", "rt_dbg_wave_list_counts", "rt_dbg_focal_boxes", "rt_dbg_classify",
    "rt_tracer_gather_only", "rt_tracer_group_info",
    "rt_tracer_intersect", "rt_tracer_intersect_device", "rt_tracer_pick", "rt_tracer_focus_at",
    "rt_tracer_occluded", "rt_tracer_occluded_device",
    "rt_tracer_exposure", "rt_tracer_exposure_device", "rt_dbg_exposure_rays",
    "rt_tracer_intersect_all", "rt_tracer_intersect_all_device",
    "rt_tracer_closest_point", "rt_tracer_closest_point_device",
    "rt_tracer_closest_all", "rt_tracer_closest_all_device",
    "rt_tracer_signed_distance", "rt_tracer_signed_distance_device",
    "rt_tracer_closest_sides", "rt_tracer_closest_sides_device", "rt_dbg_feature_normals",
    "rt_tracer_overlap", "rt_tracer_overlap_device",
    "rt_tracer_overlap_triangles", "rt_tracer_overlap_triangles_device",
    "rt_tracer_overlap_hexahedra", "rt_tracer_overlap_hexahedra_device",
    "rt_tracer_section", "rt_tracer_section_device", "rt_tracer_section_segments", "rt_tracer_section_segments_device",
    "rt_tracer_sphere_cast", "rt_tracer_sphere_cast_device",
    "rt_tracer_triangle_distance", "rt_tracer_triangle_distance_device",
    "rt_tracer_set_query_accel", "rt_tracer_query_accel_info", "rt_dbg_bvh_build", "rt_dbg_query_accel_slack",
    "rt_tracer_set_query_accel_update", "rt_tracer_query_accel_rebuild", "rt_tracer_query_accel_update_info",
    "rt_dbg_bvh_refit", "rt_dbg_query_tree_read", "rt_dbg_bvh_tree_cost", "rt_dbg_query_stack_cap",
]


class RtError(RuntimeError):
    pass


PRIM_NONE = -1
RT_MAX_HITS = 16         # rt_tracer_intersect_all: the longest row
RT_MAX_DIRS = 64         # rt_tracer_exposure: the longest direction table (one lane per direction)
RT_SWEEP_SLACK = np.float32(2.0 ** -11)   # rt_tracer_sphere_cast: a contact is within RT_SWEEP_SLACK * (max|c| + r) of touching
EXPOSURE_LOCAL, EXPOSURE_WORLD = 0, 1
QUERY_SCAN, QUERY_BVH = 0, 1
ACCEL_REBUILD, ACCEL_REFIT = 0, 1        # rt_tracer_set_query_accel_update: what an upload does to the tree of QUERY_BVH
# the arrays of rt_dbg_bvh_build (include/rt_mi355x.h): a 4-wide node and a leaf record
BVH_NODE_DTYPE = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.uint32, 4), ("cmax", np.float32, 4)])
BVH_RECORD_DTYPE = np.dtype([("e2", np.float32, 3), ("e1", np.float32, 3), ("v0", np.float32, 3), ("index", np.uint32), ("pad", np.uint32, 2)])
BVH_EMPTY, BVH_LEAF = 0xFFFFFFFF, 0x80000000
_ACCEL_KEYS = ("mode", "valid", "nodes", "leaves", "depth", "always_tested", "build_us", "device_bytes")


def bvh_build(rows, edges=False):
    """rt_dbg_bvh_build: the query BVH of upload rows (3N, 4), built on the host (no device needed) -> (nodes
    BVH_NODE_DTYPE, records BVH_RECORD_DTYPE, info dict; info["depth_bound"] is what the traversal stack is sized from)."""
    L = load_library()
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, 4)
    info = (C.c_uint64 * 8)()
    if L.rt_dbg_bvh_build(r.ctypes.data, r.shape[0], int(bool(edges)), None, 0, None, 0, info) != 0:
        raise RtError("rt_dbg_bvh_build: " + L.rt_last_error().decode())
    nodes = np.zeros(int(info[2]), BVH_NODE_DTYPE)
    recs = np.zeros(r.shape[0] // 3, BVH_RECORD_DTYPE)
    if L.rt_dbg_bvh_build(r.ctypes.data, r.shape[0], int(bool(edges)), nodes.ctypes.data, max(nodes.nbytes, 1), recs.ctypes.data,
                          max(recs.nbytes, 1), info) != 0:
        raise RtError("rt_dbg_bvh_build: " + L.rt_last_error().decode())
    return nodes, recs, _tree_info(info)


def _tree_info(info):
    d = dict(zip(_ACCEL_KEYS, (int(x) for x in info)))
    d["depth_bound"] = d.pop("mode")
    return d


def bvh_refit(rows, nodes, recs, info, edges=False):
    """rt_dbg_bvh_refit: the tree (nodes, recs, info) of bvh_build -- or of an earlier refit -- refitted on the host to the
    upload rows (3N, 4) of as many triangles -> (nodes, records, info) as new arrays.  RtError when a triangle changed between
    finite and non-finite (the partition rule: such a scene has to be built)."""
    L = load_library()
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, 4)
    nodes = np.ascontiguousarray(nodes, BVH_NODE_DTYPE).copy()
    recs = np.ascontiguousarray(recs, BVH_RECORD_DTYPE).copy()
    raw = (C.c_uint64 * 8)(info["depth_bound"], 1, *(int(info[k]) for k in _ACCEL_KEYS[2:]))
    rc = L.rt_dbg_bvh_refit(r.ctypes.data, r.shape[0], int(bool(edges)), nodes.ctypes.data, nodes.nbytes, recs.ctypes.data, recs.nbytes, raw)
    if rc != 0:
        raise RtError("rt_dbg_bvh_refit: %s (code %d)" % (L.rt_last_error().decode(), rc))
    return nodes, recs, dict(info)


def tree_cost(nodes):
    """rt_dbg_bvh_tree_cost (rtb::tree_cost on the host): the half areas of all present children's boxes over the half area of
    the union of the root's child boxes, in double; 0 without nodes or without such an area."""
    L = load_library()
    nodes = np.ascontiguousarray(nodes, BVH_NODE_DTYPE)
    return float(L.rt_dbg_bvh_tree_cost(nodes.ctypes.data, nodes.nbytes)) if nodes.shape[0] else 0.0
# rt_hit: one ray query's answer (include/rt_mi355x.h)
HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("prim", np.int32)])
# rt_side: the side half of a signed point query's answer
SIDE_DTYPE = np.dtype([("s", np.float32), ("feature", np.int32)])
FEATURE_NONE, FEATURE_FACE, FEATURE_SPHERE = -1, 0, 7
# rt_cut: where a plane cuts one primitive (rt_tracer_section_segments)
CUT_DTYPE = np.dtype([("p0", np.float32, 3), ("kind", np.int32), ("p1", np.float32, 3), ("features", np.int32)])
CUT_NONE, CUT_SEGMENT, CUT_TOUCH, CUT_COPLANAR, CUT_CIRCLE = 0, 1, 2, 3, 4
# rt_witness: the query-side half of a triangle distance query's answer
WITNESS_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("where", np.int32)])
_FEATURE_KEYS = ("triangles", "vertices", "edges", "contributing", "build_us", "bytes")


def feature_normals(rows, edges=False, return_info=False):
    """rt_dbg_feature_normals: the signed queries' feature table of upload rows (3N, 4), built on the host (no device needed)
    -> (N, 7, 4) float32: per triangle the unit pseudonormals of the face, the vertices A, B, C and the edges AB, AC, BC
    (.w = 0).  return_info: also the dict {triangles, vertices, edges, contributing, build_us, bytes}."""
    L = load_library()
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, 4)
    info = (C.c_uint64 * 8)()
    out = np.zeros((r.shape[0] // 3, 7, 4), np.float32)
    if L.rt_dbg_feature_normals(r.ctypes.data, r.shape[0], int(bool(edges)), out.ctypes.data, max(out.nbytes, 1), info) != 0:
        raise RtError("rt_dbg_feature_normals: " + L.rt_last_error().decode())
    return (out, dict(zip(_FEATURE_KEYS, (int(x) for x in info)))) if return_info else out


def _dirs_array(who, directions):
    """-> contiguous (k, 4) float32 {x, y, z, 0}, 1 <= k <= RT_MAX_DIRS, of (k, 3) or (k, 4) directions."""
    d = np.asarray(directions, np.float32)
    if d.ndim != 2 or d.shape[1] not in (3, 4):
        raise ValueError("%s: expected (k, 3) or (k, 4) float32 directions, got shape %s" % (who, d.shape))
    if not 1 <= d.shape[0] <= RT_MAX_DIRS:
        raise ValueError("%s: %d directions (1 to %d)" % (who, d.shape[0], RT_MAX_DIRS))
    out = np.zeros((d.shape[0], 4), np.float32)
    out[:, :d.shape[1]] = d
    return out


def _exposure_points_array(who, points, tmin, tmax):
    """-> contiguous (n, 8) float32 {origin, normal, tmin, tmax}: (n, 6) points get the scalar tmin / tmax in columns 6, 7."""
    p = np.asarray(points, np.float32)
    if p.ndim == 0 or p.shape[-1] not in (6, 8):
        raise ValueError("%s: expected (n, 8) or (n, 6) float32 points, got shape %s" % (who, p.shape))
    if p.shape[-1] == 8:
        if tmin is not None or tmax is not None:
            raise ValueError("%s: (n, 8) points carry their own tmin and tmax" % who)
        return RayTracer._segs_array(who, p)
    q = np.empty(p.shape[:-1] + (8,), np.float32)
    q[..., :6], q[..., 6], q[..., 7] = p, np.float32(0.0 if tmin is None else tmin), np.float32(np.inf if tmax is None else tmax)
    return np.ascontiguousarray(q).reshape(-1, 8)


def hemisphere_directions(samples):
    """A cosine-weighted Fibonacci set on the hemisphere z > 0, for Exposure's local frame: (samples, 3) float32 unit
    vectors, sample k at r^2 = (k + 1/2) / samples, phi = (k + 1/2) * pi * (3 - sqrt(5)), (r cos phi, r sin phi, sqrt(1 - r^2)),
    computed in float64 and rounded to fp32 once.  Equal weights estimate a cosine-weighted integral."""
    n = int(samples)
    if n != samples or n < 1:
        raise ValueError("hemisphere_directions: samples = %r" % (samples,))
    k = np.arange(n, dtype=np.float64) + 0.5
    r2 = k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(r2)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r2)], axis=1).astype(np.float32)


def exposure_rays(points, directions, world=False):
    """rt_dbg_exposure_rays without a tracer: the (n, k, 8) float32 segments {origin, d_ij, tmin, tmax} Exposure traces for
    (n, 8) points and (k, 3 | 4) directions, from the function its kernels call, evaluated on the host (no device needed)."""
    L = load_library()
    p = _exposure_points_array("exposure_rays", points, None, None)
    d = _dirs_array("exposure_rays", directions)
    out = np.zeros((p.shape[0], d.shape[0], 8), np.float32)
    if L.rt_dbg_exposure_rays(None, p.ctypes.data, p.shape[0], d.ctypes.data, d.shape[0], int(bool(world)), out.ctypes.data) != 0:
        raise RtError("rt_dbg_exposure_rays: " + L.rt_last_error().decode())
    return out


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("full_height", C.c_uint32),
                ("row_begin", C.c_uint32), ("use_time_seed", C.c_uint32), ("math_mode", C.c_uint32),
                ("seed", C.c_uint64), ("flags", C.c_uint32), ("samples_in_flight", C.c_uint32),
                ("lds_chunk", C.c_uint32), ("bin_list", C.c_uint32), ("transport", C.c_uint32)]


CALLBACK = C.CFUNCTYPE(None, C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p)

_lib = None
_lib_lock = threading.Lock()


def library_path():
    return _LIB_PATH


def _share_hip_runtime_with_torch():
    """One process must not hold two HIP runtimes: PyTorch wheels bundle their own
    libamdhip64.so (SONAME libamdhip64.so.7, the same as /opt/rocm's), and whichever copy
    initialises second finds no device.  The multi-GPU driver (dist.py) needs torch.distributed
    (RCCL) next to this library, so when a PyTorch install is present its libamdhip64 is mapped
    first -- WITHOUT importing torch -- and librt_mi355x.so's NEEDED libamdhip64.so.7 binds to
    that same object; a later `import torch` reuses it too.  RT_MI355X_HIP_RUNTIME=system
    keeps /opt/rocm's runtime (then do not use torch.cuda in the same process)."""
    if os.environ.get("RT_MI355X_HIP_RUNTIME", "") == "system":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return None
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return cand
    except (ImportError, OSError, ValueError):
        pass
    return None


HIP_RUNTIME = None      # path of the HIP runtime shared with PyTorch, or None for /opt/rocm's


def load_library():
    """dlopen librt_mi355x.so and declare the ABI.  Raises if the extension is missing."""
    global _lib, HIP_RUNTIME
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise RtError("HIP extension not built: %s is missing (run `python -m raytracertest_amd.build` "
                          "or __graft_entry__.build()); there is no CPU fallback" % _LIB_PATH)
        HIP_RUNTIME = _share_hip_runtime_with_torch()
        L = C.CDLL(_LIB_PATH)
        vp, u32p, f32p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        L.rt_tracer_create.argtypes = [u32p, f32p, f32p, C.c_float, C.c_float, C.c_float, C.POINTER(vp)]
        L.rt_tracer_create_ex.argtypes = [u32p, f32p, f32p, C.c_float, C.c_float, C.c_float,
                                          C.POINTER(Options), C.POINTER(vp)]
        L.rt_tracer_destroy.argtypes = [vp]
        L.rt_tracer_destroy.restype = None
        L.rt_tracer_trace.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rt_tracer_stop.argtypes = [vp]
        L.rt_tracer_stop.restype = None
        L.rt_tracer_resize.argtypes = [vp, u32p]
        L.rt_tracer_set_camera_parameters.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        L.rt_tracer_set_camera_parameters.restype = None
        L.rt_tracer_rotate_camera.argtypes = [vp, f32p]
        L.rt_tracer_rotate_camera.restype = None
        L.rt_tracer_upload_scene.argtypes = [vp, vp, C.c_size_t]
        L.rt_tracer_upload_scene_edges.argtypes = [vp, vp, C.c_size_t]
        L.rt_pack_normal.argtypes = [f32p]
        L.rt_pack_normal.restype = C.c_float
        L.rt_unpack_normal.argtypes = [C.c_float, f32p]
        L.rt_unpack_normal.restype = None
        L.rt_tracer_set_update_callback.argtypes = [vp, CALLBACK, vp]
        L.rt_tracer_set_update_callback.restype = None
        L.rt_tracer_set_finished_callback.argtypes = [vp, CALLBACK, vp]
        L.rt_tracer_set_finished_callback.restype = None
        L.rt_tracer_wait.argtypes = [vp]
        L.rt_tracer_set_seed.argtypes = [vp, C.c_uint64]
        L.rt_tracer_upload_spheres.argtypes = [vp, vp, C.c_size_t]
        L.rt_tracer_trace_enqueue.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.rt_tracer_trace_enqueue_n.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rt_tracer_sync.argtypes = [vp]
        L.rt_tracer_launch.argtypes = [vp, C.c_uint32, C.c_int, C.c_int]
        L.rt_tracer_launch_iterations.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
        L.rt_tracer_fused_iterations.argtypes = [vp, C.c_uint32]
        L.rt_tracer_set_image_mirror.argtypes = [vp, vp]
        L.rt_tracer_set_list_reuse.argtypes = [vp, C.c_int]
        L.rt_tracer_trace_stats.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)]
        L.rt_tracer_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.rt_tracer_launch_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.rt_tracer_read_buffer.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.rt_tracer_copy_buffer_to_device.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.rt_tracer_copy_buffer_to_device_async.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.rt_tracer_stream.argtypes = [vp]
        L.rt_tracer_stream.restype = vp
        L.rt_tracer_stream_b.argtypes = [vp]
        L.rt_tracer_stream_b.restype = vp
        L.rt_tracer_device_pointer.argtypes = [vp, C.c_int]
        L.rt_tracer_device_pointer.restype = vp
        L.rt_tracer_buffer_bytes.argtypes = [vp, C.c_int]
        L.rt_tracer_buffer_bytes.restype = C.c_size_t
        L.rt_tracer_info.argtypes = [vp, u32p]
        L.rt_tracer_last_error.argtypes = [vp]
        L.rt_tracer_last_error.restype = C.c_char_p
        L.rt_last_error.restype = C.c_char_p
        L.rt_device_count.restype = C.c_int
        L.rt_version.restype = C.c_char_p
        L.rt_dbg_hit_triangle.argtypes = [C.c_int, C.c_uint32, C.c_uint32, f32p, f32p, C.c_int,
                                          C.POINTER(C.c_int32), f32p, f32p, f32p]
        L.rt_dbg_sincos.argtypes = [C.c_int, C.c_uint32, f32p, f32p, f32p]
        L.rt_dbg_uniform.argtypes = [C.c_int, C.c_uint32, C.c_uint32, u32p, f32p]
        L.rt_dbg_valu_peak.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.rt_dbg_trace_occupancy.argtypes = [C.c_int, C.c_int, C.c_uint32]
        L.rt_dbg_get_ray.argtypes = [vp, C.c_uint32, u32p, u32p, f32p]
        L.rt_dbg_rng_init_host.argtypes = [C.c_uint64, C.c_uint64, u32p]
        L.rt_dbg_rng_init_host.restype = None
        if hasattr(L, "rt_dbg_owed_state"):               # (an older build selected by RT_MI355X_LIB for a kernel A/B has none of the three)
            L.rt_dbg_rng_advance_host.argtypes = [u32p, C.c_uint32, C.c_int]
            L.rt_dbg_rng_advance_host.restype = None
            L.rt_dbg_rng_advance_host_n.argtypes = [u32p, C.c_uint32, C.c_uint32, C.c_int]
            L.rt_dbg_rng_advance_host_n.restype = None
            L.rt_dbg_owed_state.argtypes = [vp, C.POINTER(C.c_uint64)]
        if hasattr(L, "rt_dbg_enqueue_calls"):            # (nor has an older build this one)
            L.rt_dbg_enqueue_calls.argtypes = [vp, C.POINTER(C.c_uint64)]
        if hasattr(L, "rt_dbg_list_builds"):              # (nor this one)
            L.rt_dbg_list_builds.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_tracer_create_multi.argtypes = [u32p, f32p, f32p, C.c_float, C.c_float, C.c_float, C.POINTER(Options),
                                             C.POINTER(C.c_int32), C.c_uint32, C.POINTER(vp)]
        L.rt_group_unique_id.argtypes = [C.c_char_p]
        L.rt_tracer_join_group.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p]
        L.rt_tracer_leave_group.argtypes = [vp]
        L.rt_tracer_gather_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.rt_tracer_band_count.argtypes = [vp]
        L.rt_tracer_band_info.argtypes = [vp, C.c_uint32, u32p]
        L.rt_tracer_join_group_bands.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p, u32p]
        L.rt_balance_rows.argtypes = [C.c_uint32, u32p, C.POINTER(C.c_double), C.c_uint32, u32p]
        L.rt_tracer_rebalance.argtypes = [vp]
        L.rt_tracer_set_band.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.rt_dbg_read_tile_lists.argtypes = [vp, u32p, C.c_size_t, u32p]
        L.rt_dbg_wave_list_counts.argtypes = [vp, C.c_int, u32p, C.c_size_t, u32p, u32p]
        L.rt_dbg_focal_boxes.argtypes = [vp, C.c_float, f32p, C.c_size_t, f32p, C.c_size_t]
        L.rt_tracer_gather_only.argtypes = [vp]
        L.rt_tracer_group_info.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.rt_dbg_classify.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32, f32p, C.c_size_t]
        L.rt_tracer_intersect.argtypes = [vp, vp, C.c_size_t, vp]
        L.rt_tracer_intersect_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.rt_tracer_pick.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.rt_tracer_focus_at.argtypes = [vp, C.c_uint32, C.c_uint32, f32p]
        L.rt_tracer_occluded.argtypes = [vp, vp, C.c_size_t, vp]
        L.rt_tracer_occluded_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.rt_tracer_exposure.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp]
        L.rt_tracer_exposure_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp]
        L.rt_dbg_exposure_rays.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp]
        L.rt_tracer_intersect_all.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp]
        L.rt_tracer_intersect_all_device.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
        L.rt_tracer_closest_point.argtypes = [vp, vp, C.c_size_t, vp]
        L.rt_tracer_closest_point_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.rt_tracer_closest_all.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
        L.rt_tracer_closest_all_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
        L.rt_tracer_signed_distance.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.rt_tracer_signed_distance_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        L.rt_tracer_closest_sides.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]
        L.rt_tracer_closest_sides_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
        L.rt_tracer_overlap.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
        L.rt_tracer_overlap_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
        if hasattr(L, "rt_tracer_overlap_triangles"):     # (an older build selected by RT_MI355X_LIB for an A/B has no triangle regions)
            L.rt_tracer_overlap_triangles.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
            L.rt_tracer_overlap_triangles_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
        if hasattr(L, "rt_tracer_overlap_hexahedra"):     # (an older build selected by RT_MI355X_LIB for an A/B has no hexahedron regions)
            L.rt_tracer_overlap_hexahedra.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
            L.rt_tracer_overlap_hexahedra_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
        if hasattr(L, "rt_tracer_section"):               # (an older build selected by RT_MI355X_LIB for an A/B has no section queries)
            L.rt_tracer_section.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
            L.rt_tracer_section_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp]
            L.rt_tracer_section_segments.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]
            L.rt_tracer_section_segments_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp]
        if hasattr(L, "rt_tracer_sphere_cast"):           # (an older build selected by RT_MI355X_LIB for an A/B has no swept query)
            L.rt_tracer_sphere_cast.argtypes = [vp, vp, C.c_size_t, vp]
            L.rt_tracer_sphere_cast_device.argtypes = [vp, vp, C.c_size_t, vp, vp]
        if hasattr(L, "rt_tracer_triangle_distance"):     # (an older build selected by RT_MI355X_LIB for an A/B has no triangle distance)
            L.rt_tracer_triangle_distance.argtypes = [vp, vp, C.c_size_t, vp, vp]
            L.rt_tracer_triangle_distance_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        L.rt_dbg_feature_normals.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
        L.rt_tracer_set_query_accel.argtypes = [vp, C.c_uint32]
        L.rt_tracer_query_accel_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_dbg_query_accel_slack.argtypes = [vp, C.c_uint32]
        L.rt_dbg_query_stack_cap.argtypes = [vp, C.c_uint32]
        L.rt_dbg_bvh_build.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.rt_tracer_set_query_accel_update.argtypes = [vp, C.c_uint32]
        L.rt_tracer_query_accel_rebuild.argtypes = [vp]
        L.rt_tracer_query_accel_update_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_dbg_bvh_refit.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.rt_dbg_query_tree_read.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.rt_dbg_bvh_tree_cost.argtypes = [vp, C.c_size_t]
        L.rt_dbg_bvh_tree_cost.restype = C.c_double
        _lib = L
        return _lib


def device_count():
    return int(load_library().rt_device_count())


def balance_rows(row_begin, cost, granule=8):
    """Boundaries (len(cost) + 1 row indices) that equalise the bands' cost (rt_balance_rows)."""
    b = np.ascontiguousarray(row_begin, np.uint32)
    c = np.ascontiguousarray(cost, np.float64)
    out = np.zeros_like(b)
    rc = load_library().rt_balance_rows(c.size, _u32p(b), c.ctypes.data_as(C.POINTER(C.c_double)), granule, _u32p(out))
    if rc != 0:
        raise RtError("rt_balance_rows: invalid partition")
    return [int(x) for x in out]


def group_unique_id():
    """The id (bytes) rank 0 creates and the launcher's rendezvous hands to every rank for JoinGroup."""
    buf = C.create_string_buffer(GROUP_ID_BYTES)
    rc = load_library().rt_group_unique_id(buf)
    if rc != 0:
        raise RtError("rt_group_unique_id failed (%d): %s" % (rc, load_library().rt_last_error().decode()))
    return buf.raw


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class RayTracer:
    """rt::RayTracer.  Reference methods keep their names: Trace, Stop, Resize,
    SetCameraParameters, RotateCamera, UploadScene, SetUpdateCallback, SetFinishedCallback.
    Callbacks receive (image, size_bytes): image is a host numpy view (rows, W) of BGRA8
    uint32 valid during the call (the reference hands a device pointer: PBO interop is cut)."""

    def __init__(self, imageSize, cameraPosition=(0.0, 0.0, 0.0), cameraAngles=(0.0, 0.0), fov=70.0,
                 focalLength=10.0, aperture=4.0, *, seed=None, device=0, math_mode=MATH_FMA,
                 full_height=0, row_begin=0, no_filter=False, no_binning=False, nearest_hit=False, smooth_normals=False, no_macro_bins=False, no_super_bins=False, samples_in_flight=0,
                 lds_chunk=0, bin_list=0, devices=None, no_sure_hit=False, transport="rccl"):
        """devices: a list of HIP device ordinals, one per row band -> the frame is sharded over them inside
        this process (rt_tracer_create_multi; ordinals may repeat); None -> one tracer on `device`."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self._cbs = {}
        self._retired = []
        self._scene_rows, self._scene_edges, self._sphere_rows = None, False, None   # host copies, for ClosestPositions
        size = np.array(imageSize, np.uint32)
        opt = Options()
        opt.struct_size = C.sizeof(Options)
        opt.device = device
        opt.full_height, opt.row_begin = full_height, row_begin
        opt.use_time_seed = 1 if seed is None else 0          # Random.cu:45 when no seed is given
        opt.seed = 0 if seed is None else int(seed)
        opt.math_mode = math_mode
        opt.flags = ((FLAG_NO_FILTER if no_filter else 0) | (FLAG_NO_BINNING if no_binning else 0) |
                     (FLAG_NEAREST_HIT if nearest_hit else 0) | (FLAG_SMOOTH_NORMALS if smooth_normals else 0) | (FLAG_NO_MACRO_BINS if no_macro_bins else 0) | (FLAG_NO_SUPER_BINS if no_super_bins else 0) |
                     (FLAG_NO_SURE_HIT if no_sure_hit else 0))
        opt.samples_in_flight, opt.lds_chunk, opt.bin_list = samples_in_flight, lds_chunk, bin_list
        opt.transport = {"rccl": TRANSPORT_RCCL, "peer": TRANSPORT_PEER}[transport]
        if devices is not None:
            devs = np.ascontiguousarray(devices, np.int32)
            rc = self._lib.rt_tracer_create_multi(_u32p(size), _f32p(np.array(cameraPosition, np.float32)),
                                                  _f32p(np.array(cameraAngles, np.float32)), fov, focalLength, aperture,
                                                  C.byref(opt), devs.ctypes.data_as(C.POINTER(C.c_int32)), devs.size,
                                                  C.byref(self._h))
        else:
            rc = self._lib.rt_tracer_create_ex(_u32p(size), _f32p(np.array(cameraPosition, np.float32)),
                                               _f32p(np.array(cameraAngles, np.float32)), fov, focalLength,
                                               aperture, C.byref(opt), C.byref(self._h))
        if rc != 0 or not self._h:
            raise RtError("rt_tracer_create failed (%d): %s" % (rc, self._lib.rt_last_error().decode()))
        self.full_height = int(full_height) if full_height else int(size[1])
        self._band = bool(full_height) and devices is None
        self.width = int(size[0])
        self.rows = int(size[1])

    # ---- reference API -------------------------------------------------------------
    def Trace(self, iterationCount, samplesPerIteration, updateInterval):
        self._check(self._lib.rt_tracer_trace(self._h, iterationCount, samplesPerIteration, updateInterval))

    def Stop(self):
        self._lib.rt_tracer_stop(self._h)

    def Resize(self, size):
        s = np.array(size, np.uint32)
        self._check(self._lib.rt_tracer_resize(self._h, _u32p(s)))
        self.width, self.rows = int(s[0]), int(s[1])
        if not self._band:                      # whole-frame and multi-device handles: the frame IS the new size
            self.full_height = self.rows

    def SetCameraParameters(self, fov, focalLength, aperture):
        self._lib.rt_tracer_set_camera_parameters(self._h, fov, focalLength, aperture)

    def RotateCamera(self, angles):
        self._lib.rt_tracer_rotate_camera(self._h, _f32p(np.array(angles, np.float32)))

    def UploadScene(self, hostData):
        """hostData: (3N, 4) float32.  Like the reference, an invalid size is rejected
        without raising (RayTracerImpl.cu:121-125); returns False in that case."""
        a = np.ascontiguousarray(hostData, np.float32).reshape(-1, 4)
        rc = self._lib.rt_tracer_upload_scene(self._h, a.ctypes.data, a.shape[0])
        if rc == 1:
            return False
        self._check(rc)
        self._scene_rows, self._scene_edges = a.copy(), False
        return True

    def UploadSceneEdges(self, hostData):
        """(3N, 4) float32 in the v0, e0, e1 layout of Documentation/gpu.meshes.txt:16-17."""
        a = np.ascontiguousarray(hostData, np.float32).reshape(-1, 4)
        rc = self._lib.rt_tracer_upload_scene_edges(self._h, a.ctypes.data, a.shape[0])
        if rc == 1:
            return False
        self._check(rc)
        self._scene_rows, self._scene_edges = a.copy(), True
        return True

    def SetUpdateCallback(self, callback):
        self._set_cb("update", callback, self._lib.rt_tracer_set_update_callback)

    def SetFinishedCallback(self, callback):
        self._set_cb("finished", callback, self._lib.rt_tracer_set_finished_callback)

    # ---- extensions ------------------------------------------------------------------
    def Wait(self):
        ok = bool(self._lib.rt_tracer_wait(self._h))
        self._retired.clear()                  # the render thread has ended: nobody holds a replaced thunk
        return ok

    def SetSeed(self, seed):
        self._check(self._lib.rt_tracer_set_seed(self._h, int(seed)))

    def UploadSpheres(self, spheres):
        a = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        self._check(self._lib.rt_tracer_upload_spheres(self._h, a.ctypes.data, a.shape[0]))
        self._sphere_rows = a.copy()

    def TraceEnqueue(self, iterationCount, samplesPerIteration):
        self._check(self._lib.rt_tracer_trace_enqueue(self._h, iterationCount, samplesPerIteration))

    def TraceEnqueueN(self, iterationCount, samplesPerIteration, n_steps):
        """n_steps passes of TraceEnqueue enqueued by one call (the step loop runs inside the library)."""
        self._check(self._lib.rt_tracer_trace_enqueue_n(self._h, iterationCount, samplesPerIteration, n_steps))

    def Launch(self, samples, clear_first=False, emit_image=False, iterations=1):
        """`iterations` iterations of TraceFunct's loop on the device as one launch (no callbacks, no
        host sync); iterations <= FusedIterations(samples)."""
        if iterations == 1:
            self._check(self._lib.rt_tracer_launch(self._h, samples, int(clear_first), int(emit_image)))
        else:
            self._check(self._lib.rt_tracer_launch_iterations(self._h, samples, iterations, int(clear_first), int(emit_image)))

    def SetListReuse(self, across_traces=True):
        """Keep the tiles' candidate lists from one Trace to the next while nothing they depend on changes
        (default) or only within one Trace (False: every Trace classifies afresh)."""
        self._check(self._lib.rt_tracer_set_list_reuse(self._h, 1 if across_traces else 0))

    def SetImageMirror(self, device_visible_ptr):
        """Emitting Launch/TraceEnqueue launches also write the BGRA8 image to this device-visible
        buffer (e.g. a collective's send tensor); 0/None switches it off."""
        self._check(self._lib.rt_tracer_set_image_mirror(self._h, C.c_void_p(device_visible_ptr or 0)))

    def FusedIterations(self, samples):
        """How many consecutive iterations one launch may run (1 = no fusing)."""
        return max(1, int(self._lib.rt_tracer_fused_iterations(self._h, samples)))

    def Sync(self):
        self._check(self._lib.rt_tracer_sync(self._h))

    def TraceStats(self, samples):
        """One instrumented launch; see rt_tracer_trace_stats in include/rt_mi355x.h."""
        out = (C.c_uint64 * 16)()
        self._check(self._lib.rt_tracer_trace_stats(self._h, samples, out))
        v = [int(x) for x in out]
        return {"exit_det": v[0], "exit_u": v[1], "exit_v": v[2], "exit_hit": v[3],
                "skip_a": v[4], "skip_b": v[5], "skip_c": v[6], "reach_d": v[7],
                "bin_candidates": v[8], "bin_rounds": v[9], "pretest_skips": v[10],
                "tiles_by_list": {"0": v[11], "1": v[12], "sure": v[13], "2": v[14], "more": v[15]}}

    def KernelTime(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        self._lib.rt_tracer_kernel_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0)
        return ms.value, n.value

    def LaunchTime(self, reset=True):
        """(total ms, launches) of the sampled launches by their cost: split launches to the end of the later half (rt_tracer_launch_time)."""
        ms, n = C.c_double(), C.c_uint64()
        self._lib.rt_tracer_launch_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0)
        return ms.value, n.value

    def _read(self, which, dtype, shape):
        out = np.empty(shape, dtype)
        self._check(self._lib.rt_tracer_read_buffer(self._h, which, out.ctypes.data, out.nbytes))
        return out

    def RenderBuffer(self):
        return self._read(BUF_RENDER, np.float32, (self.rows, self.width, 4))

    def SampleCounts(self):
        return self._read(BUF_COUNTS, np.uint32, (self.rows, self.width))

    def Image(self):
        return self._read(BUF_IMAGE, np.uint32, (self.rows, self.width))

    def RngStates(self):
        """(rows, W, 6) uint32 {d, v0..v4} per pixel (device layout is 6 planes)."""
        planes = self._read(BUF_RNG, np.uint32, (6, self.rows, self.width))
        return np.ascontiguousarray(np.moveaxis(planes, 0, -1))

    # ---- a frame sharded over several GPUs ------------------------------------------------------
    def JoinGroup(self, n_ranks, rank, unique_id=None, row_begin=None):
        """This band tracer becomes rank `rank` of `n_ranks` processes that share one frame (collective call).
        row_begin: n_ranks + 1 boundaries of an explicit partition (default: equal bands)."""
        if row_begin is None:
            self._check(self._lib.rt_tracer_join_group(self._h, n_ranks, rank, unique_id))
        else:
            b = np.ascontiguousarray(row_begin, np.uint32)
            self._check(self._lib.rt_tracer_join_group_bands(self._h, n_ranks, rank, unique_id, _u32p(b)))

    def SetBand(self, row_begin, rows):
        """Move a band tracer to other rows of its frame (buffers and RNG states re-created, like Resize)."""
        self._check(self._lib.rt_tracer_set_band(self._h, row_begin, rows))
        self.rows = int(rows)

    def Rebalance(self):
        """Multi-device tracer: re-partition the rows so that every band costs the same, from the bands' kernel times."""
        self._check(self._lib.rt_tracer_rebalance(self._h))

    def LeaveGroup(self):
        self._check(self._lib.rt_tracer_leave_group(self._h))

    def Frame(self):
        """The gathered (H, W) BGRA8 frame: rank 0 of a group / a multi-device tracer."""
        return self._read(BUF_FRAME, np.uint32, (self.full_height, self.width))

    def GatherTime(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        self._lib.rt_tracer_gather_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0)
        return ms.value, n.value

    def GatherOnly(self):
        """One more exchange of the tiles as they are, no tracing (collective in a multi-process group)."""
        self._check(self._lib.rt_tracer_gather_only(self._h))

    def GroupInfo(self):
        """dict: transport, ranks, band -> rank map, local devices, RCCL version and communicators (rt_tracer_group_info)."""
        import json
        buf = C.create_string_buffer(8192)
        self._check(self._lib.rt_tracer_group_info(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def Bands(self):
        """[{device, row0, rows, rank}] of the handle's bands (one entry for a plain tracer)."""
        out = []
        for k in range(int(self._lib.rt_tracer_band_count(self._h))):
            v = np.zeros(4, np.uint32)
            self._check(self._lib.rt_tracer_band_info(self._h, k, _u32p(v)))
            out.append({"device": int(v[0]), "row0": int(v[1]), "rows": int(v[2]), "rank": int(v[3])})
        return out

    def DevicePointer(self, which):
        return self._lib.rt_tracer_device_pointer(self._h, which)

    def CopyToDevice(self, which, dst_ptr, nbytes):
        self._check(self._lib.rt_tracer_copy_buffer_to_device(self._h, which, dst_ptr, nbytes))

    def CopyToDeviceAsync(self, which, dst_ptr, nbytes):
        """Enqueue the copy on the tracer's stream, no host sync (order other streams with Stream())."""
        self._check(self._lib.rt_tracer_copy_buffer_to_device_async(self._h, which, dst_ptr, nbytes))

    def Stream(self):
        """The tracer's hipStream_t as an integer (torch.cuda.ExternalStream(ptr) wraps it)."""
        return int(self._lib.rt_tracer_stream(self._h) or 0)

    def StreamB(self):
        """The second stream, on which the lower half of split trace launches runs (rt_tracer_stream_b)."""
        return int(self._lib.rt_tracer_stream_b(self._h) or 0)

    def Info(self):
        out = np.zeros(8, np.uint32)
        self._lib.rt_tracer_info(self._h, _u32p(out))
        keys = ("samples_in_flight", "lds_chunk", "lds_bytes", "grid_x", "grid_y", "n_tris", "n_spheres", "device")
        return dict(zip(keys, (int(v) for v in out)))

    def LastError(self):
        return self._lib.rt_tracer_last_error(self._h).decode()

    def DebugTileLists(self):
        """(tiles_y, tiles_x) arrays (count, winner triangle, certain-winner flag) of the stored tile lists."""
        bx, by = (self.width + 31) // 32, (self.rows + 7) // 8
        wpt = np.zeros(1, np.uint32)
        buf = np.zeros(bx * (by + 1) * 4 * 1025, np.uint32)
        self._check(self._lib.rt_dbg_read_tile_lists(self._h, _u32p(buf), buf.size, _u32p(wpt)))
        w = int(wpt[0])
        words = buf[:bx * by * 4 * w].reshape(by, bx * 4, w)[:, :, 0]
        return (words & 0x3FF).astype(np.int32), ((words >> 10) & 0x3FF).astype(np.int32), (words >> 31).astype(bool)

    def DebugOwedState(self):
        """rt_dbg_owed_state: dict of the RNG draws the tracer owes to its certain-winner tiles."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.rt_dbg_owed_state(self._h, out))
        return dict(zip(("owed_draws", "owing_launches", "settles_enqueued", "tables"), (int(x) for x in out)))

    def DebugEnqueueCalls(self):
        """rt_dbg_enqueue_calls: dict of the runtime calls the trace launches' enqueue path issued since the last read (cleared by
        it); `calls` = launches + records + waits.  None with a library that has no such entry (an older build in an A/B)."""
        if not hasattr(self._lib, "rt_dbg_enqueue_calls"):
            return None
        out = (C.c_uint64 * 8)()
        self._check(self._lib.rt_dbg_enqueue_calls(self._h, out))
        d = dict(zip(("steps", "launches", "records", "waits", "ready_records", "free_records", "stop_events"), (int(x) for x in out)))
        d["calls"] = d["launches"] + d["records"] + d["waits"]
        return d

    def DebugListBuilds(self):
        """rt_dbg_list_builds: the small-scene list builds since the tracer was created, per builder kernel -- [region pairs,
        regions, one-level tiles of up to 32 triangles, one-level tiles]."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.rt_dbg_list_builds(self._h, out))
        return [int(x) for x in out]

    def DebugWaveListCounts(self, half=0):
        """(counts, capacity): candidate count per tile (grid order of the half's launch; 0xFFFFFFFF = overflow) of a dense scene's
        lists in HBM (rt_dbg_wave_list_counts)."""
        n, cap = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        buf = np.zeros(((self.width + 31) // 32) * ((self.rows + 7) // 8 + 1) * 4, np.uint32)
        self._check(self._lib.rt_dbg_wave_list_counts(self._h, half, _u32p(buf), buf.size, _u32p(n), _u32p(cap)))
        return buf[:int(n[0])].copy(), int(cap[0])

    def DebugTileListWords(self):
        """(tiles_y, tiles_x, 1 + bin_list) words of the stored tile lists: word 0 = count | winner << 10 | certain << 31, then
        the kept triangle indices in ascending order (rt_dbg_read_tile_lists)."""
        bx, by = (self.width + 31) // 32, (self.rows + 7) // 8
        wpt = np.zeros(1, np.uint32)
        buf = np.zeros(bx * (by + 1) * 4 * 1025, np.uint32)
        self._check(self._lib.rt_dbg_read_tile_lists(self._h, _u32p(buf), buf.size, _u32p(wpt)))
        w = int(wpt[0])
        return buf[:bx * by * 4 * w].reshape(by, bx * 4, w).copy()

    def DebugFocalBoxes(self, curv_scale=1.0):
        """(boxes (tiles_y, tiles_x, 8): lo[3], hi[3], corner path, usable; focal (rows, width, 3)) of a trace launch's tiles."""
        bx, by = (self.width + 31) // 32, (self.rows + 7) // 8
        boxes = np.zeros((by, bx * 4, 8), np.float32)
        focal = np.zeros((self.rows, self.width, 3), np.float32)
        self._check(self._lib.rt_dbg_focal_boxes(self._h, float(curv_scale), _f32p(boxes), boxes.size, _f32p(focal), focal.size))
        return boxes, focal

    def DebugClassify(self, regions, level=0, forms=False, slack_milli=1000):
        """rt_dbg_classify: (header (n, 16), records (n, n_tris, 12 | 32)) for the regions [(x0, y0)] of the band."""
        reg = np.ascontiguousarray(regions, np.uint32).reshape(-1, 2)
        n_tris = self.Info()["n_tris"]
        per = 16 + n_tris * (32 if forms else 12)
        out = np.zeros((reg.shape[0], per), np.float32)
        self._check(self._lib.rt_dbg_classify(self._h, level, 1 if forms else 0, slack_milli, _u32p(reg), reg.shape[0], _f32p(out), out.size))
        return out[:, :16], out[:, 16:].reshape(reg.shape[0], n_tris, 32 if forms else 12)

    # ---- ray queries (rt_tracer_intersect / _device, rt_tracer_pick, rt_tracer_focus_at) -----------------------------
    def Intersect(self, rays):
        """What each ray hits, under the tracer's arithmetic and hit rule.  rays: (n, 6) float32 {origin, direction}, used as
        given.  A numpy array -> structured array HIT_DTYPE (t, u, v, prim), on return.  A contiguous torch float32 tensor
        on the tracer's device -> (n, 4) float32 tensor {t, u, v, prim bits} (column 3 .view(torch.int32)), enqueued on
        torch.cuda.current_stream() without a host synchronisation.  prim: triangle index, n_tris + sphere index, or -1."""
        if type(rays).__module__.startswith("torch"):
            return self._intersect_tensor(rays)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        hits = np.zeros(r.shape[0], HIT_DTYPE)
        self._check(self._lib.rt_tracer_intersect(self._h, r.ctypes.data, r.shape[0], hits.ctypes.data))
        return hits

    def _intersect_tensor(self, rays):
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 6 or not rays.is_contiguous():
            raise ValueError("Intersect: expected a contiguous (n, 6) float32 tensor")
        stream = self._stream_of("Intersect", "rays", rays)
        hits = torch.empty((rays.shape[0], 4), dtype=torch.float32, device=rays.device)
        self._check(self._lib.rt_tracer_intersect_device(self._h, rays.data_ptr(), rays.shape[0], hits.data_ptr(), stream))
        return hits

    def _stream_of(self, who, what, t):
        """The tensor paths' device check (`what`: how the query calls its input) -> torch's current stream on that device."""
        import torch
        dev = self.Bands()[0]["device"]
        if t.device.type != "cuda" or t.device.index != dev:
            raise ValueError("%s: the %s are on %s, the tracer on cuda:%d" % (who, what, t.device, dev))
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    @staticmethod
    def _max_hits(who, max_hits):
        k = int(max_hits)
        if k != max_hits or not 1 <= k <= RT_MAX_HITS:
            raise ValueError("%s: max_hits = %r (1 to %d)" % (who, max_hits, RT_MAX_HITS))
        return k

    def Pick(self, pixels, return_rays=False):
        """Pinhole rays of full-image (x, y) pixels (one pair or (n, 2)) against the scene: structured array HIT_DTYPE,
        and with return_rays the (n, 6) rays as well."""
        pix = np.ascontiguousarray(pixels, np.uint32).reshape(-1, 2)
        hits = np.zeros(pix.shape[0], HIT_DTYPE)
        rays = np.zeros((pix.shape[0], 6), np.float32) if return_rays else None
        self._check(self._lib.rt_tracer_pick(self._h, pix.ctypes.data, pix.shape[0], hits.ctypes.data,
                                             None if rays is None else rays.ctypes.data))
        return (hits, rays) if return_rays else hits

    def FocusAt(self, x, y):
        """Sets the focal length to the distance the pinhole ray of pixel (x, y) travels to its hit; returns it.  Raises
        RtError (camera unchanged) on a background pixel or a hit that is not in front of the camera."""
        f = C.c_float()
        self._check(self._lib.rt_tracer_focus_at(self._h, x, y, C.byref(f)))
        return np.float32(f.value)

    @staticmethod
    def _segs_array(who, segs):
        s = np.asarray(segs, np.float32)
        if s.ndim == 0 or s.shape[-1] != 8:                                # (an (n, 6) ray array is not silently reinterpreted)
            raise ValueError("%s: expected (n, 8) float32 segments, got shape %s" % (who, s.shape))
        return np.ascontiguousarray(s).reshape(-1, 8)

    def _segs_tensor(self, who, segs, max_hits=1):
        """-> (max_hits checked, stream): dtype and shape, then max_hits (IntersectAll's), then the device."""
        import torch
        if segs.dtype != torch.float32 or segs.dim() != 2 or segs.shape[1] != 8 or not segs.is_contiguous():
            raise ValueError("%s: expected a contiguous (n, 8) float32 tensor" % who)
        return self._max_hits(who, max_hits), self._stream_of(who, "segments", segs)

    def Occluded(self, segs):
        """Visibility: is each ray blocked within its own interval?  segs: (n, 8) float32 {origin, direction (used as given),
        tmin, tmax}; the answer is 1 when some primitive is hit with tmin <= t <= tmax (closed, fp32; NaN never occludes),
        whatever the tracer's hit rule.  A numpy array -> bool array, on return.  A contiguous torch float32 tensor on the
        tracer's device -> uint8 tensor, enqueued on torch.cuda.current_stream() without a host synchronisation."""
        if type(segs).__module__.startswith("torch"):
            return self._occluded_tensor(segs)
        s = self._segs_array("Occluded", segs)
        out = np.zeros(s.shape[0], np.uint8)
        self._check(self._lib.rt_tracer_occluded(self._h, s.ctypes.data, s.shape[0], out.ctypes.data))
        return out.view(np.bool_)

    def _occluded_tensor(self, segs):
        import torch
        _, stream = self._segs_tensor("Occluded", segs)
        out = torch.empty((segs.shape[0],), dtype=torch.uint8, device=segs.device)
        self._check(self._lib.rt_tracer_occluded_device(self._h, segs.data_ptr(), segs.shape[0], out.data_ptr(), stream))
        return out

    def Exposure(self, points, directions, tmin=None, tmax=None, world=False):
        """A bundle of rays per point as one bit mask (rt_tracer_exposure).  points: (n, 8) float32 {origin, unit normal, tmin,
        tmax} laid out like Occluded's segments, or (n, 6) with the scalar tmin / tmax (default 0, +inf) filled in; directions:
        (k, 3) or (k, 4), 1 <= k <= RT_MAX_DIRS, shared by all points -- in the frame of each point's normal (z along it), or
        with world=True used as given (the normals are then not read).  Bit j of mask i is set when direction j from point i is
        OPEN: Occluded would answer False for {origin_i, d_ij, tmin_i, tmax_i}; bits >= k are 0.  numpy arrays -> (n,) uint64,
        on return.  Contiguous torch float32 tensors on the tracer's device -> (n,) int64 tensor holding the same bit patterns,
        enqueued on torch.cuda.current_stream() without a host synchronisation when points AND directions are such tensors
        (numpy directions beside torch points are uploaded first, a synchronous copy)."""
        if type(points).__module__.startswith("torch"):
            return self._exposure_tensor(points, directions, tmin, tmax, world)
        p = _exposure_points_array("Exposure", points, tmin, tmax)
        d = _dirs_array("Exposure", directions)
        out = np.zeros(p.shape[0], np.uint64)
        self._check(self._lib.rt_tracer_exposure(self._h, p.ctypes.data, p.shape[0], d.ctypes.data, d.shape[0], int(bool(world)),
                                                 out.ctypes.data))
        return out

    def _exposure_tensor(self, points, directions, tmin, tmax, world):
        import torch
        if points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 6:
            q = torch.empty((points.shape[0], 8), dtype=torch.float32, device=points.device)
            q[:, :6], q[:, 6], q[:, 7] = points, float(0.0 if tmin is None else tmin), float(np.inf if tmax is None else tmax)
            points = q
        elif tmin is not None or tmax is not None:
            raise ValueError("Exposure: (n, 8) points carry their own tmin and tmax")
        _, stream = self._segs_tensor("Exposure", points)
        d = directions
        if not type(d).__module__.startswith("torch"):
            d = torch.from_numpy(_dirs_array("Exposure", d)).to(points.device)
        if d.dtype != torch.float32 or d.dim() != 2 or d.shape[1] not in (3, 4) or not 1 <= d.shape[0] <= RT_MAX_DIRS:
            raise ValueError("Exposure: expected (k, 3) or (k, 4) float32 directions, 1 <= k <= %d" % RT_MAX_DIRS)
        if d.device != points.device:
            raise ValueError("Exposure: the directions are on %s, the points on %s" % (d.device, points.device))
        if d.shape[1] == 3:
            d4 = torch.zeros((d.shape[0], 4), dtype=torch.float32, device=d.device)
            d4[:, :3] = d
            d = d4
        elif not d.is_contiguous():
            raise ValueError("Exposure: expected contiguous (k, 4) float32 directions")
        out = torch.empty((points.shape[0],), dtype=torch.int64, device=points.device)
        self._check(self._lib.rt_tracer_exposure_device(self._h, points.data_ptr(), points.shape[0], d.data_ptr(), d.shape[0],
                                                        int(bool(world)), out.data_ptr(), stream))
        return out

    def AmbientOcclusion(self, points, normals, samples=64, max_distance=np.inf, bias=1e-3):
        """(n,) float32: the share of `samples` cosine-weighted hemisphere directions (hemisphere_directions) about each
        normal that are open over [bias, max_distance] -- 1 = fully exposed.  points, normals: (n, 3) numpy arrays; the
        normals are normalised in float64 on the host.  ceil(samples / RT_MAX_DIRS) calls of Exposure over slices of the set."""
        p = np.asarray(points, np.float32).reshape(-1, 3)
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        if p.shape != nrm.shape:
            raise ValueError("AmbientOcclusion: %d points, %d normals" % (p.shape[0], nrm.shape[0]))
        with np.errstate(all="ignore"):
            nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
        dirs = hemisphere_directions(samples)
        pts = np.empty((p.shape[0], 8), np.float32)
        pts[:, :3], pts[:, 3:6], pts[:, 6], pts[:, 7] = p, nrm, np.float32(bias), np.float32(max_distance)
        count = np.zeros(p.shape[0], np.int64)
        for k in range(0, dirs.shape[0], RT_MAX_DIRS):
            masks = self.Exposure(pts, dirs[k:k + RT_MAX_DIRS])
            count += np.unpackbits(masks.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1, dtype=np.int64)
        return (count / np.float64(dirs.shape[0])).astype(np.float32)

    def DebugExposureRays(self, points, directions, world=False):
        """rt_dbg_exposure_rays on the tracer's device: exposure_rays' (n, k, 8) segments from the device function."""
        p = _exposure_points_array("DebugExposureRays", points, None, None)
        d = _dirs_array("DebugExposureRays", directions)
        out = np.zeros((p.shape[0], d.shape[0], 8), np.float32)
        self._check(self._lib.rt_dbg_exposure_rays(self._h, p.ctypes.data, p.shape[0], d.ctypes.data, d.shape[0], int(bool(world)),
                                                   out.ctypes.data))
        return out

    def IntersectAll(self, segs, max_hits=RT_MAX_HITS):
        """All hits along each ray within its own interval, in order.  segs: (n, 8) float32 as Occluded takes them; 1 <= max_hits
        <= RT_MAX_HITS.  Row i holds the ray's first counts[i] <= max_hits hits with tmin <= t <= tmax in ascending t (equal t by
        ascending prim), then records {0, 0, 0, PRIM_NONE}; counts[i] == max_hits means there may be more (call again with tmin
        = the last t and skip what was seen).  Independent of the tracer's hit rule.  A numpy array -> (hits (n, max_hits)
        HIT_DTYPE, counts (n,) uint32), on return.  A contiguous torch float32 tensor on the tracer's device -> ((n, max_hits, 4)
        float32 {t, u, v, prim bits}, (n,) int32), enqueued on torch.cuda.current_stream() without a host synchronisation."""
        if type(segs).__module__.startswith("torch"):
            return self._intersect_all_tensor(segs, max_hits)
        s = self._segs_array("IntersectAll", segs)
        k = self._max_hits("IntersectAll", max_hits)
        hits = np.zeros((s.shape[0], k), HIT_DTYPE)
        counts = np.zeros(s.shape[0], np.uint32)
        self._check(self._lib.rt_tracer_intersect_all(self._h, s.ctypes.data, s.shape[0], k, hits.ctypes.data, counts.ctypes.data))
        return hits, counts

    def _intersect_all_tensor(self, segs, max_hits=RT_MAX_HITS):
        import torch
        k, stream = self._segs_tensor("IntersectAll", segs, max_hits)
        hits = torch.empty((segs.shape[0], k, 4), dtype=torch.float32, device=segs.device)
        counts = torch.empty((segs.shape[0],), dtype=torch.int32, device=segs.device)
        self._check(self._lib.rt_tracer_intersect_all_device(self._h, segs.data_ptr(), segs.shape[0], k, hits.data_ptr(),
                                                             counts.data_ptr(), stream))
        return hits, counts

    # ---- point queries (rt_tracer_closest_point / _device) -----------------------------------------------------------
    @staticmethod
    def _d2max(max_distance):
        with np.errstate(over="ignore"):
            d = np.float32(max_distance)
            return np.copysign(d * d, d)

    @staticmethod
    def _points_array(who, points, max_distance):
        """-> contiguous (n, 4) float32 {x, y, z, squared radius}: (n, 3) points get _d2max(max_distance) in column 3."""
        p = np.asarray(points, np.float32)
        if p.ndim == 0 or p.shape[-1] not in (3, 4):
            raise ValueError("%s: expected (n, 3) or (n, 4) float32 points, got shape %s" % (who, p.shape))
        if p.shape[-1] == 3:
            q = np.empty(p.shape[:-1] + (4,), np.float32)
            q[..., :3], q[..., 3] = p, RayTracer._d2max(max_distance)
            p = q
        return np.ascontiguousarray(p).reshape(-1, 4)

    def _points_tensor(self, who, points, max_distance, max_hits=1):
        """-> ((n, 4) points as _points_array forms them, max_hits checked, stream): dtype and shape, then max_hits (ClosestAll's),
        then the device, then the contiguity of an (n, 4) tensor."""
        import torch
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] not in (3, 4):
            raise ValueError("%s: expected an (n, 3) or (n, 4) float32 tensor" % who)
        k = self._max_hits(who, max_hits)
        stream = self._stream_of(who, "points", points)
        if points.shape[1] == 3:
            q = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
            q[:, :3] = points
            q[:, 3] = float(self._d2max(max_distance))
            points = q
        elif not points.is_contiguous():
            raise ValueError("%s: expected a contiguous (n, 4) float32 tensor" % who)
        return points, k, stream

    def ClosestPoint(self, points, max_distance=np.inf):
        """The nearest surface point of the scene to each point.  points: (n, 3) float32 x, y, z, searched within max_distance
        (squared on the host in fp32; a negative one keeps its sign and accepts nothing), or (n, 4) with the SQUARED search radius
        of each point in column 3 (+inf = unbounded), as rt_tracer_closest_point takes them.  The answer's t is the squared
        distance, u, v the nearest point's barycentrics (ClosestPositions forms the point), prim the triangle, n_tris + sphere
        index, or PRIM_NONE when nothing lies within the radius.  Independent of the tracer's arithmetic mode and hit rule.  A
        numpy array -> structured array HIT_DTYPE, on return.  A contiguous torch float32 tensor on the tracer's device -> (n, 4)
        float32 tensor {t, u, v, prim bits}, enqueued on torch.cuda.current_stream() without a host synchronisation."""
        if type(points).__module__.startswith("torch"):
            return self._closest_point_tensor(points, max_distance)
        p = self._points_array("ClosestPoint", points, max_distance)
        hits = np.zeros(p.shape[0], HIT_DTYPE)
        self._check(self._lib.rt_tracer_closest_point(self._h, p.ctypes.data, p.shape[0], hits.ctypes.data))
        return hits

    def _closest_point_tensor(self, points, max_distance=np.inf):
        import torch
        points, _, stream = self._points_tensor("ClosestPoint", points, max_distance)
        hits = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
        self._check(self._lib.rt_tracer_closest_point_device(self._h, points.data_ptr(), points.shape[0], hits.data_ptr(), stream))
        return hits

    # ---- the k nearest primitives (rt_tracer_closest_all / _device) ------------------------------------------------------
    def ClosestAll(self, points, max_hits=RT_MAX_HITS, max_distance=np.inf, after=None):
        """The max_hits nearest primitives of the scene to each point, in order.  points and max_distance as ClosestPoint takes
        them; 1 <= max_hits <= RT_MAX_HITS.  Row i holds the point's counts[i] <= max_hits nearest accepted primitives in
        ascending t (equal t by ascending prim), then records {0, 0, 0, PRIM_NONE}; record 0 is ClosestPoint's answer.
        counts[i] == max_hits means there may be more: call again with after[i] = the row's last record (ClosestWithin does).
        after: the cursor, one record per point -- only candidates that sort strictly behind (after.t, after.prim) are
        accepted; a record with prim PRIM_NONE is no cursor.  A numpy array -> (hits (n, max_hits) HIT_DTYPE, counts (n,)
        uint32), on return; after is then a HIT_DTYPE (n,) array.  A torch float32 tensor on the tracer's device -> ((n,
        max_hits, 4) float32 {t, u, v, prim bits}, (n,) int32), enqueued on torch.cuda.current_stream() without a host
        synchronisation; after is then a contiguous (n, 4) float32 tensor."""
        if type(points).__module__.startswith("torch"):
            return self._closest_all_tensor(points, max_hits, max_distance, after)
        p = self._points_array("ClosestAll", points, max_distance)
        k = self._max_hits("ClosestAll", max_hits)
        a = None
        if after is not None:
            a = np.ascontiguousarray(np.asarray(after).reshape(-1))
            if a.dtype != HIT_DTYPE or a.shape[0] != p.shape[0]:
                raise ValueError("ClosestAll: after must be a HIT_DTYPE array with one record per point")
        hits = np.zeros((p.shape[0], k), HIT_DTYPE)
        counts = np.zeros(p.shape[0], np.uint32)
        self._check(self._lib.rt_tracer_closest_all(self._h, p.ctypes.data, None if a is None else a.ctypes.data, p.shape[0], k,
                                                    hits.ctypes.data, counts.ctypes.data))
        return hits, counts

    def _closest_all_tensor(self, points, max_hits=RT_MAX_HITS, max_distance=np.inf, after=None):
        import torch
        points, k, stream = self._points_tensor("ClosestAll", points, max_distance, max_hits)
        if after is not None:
            if (not type(after).__module__.startswith("torch") or after.dtype != torch.float32 or after.dim() != 2 or
                    tuple(after.shape) != (points.shape[0], 4) or not after.is_contiguous() or after.device != points.device):
                raise ValueError("ClosestAll: after must be a contiguous (n, 4) float32 tensor on the points' device")
        hits = torch.empty((points.shape[0], k, 4), dtype=torch.float32, device=points.device)
        counts = torch.empty((points.shape[0],), dtype=torch.int32, device=points.device)
        self._check(self._lib.rt_tracer_closest_all_device(self._h, points.data_ptr(), None if after is None else after.data_ptr(),
                                                           points.shape[0], k, hits.data_ptr(), counts.data_ptr(), stream))
        return hits, counts

    def ClosestWithin(self, points, max_distance, max_hits=RT_MAX_HITS):
        """Every primitive within max_distance of each point (the sphere-overlap query), numpy only: ClosestAll repeated with
        the cursor until every count is below max_hits.  points: (n, 3) with max_distance, or (n, 4) with the squared radius of
        each point in column 3 (max_distance is then not used).  Returns (hits, offsets): the accepted primitives of all
        points, flat, HIT_DTYPE, each point's in ascending (t, prim) order; point i's are hits[offsets[i]:offsets[i + 1]],
        offsets (n + 1,) int64."""
        p = self._points_array("ClosestWithin", points, max_distance)
        k = self._max_hits("ClosestAll", max_hits)
        n = p.shape[0]
        live = np.arange(n)                                                # the points that may have more
        after = None
        parts, owners = [], []
        while live.size:
            hits, counts = self.ClosestAll(p[live], k, after=after)
            keep = np.arange(k)[None, :] < counts[:, None]
            parts.append(hits[keep])
            owners.append(np.repeat(live, counts))
            more = counts == k
            after = np.ascontiguousarray(hits[more, k - 1])
            live = live[more]
        owner = np.concatenate(owners) if owners else np.zeros(0, np.int64)
        flat = np.concatenate(parts) if parts else np.zeros(0, HIT_DTYPE)
        order = np.argsort(owner, kind="stable")                           # rounds are in order within a point already
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(owner, minlength=n), out=offsets[1:])
        return flat[order], offsets

    # ---- region queries (rt_tracer_overlap / _device) ------------------------------------------------------------------
    @staticmethod
    def _boxes_array(who, boxes):
        """-> contiguous (n, 8) float32 {lo xyz, 0, hi xyz, 0}: from (n, 8) as it is (the pads are never read), from (n, 6)
        {lo xyz, hi xyz}, or from a (lo, hi) pair of (n, 3) arrays."""
        if isinstance(boxes, (tuple, list)) and len(boxes) == 2 and np.ndim(boxes[0]) >= 1 and np.shape(boxes[0])[-1] == 3:
            lo, hi = (np.asarray(b, np.float32).reshape(-1, 3) for b in boxes)
            if lo.shape != hi.shape:
                raise ValueError("%s: %d lower corners, %d upper corners" % (who, lo.shape[0], hi.shape[0]))
            b = np.concatenate([lo, hi], axis=1)
        else:
            b = np.asarray(boxes, np.float32)
        if b.ndim == 0 or b.shape[-1] not in (6, 8):
            raise ValueError("%s: expected (n, 6) or (n, 8) float32 boxes or a (lo, hi) pair, got shape %s" % (who, b.shape))
        if b.shape[-1] == 6:
            b = b.reshape(-1, 6)
            q = np.zeros((b.shape[0], 8), np.float32)
            q[:, 0:3], q[:, 4:7] = b[:, 0:3], b[:, 3:6]
            b = q
        return np.ascontiguousarray(b).reshape(-1, 8)

    @staticmethod
    def _overlap_hits(max_hits):
        k = int(max_hits)
        if k != max_hits or not 0 <= k <= RT_MAX_HITS:
            raise ValueError("Overlap: max_hits = %r (0 to %d)" % (max_hits, RT_MAX_HITS))
        return k

    def _region_query(self, name, noun, array, fn, queries, max_hits, after):
        """The numpy form of the three region queries: `array` lays the queries out, `fn` is the C entry point."""
        q = array(name, queries)
        k = self._overlap_hits(max_hits)
        a = None
        if after is not None:
            a = np.ascontiguousarray(after, np.int32).reshape(-1)
            if a.shape[0] != q.shape[0]:
                raise ValueError("%s: after must hold one int32 cursor per %s" % (name, noun))
        prims = np.full((q.shape[0], k), PRIM_NONE, np.int32)
        counts = np.zeros(q.shape[0], np.uint32)
        self._check(fn(self._h, q.ctypes.data, None if a is None else a.ctypes.data, q.shape[0], k,
                       prims.ctypes.data if k else None, counts.ctypes.data))
        return prims, counts

    def _region_tensor(self, name, arg, floats, fn, queries, max_hits, after):
        """Their torch form: a contiguous (n, floats) tensor called `arg`, `fn` the _device entry point."""
        import torch
        if queries.dtype != torch.float32 or queries.dim() != 2 or queries.shape[1] != floats or not queries.is_contiguous():
            raise ValueError("%s: expected a contiguous (n, %d) float32 tensor" % (name, floats))
        k = self._overlap_hits(max_hits)
        stream = self._stream_of(name, arg, queries)
        n = queries.shape[0]
        if after is not None:
            if (not type(after).__module__.startswith("torch") or after.dtype != torch.int32 or tuple(after.shape) != (n,) or
                    not after.is_contiguous() or after.device != queries.device):
                raise ValueError("%s: after must be a contiguous (n,) int32 tensor on the %s' device" % (name, arg))
        prims = torch.empty((n, k), dtype=torch.int32, device=queries.device)
        counts = torch.empty((n,), dtype=torch.int32, device=queries.device)
        self._check(fn(self._h, queries.data_ptr(), None if after is None else after.data_ptr(), n, k,
                       prims.data_ptr() if k else None, counts.data_ptr(), stream))
        return prims, counts

    def _region_all(self, query, array, name, queries, max_hits):
        """Their cursor chain: `query` repeated with the cursor while a count exceeds the row length."""
        q = array(name, queries)
        k = self._max_hits(name, max_hits)
        n = q.shape[0]
        live = np.arange(n)                                                # the queries that have more
        after = None
        parts, owners = [], []
        while live.size:
            prims, counts = query(q[live], k, after=after)
            stored = np.minimum(counts, k)
            keep = np.arange(k)[None, :] < stored[:, None]
            parts.append(prims[keep])
            owners.append(np.repeat(live, stored))
            more = counts > k
            after = np.ascontiguousarray(prims[more, k - 1])
            live = live[more]
        owner = np.concatenate(owners) if owners else np.zeros(0, np.int64)
        flat = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        order = np.argsort(owner, kind="stable")                           # rounds are in order within a query already
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(owner, minlength=n), out=offsets[1:])
        return flat[order], offsets

    def Overlap(self, boxes, max_hits=RT_MAX_HITS, after=None):
        """The primitives that touch each axis-aligned box (rt_tracer_overlap).  boxes: (n, 8) float32 {lo xyz, -, hi xyz, -},
        (n, 6) {lo xyz, hi xyz}, or a (lo, hi) pair of (n, 3) arrays; closed boxes, touching counts; a NaN bound or lo > hi on
        an axis touches nothing.  0 <= max_hits <= RT_MAX_HITS.  Returns (prims (n, max_hits) int32, counts (n,) uint32): row i
        holds the min(counts[i], max_hits) lowest touching prims in ascending order, then PRIM_NONE; counts[i] is the TOTAL
        behind the cursor, so counts[i] > max_hits means there are more (OverlapAll chains the cursor).  after: (n,) int32, only
        prims above after[i] are accepted; PRIM_NONE is no cursor.  Independent of the tracer's arithmetic mode and hit rule; a
        sphere is its surface.  numpy in, numpy out, on return.  A contiguous (n, 8) float32 torch tensor on the tracer's device
        -> ((n, max_hits) int32, (n,) int32) tensors, enqueued on torch.cuda.current_stream() without a host synchronisation;
        after is then a contiguous (n,) int32 tensor."""
        if type(boxes).__module__.startswith("torch"):
            return self._overlap_tensor(boxes, max_hits, after)
        return self._region_query("Overlap", "box", self._boxes_array, self._lib.rt_tracer_overlap, boxes, max_hits, after)

    def _overlap_tensor(self, boxes, max_hits=RT_MAX_HITS, after=None):
        return self._region_tensor("Overlap", "boxes", 8, self._lib.rt_tracer_overlap_device, boxes, max_hits, after)

    def OverlapAll(self, boxes, max_hits=RT_MAX_HITS):
        """Every primitive that touches each box, numpy only: Overlap repeated with the cursor while a count exceeds max_hits
        (1 <= max_hits <= RT_MAX_HITS is the row length of one round).  Returns (prims, offsets): the touching prims of all
        boxes, flat, int32, each box's in ascending order; box i's are prims[offsets[i]:offsets[i + 1]], offsets (n + 1,)
        int64."""
        return self._region_all(self.Overlap, self._boxes_array, "OverlapAll", boxes, max_hits)

    @staticmethod
    def voxel_boxes(origin, spacing, shape):
        """The (nx * ny * nz, 8) float32 boxes of Voxelize's grid, voxel (i, j, k) at row (i * ny + j) * nz + k.  All in fp32,
        per axis:  lo = origin + spacing * float32(i),  hi = origin + spacing * float32(i + 1)  (one multiplication, one
        addition, each rounded) -- so hi of voxel i and lo of voxel i + 1 are the same bits and neighbours share their face."""
        o = np.asarray(origin, np.float32).reshape(3)
        sp = np.broadcast_to(np.asarray(spacing, np.float32), (3,))
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3 or min(shape) < 0:
            raise ValueError("Voxelize: shape must be three non-negative counts")
        edges = [(o[a] + sp[a] * np.arange(shape[a] + 1, dtype=np.float32)).astype(np.float32) for a in range(3)]
        boxes = np.zeros(shape + (8,), np.float32)
        for a in range(3):
            sl = [None, None, None]
            sl[a] = slice(None)
            boxes[..., a] = edges[a][:-1][tuple(sl)]
            boxes[..., 4 + a] = edges[a][1:][tuple(sl)]
        return boxes.reshape(-1, 8)

    def Voxelize(self, origin, spacing, shape):
        """Surface voxelisation: a bool array of `shape` = (nx, ny, nz), True where the closed voxel touches a primitive (the
        surface: a voxel wholly inside a closed mesh or a ball is False; DistanceField / Contains give the solid).  Voxel (i, j,
        k) is the box voxel_boxes states, origin + spacing * (i, j, k) .. origin + spacing * (i + 1, j + 1, k + 1) in fp32;
        spacing is a scalar or one value per axis.  One Overlap call with max_hits = 0: True when counts > 0."""
        boxes = self.voxel_boxes(origin, spacing, shape)
        _, counts = self.Overlap(boxes, 0)
        return (counts > 0).reshape(tuple(int(v) for v in shape))

    # ---- triangle-shaped regions (rt_tracer_overlap_triangles / _device) ---------------------------------------------------
    @staticmethod
    def _triangles_array(who, triangles):
        """-> contiguous (n, 12) float32 {P0 xyz, 0, P1 xyz, 0, P2 xyz, 0}: from (n, 12) as it is (the pads are never read), from
        (n, 3, 3) or from (n, 9) {P0 xyz, P1 xyz, P2 xyz}."""
        t = np.asarray(triangles, np.float32)
        if t.ndim >= 2 and t.shape[-2:] == (3, 3):
            t = t.reshape(-1, 9)
        if t.ndim == 0 or t.shape[-1] not in (9, 12):
            raise ValueError("%s: expected (n, 3, 3), (n, 9) or (n, 12) float32 triangles, got shape %s" % (who, t.shape))
        if t.shape[-1] == 9:
            t = t.reshape(-1, 3, 3)
            q = np.zeros((t.shape[0], 3, 4), np.float32)
            q[:, :, :3] = t
            t = q
        return np.ascontiguousarray(t).reshape(-1, 12)

    def OverlapTriangles(self, triangles, max_hits=RT_MAX_HITS, after=None):
        """The primitives that touch each query triangle (rt_tracer_overlap_triangles).  triangles: (n, 3, 3) or (n, 9) float32
        corners, or (n, 12) {P0 xyz, -, P1 xyz, -, P2 xyz, -}; closed, touching counts; a query with a non-finite coordinate
        touches nothing.  max_hits, after and the returned (prims (n, max_hits) int32, counts (n,) uint32) are Overlap's: the
        lowest touching prims in ascending order, then PRIM_NONE, and the TOTAL behind the cursor (OverlapTrianglesAll chains
        it).  A query corner bit-equal to a corner of a scene triangle's record always touches that triangle.  Independent of
        the tracer's arithmetic mode and hit rule; a sphere is its surface.  numpy in, numpy out, on return.  A contiguous
        (n, 12) float32 torch tensor on the tracer's device -> ((n, max_hits) int32, (n,) int32) tensors, enqueued on
        torch.cuda.current_stream() without a host synchronisation; after is then a contiguous (n,) int32 tensor."""
        if type(triangles).__module__.startswith("torch"):
            return self._overlap_triangles_tensor(triangles, max_hits, after)
        return self._region_query("OverlapTriangles", "triangle", self._triangles_array, self._lib.rt_tracer_overlap_triangles, triangles,
                                  max_hits, after)

    def _overlap_triangles_tensor(self, triangles, max_hits=RT_MAX_HITS, after=None):
        return self._region_tensor("OverlapTriangles", "triangles", 12, self._lib.rt_tracer_overlap_triangles_device, triangles, max_hits,
                                   after)

    def OverlapTrianglesAll(self, triangles, max_hits=RT_MAX_HITS):
        """Every primitive that touches each query triangle, numpy only: OverlapTriangles repeated with the cursor while a count
        exceeds max_hits (1 <= max_hits <= RT_MAX_HITS is the row length of one round).  Returns (prims, offsets) as OverlapAll
        does: triangle i's prims, ascending, are prims[offsets[i]:offsets[i + 1]]."""
        return self._region_all(self.OverlapTriangles, self._triangles_array, "OverlapTrianglesAll", triangles, max_hits)

    @staticmethod
    def scene_corners(rows, edges=False):
        """(T, 3, 3) float32: the corners SelfIntersections queries and compares -- the uploaded vertices of the vertex layout;
        A = v0, fl(v0 + e1), fl(v0 + e2) of the edge layout (the corners the rule itself works on)."""
        r = np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3].copy()
        if edges:
            r[:, 1], r[:, 2] = r[:, 0] + r[:, 1], r[:, 0] + r[:, 2]
        return r

    def SelfIntersections(self):
        """The pairs (i, j), i < j, of the scene's own triangles that touch without sharing a corner, (m, 2) int32 in ascending
        order: every triangle of the last upload queried against the scene (OverlapTrianglesAll), spheres left out.  Two
        triangles share a corner when any corner of one == (on values) any corner of the other, corners as scene_corners
        gives them; neighbours of a mesh therefore never count, and a FOLD BETWEEN NEIGHBOURS (two triangles that share an edge
        or a vertex and also cross or lie on each other) is not reported.  What is reported is what makes Contains and
        SignedDistance untrustworthy on a mesh: parts that pass through each other."""
        if self._scene_rows is None or self._scene_rows.shape[0] == 0:
            return np.zeros((0, 2), np.int32)
        c = self.scene_corners(self._scene_rows, self._scene_edges)
        return self.self_pairs(c, *self.OverlapTrianglesAll(c))

    @staticmethod
    def self_pairs(corners, prims, offsets):
        """SelfIntersections' second half: from the scene's corners (T, 3, 3) and OverlapTrianglesAll's answer for them, the
        pairs i < j of triangles that are accepted and share no corner (== on values), (m, 2) int32."""
        c = np.asarray(corners, np.float32).reshape(-1, 3, 3)
        i = np.repeat(np.arange(c.shape[0]), np.diff(offsets))
        j = np.asarray(prims).astype(np.int64)
        keep = (j > i) & (j < c.shape[0])                                  # each pair once; no spheres
        i, j = i[keep], j[keep]
        with np.errstate(invalid="ignore"):
            shared = (c[i][:, :, None, :] == c[j][:, None, :, :]).all(axis=3).any(axis=(1, 2))
        return np.stack([i[~shared], j[~shared]], axis=1).astype(np.int32)

    # ---- hexahedron-shaped regions: frusta, oriented boxes (rt_tracer_overlap_hexahedra / _device) -------------------------
    @staticmethod
    def _hexahedra_array(who, corners):
        """-> contiguous (n, 32) float32, eight rows {C_k xyz, 0}: from (n, 32) or (n, 8, 4) as it is (the pads are never read),
        or from (n, 8, 3)."""
        c = np.asarray(corners, np.float32)
        if c.ndim >= 2 and c.shape[-2:] == (8, 4):
            c = c.reshape(-1, 32)
        elif c.ndim >= 2 and c.shape[-2:] == (8, 3):
            q = np.zeros((c.size // 24, 8, 4), np.float32)
            q[:, :, :3] = c.reshape(-1, 8, 3)
            c = q.reshape(-1, 32)
        if c.ndim == 0 or c.shape[-1] != 32:
            raise ValueError("%s: expected (n, 8, 3), (n, 8, 4) or (n, 32) float32 corners, got shape %s" % (who, c.shape))
        return np.ascontiguousarray(c).reshape(-1, 32)

    def OverlapHexahedra(self, corners, max_hits=RT_MAX_HITS, after=None):
        """The primitives that touch each hexahedron (rt_tracer_overlap_hexahedra): the convex hull of eight corners in box-like
        order -- bit 0 of the corner index is the side along the region's first direction, bit 1 the second, bit 2 the third
        (box_corners, oriented_box_corners and frustum_corners build them).  corners: (n, 8, 3), (n, 8, 4) or (n, 32) float32
        {C_k xyz, -}; closed, touching counts; a region with a non-finite coordinate touches nothing.  max_hits, after and the
        returned (prims (n, max_hits) int32, counts (n,) uint32) are Overlap's: the lowest touching prims in ascending order,
        then PRIM_NONE, and the TOTAL behind the cursor (OverlapHexahedraAll chains it).  Independent of the tracer's arithmetic
        mode and hit rule; a sphere is its surface.  numpy in, numpy out, on return.  A contiguous (n, 32) float32 torch tensor
        on the tracer's device -> ((n, max_hits) int32, (n,) int32) tensors, enqueued on torch.cuda.current_stream() without a
        host synchronisation; after is then a contiguous (n,) int32 tensor."""
        if type(corners).__module__.startswith("torch"):
            return self._overlap_hexahedra_tensor(corners, max_hits, after)
        return self._region_query("OverlapHexahedra", "region", self._hexahedra_array, self._lib.rt_tracer_overlap_hexahedra, corners,
                                  max_hits, after)

    def _overlap_hexahedra_tensor(self, corners, max_hits=RT_MAX_HITS, after=None):
        return self._region_tensor("OverlapHexahedra", "corners", 32, self._lib.rt_tracer_overlap_hexahedra_device, corners, max_hits,
                                   after)

    def OverlapHexahedraAll(self, corners, max_hits=RT_MAX_HITS):
        """Every primitive that touches each hexahedron, numpy only: OverlapHexahedra repeated with the cursor while a count
        exceeds max_hits (1 <= max_hits <= RT_MAX_HITS is the row length of one round).  Returns (prims, offsets) as OverlapAll
        does: region i's prims, ascending, are prims[offsets[i]:offsets[i + 1]]."""
        return self._region_all(self.OverlapHexahedra, self._hexahedra_array, "OverlapHexahedraAll", corners, max_hits)

    # ---- planes and slabs (rt_tracer_section / rt_tracer_section_segments, and their _device forms) -------------------------
    @staticmethod
    def plane_rows(normal, d0, d1=None):
        """(n, 8) float32 {nx, ny, nz, d0, d1, 0, 0, 0}: the slabs d0 <= normal.x <= d1 of Section, a plane where d1 is None (d1 =
        d0).  normal (3,) or (n, 3), used as given (not normalised); d0, d1 scalars or (n,); the three broadcast to the longest."""
        nrm = np.asarray(normal, np.float32).reshape(-1, 3)
        a = np.asarray(d0, np.float32).reshape(-1)
        b = a if d1 is None else np.asarray(d1, np.float32).reshape(-1)
        sizes = (nrm.shape[0], a.shape[0], b.shape[0])
        out = np.zeros((0 if 0 in sizes else max(sizes), 8), np.float32)
        out[:, 0:3], out[:, 3], out[:, 4] = nrm, a, b
        return out

    @staticmethod
    def _planes_array(who, planes):
        """-> contiguous (n, 8) float32 {nx, ny, nz, d0, d1, 0, 0, 0}: from (n, 8) as it is (the pads are never read), from (n, 5)
        {n xyz, d0, d1}, or from (n, 4) {n xyz, d}, a plane."""
        p = np.asarray(planes, np.float32)
        if p.ndim == 0 or p.shape[-1] not in (4, 5, 8):
            raise ValueError("%s: expected (n, 4), (n, 5) or (n, 8) float32 planes, got shape %s" % (who, p.shape))
        if p.shape[-1] != 8:
            w = p.shape[-1]
            p = p.reshape(-1, w)
            q = np.zeros((p.shape[0], 8), np.float32)
            q[:, :w] = p
            if w == 4:
                q[:, 4] = p[:, 3]
            p = q
        return np.ascontiguousarray(p).reshape(-1, 8)

    def Section(self, planes, max_hits=RT_MAX_HITS, after=None):
        """The primitives each plane or slab cuts (rt_tracer_section): the region d0 <= n.x <= d1, a plane when d0 == d1, a
        half-space when one end is infinite (plane_rows builds the rows).  planes: (n, 8) float32 {nx, ny, nz, d0, d1, -, -, -},
        (n, 5) {n xyz, d0, d1} or (n, 4) {n xyz, d}; closed, touching counts; a non-finite normal, a NaN or d0 > d1 cuts nothing.
        max_hits, after and the returned (prims (n, max_hits) int32, counts (n,) uint32) are Overlap's: the lowest cut prims in
        ascending order, then PRIM_NONE, and the TOTAL behind the cursor (SectionAll chains it).  Independent of the tracer's
        arithmetic mode and hit rule; a sphere is its surface.  numpy in, numpy out, on return.  A contiguous (n, 8) float32
        torch tensor on the tracer's device -> ((n, max_hits) int32, (n,) int32) tensors, enqueued on
        torch.cuda.current_stream() without a host synchronisation; after is then a contiguous (n,) int32 tensor."""
        if type(planes).__module__.startswith("torch"):
            return self._region_tensor("Section", "planes", 8, self._lib.rt_tracer_section_device, planes, max_hits, after)
        return self._region_query("Section", "plane", self._planes_array, self._lib.rt_tracer_section, planes, max_hits, after)

    def SectionAll(self, planes, max_hits=RT_MAX_HITS):
        """Every primitive each plane or slab cuts, numpy only: Section repeated with the cursor while a count exceeds max_hits
        (1 <= max_hits <= RT_MAX_HITS is the row length of one round).  Returns (prims, offsets) as OverlapAll does: plane i's
        prims, ascending, are prims[offsets[i]:offsets[i + 1]]."""
        return self._region_all(self.Section, self._planes_array, "SectionAll", planes, max_hits)

    def SectionSegments(self, planes, prims, side=0):
        """Where the plane n.x = d0 (side 0) or n.x = d1 (side 1) cuts the prims Section returned (rt_tracer_section_segments):
        prims of shape (n,) or (n, per_plane) int32, per_plane <= RT_MAX_HITS -> CUT_DTYPE of the same shape {p0, kind, p1,
        features}: CUT_SEGMENT from p0 to p1 along n x (e1 x e2), CUT_TOUCH (the on-corners), CUT_COPLANAR, CUT_CIRCLE (a
        sphere: p0 the circle's centre, p1[0] its radius) or CUT_NONE (PRIM_NONE, a prim outside the scene, no cut).  features
        = f0 | f1 << 8 names the edge (0 AB, 1 BC, 2 CA) or corner (4 A, 5 B, 6 C) each point lies on.  torch: planes a
        contiguous (n, 8) float32 tensor, prims a contiguous (n,) or (n, per_plane) int32 tensor on its device -> (..., 8)
        float32 {p0 xyz, kind bits, p1 xyz, features bits}, enqueued on torch.cuda.current_stream()."""
        side = int(side)
        if type(planes).__module__.startswith("torch"):
            import torch
            if planes.dtype != torch.float32 or planes.dim() != 2 or planes.shape[1] != 8 or not planes.is_contiguous():
                raise ValueError("SectionSegments: expected a contiguous (n, 8) float32 tensor")
            stream = self._stream_of("SectionSegments", "planes", planes)
            n = planes.shape[0]
            if (not type(prims).__module__.startswith("torch") or prims.dtype != torch.int32 or prims.dim() not in (1, 2) or
                    prims.shape[0] != n or not prims.is_contiguous() or prims.device != planes.device):
                raise ValueError("SectionSegments: prims must be a contiguous (n,) or (n, per_plane) int32 tensor on the planes' device")
            k = 1 if prims.dim() == 1 else self._max_hits("SectionSegments", prims.shape[1])
            cuts = torch.empty(tuple(prims.shape) + (8,), dtype=torch.float32, device=planes.device)
            self._check(self._lib.rt_tracer_section_segments_device(self._h, planes.data_ptr(), prims.data_ptr(), n, k, side,
                                                                    cuts.data_ptr(), stream))
            return cuts
        q = self._planes_array("SectionSegments", planes)
        r = np.ascontiguousarray(prims, np.int32)
        if r.ndim not in (1, 2) or r.shape[0] != q.shape[0]:
            raise ValueError("SectionSegments: expected the int32 prims (n,) or (n, per_plane) of these %d planes" % q.shape[0])
        k = 1 if r.ndim == 1 else self._max_hits("SectionSegments", r.shape[1])
        cuts = np.zeros(r.shape, CUT_DTYPE)
        self._check(self._lib.rt_tracer_section_segments(self._h, q.ctypes.data, r.ctypes.data, q.shape[0], k, side, cuts.ctypes.data))
        return cuts

    def Slice(self, normal, offsets):
        """The contour segments of the scene in the planes normal.x = offsets[i], numpy only: a plane per offset (plane_rows),
        SectionAll, then SectionSegments on every returned prim.  Returns (cuts, layer_offsets): the CUT_DTYPE records of kind
        CUT_SEGMENT of all layers, flat; layer i's are cuts[layer_offsets[i]:layer_offsets[i + 1]], layer_offsets (n + 1,)
        int64.  Touching and coplanar triangles and spheres' circles are left out (SectionSegments returns them)."""
        planes = self.plane_rows(normal, np.asarray(offsets, np.float32).reshape(-1))
        n = planes.shape[0]
        prims, po = self.SectionAll(planes)
        owner = np.repeat(np.arange(n), np.diff(po))
        cuts = self.SectionSegments(planes[owner], prims) if prims.size else np.zeros(0, CUT_DTYPE)
        keep = cuts["kind"] == CUT_SEGMENT
        layer_offsets = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(owner[keep], minlength=n), out=layer_offsets[1:])
        return cuts[keep], layer_offsets

    @staticmethod
    def box_corners(lo, hi):
        """(n, 8, 3) float32: the corners of axis-aligned boxes lo, hi ((3,) or (n, 3)) in OverlapHexahedra's order; no
        arithmetic, C_k takes hi's component where bit 0 / 1 / 2 of k is set (x / y / z) and lo's elsewhere."""
        lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
        out = np.empty((lo.shape[0], 8, 3), np.float32)
        for k in range(8):
            for ax in range(3):
                out[:, k, ax] = (hi if (k >> ax) & 1 else lo)[:, ax]
        return out

    @staticmethod
    def oriented_box_corners(centre, axes):
        """(n, 8, 3) float32: the corners of boxes with centre (3,) or (n, 3) and half-axis vectors axes (3, 3) or (n, 3, 3)
        (rows; they need be neither unit nor orthogonal: a sheared box is a region too), in float32, one rounding per
        operation: C_k = ((centre + s0*axes[0]) + s1*axes[1]) + s2*axes[2] with s_j = +1 where bit j of k is set, else -1
        (the products are exact)."""
        c = np.asarray(centre, np.float32).reshape(-1, 3)
        a = np.asarray(axes, np.float32).reshape(-1, 3, 3)
        out = np.empty((max(c.shape[0], a.shape[0]), 8, 3), np.float32)
        for k in range(8):
            v = c
            for j in range(3):
                v = (v + a[:, j] if (k >> j) & 1 else v - a[:, j]).astype(np.float32)
            out[:, k] = v
        return out

    @staticmethod
    def frustum_corners(rays4, near, far):
        """(n, 8, 3) float32: the frustum between four rays, cut at the ray parameters near and far.  rays4: (4, 6) or (n, 4, 6)
        {origin, direction} in the order (x0, y0), (x1, y0), (x0, y1), (x1, y1); near, far: scalars or (n,) -- one parameter for
        the four rays -- or (n, 4), one per ray.  In float32, one rounding per operation: C_k = o_k + near*d_k and
        C_{k+4} = o_k + far*d_k, k = 0 .. 3.  The caps are the flat quadrilaterals through those points: with unit directions and
        one parameter for all four, a point at parameter t on a ray strictly between the four lies inside only for
        near/cos(a) <= t <= far*cos(a), a the largest angle between that ray and a corner ray (cap_parameters gives per-ray
        parameters whose caps enclose everything between near and far)."""
        r = np.asarray(rays4, np.float32).reshape(-1, 4, 6)
        o, d = r[:, :, :3], r[:, :, 3:]
        n = r.shape[0]

        def per_ray(v):
            v = np.asarray(v, np.float32)
            v = v.reshape(-1, 4) if v.ndim and v.shape[-1] == 4 and v.size == 4 * n else v.reshape(-1, 1)
            return np.broadcast_to(v, (n, 4))[:, :, None]
        out = np.empty((n, 8, 3), np.float32)
        with np.errstate(all="ignore"):
            out[:, :4] = o + (per_ray(near) * d).astype(np.float32)
            out[:, 4:] = o + (per_ray(far) * d).astype(np.float32)
        return out

    @staticmethod
    def cap_parameters(rays4, near, far):
        """Per-ray parameters (near_k, far_k), each (n, 4) float32, whose flat caps ENCLOSE every point o + t*d with
        near <= t <= far on every unit direction d between the four rays (the rays share their origin): the caps lie in planes
        perpendicular to w = ((d0 + d1) + d2) + d3.  With c_k = d_k.w (dot products (x*x' + y*y') + z*z'), cmin = min_k c_k and
        |w| = sqrt(w.w), in float32, one rounding per operation:  near_k = (near * cmin) / c_k  (the direction farthest from w
        is a corner),  far_k = (far * |w|) / c_k  (the direction along w reaches farthest)."""
        d = np.asarray(rays4, np.float32).reshape(-1, 4, 6)[:, :, 3:]
        f32 = np.float32
        with np.errstate(all="ignore"):
            w = ((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]
            dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
            c = dot(d, w[:, None, :])
            cmin = np.minimum(np.minimum(np.minimum(c[:, 0], c[:, 1]), c[:, 2]), c[:, 3])
            wl = np.sqrt(dot(w, w))
            nr = (np.asarray(near, f32).reshape(-1) * cmin)[:, None] / c
            fr = (np.asarray(far, f32).reshape(-1) * wl)[:, None] / c
        assert nr.dtype == f32 and fr.dtype == f32
        return nr, fr

    def PixelFrustum(self, x0, y0, x1, y1, near, far):
        """(8, 3) float32: the frustum of the pixel rectangle [x0, x1] x [y0, y1] (full-image pixels, corners included) that
        holds everything its pixels' pinhole rays meet at ray parameters between near and far: frustum_corners on the rays
        through the CENTRES of the four corner pixels, exactly as Pick(..., return_rays=True) reports them for the camera the
        tracer holds, at cap_parameters' per-ray parameters -- the pinhole directions are unit vectors, so the flat caps
        through the points AT near and far would leave out what the middle of a wide rectangle sees just short of far.  A hit
        that Pick reports with near <= t <= far for a pixel inside the rectangle lies inside this frustum.  The thin lens's
        aperture does not widen it."""
        x0, x1 = sorted((int(x0), int(x1)))
        y0, y1 = sorted((int(y0), int(y1)))
        _, rays = self.Pick([[x0, y0], [x1, y0], [x0, y1], [x1, y1]], return_rays=True)
        return self.frustum_corners(rays, *self.cap_parameters(rays, near, far))[0]

    def SelectRect(self, x0, y0, x1, y1, near=0.0, *, far):
        """Marquee selection: the sorted prims (int32) that touch the frustum of the pixel rectangle between near and far
        (PixelFrustum, OverlapHexahedraAll).  far is required and must be finite."""
        if not (np.isfinite(far) and np.isfinite(near)):
            raise ValueError("SelectRect: near and far must be finite")
        prims, _ = self.OverlapHexahedraAll(self.PixelFrustum(x0, y0, x1, y1, near, far)[None])
        return prims

    # ---- signed point queries (rt_tracer_signed_distance / rt_tracer_closest_sides, and their _device forms) -------------
    def SignedDistance(self, points, max_distance=np.inf):
        """ClosestPoint and the side of the nearest surface each point lies on.  points and max_distance as ClosestPoint takes
        them.  Returns (hits, sides): hits is ClosestPoint's answer bit for bit; sides["s"] > 0 in front of the surface
        (outside a closed, outward-wound mesh), < 0 behind it, 0 on it or undecided; sides["feature"] is the part of the
        triangle that holds the nearest point (0 the face, 1-3 the vertices A, B, C, 4-6 the edges AB, AC, BC, FEATURE_SPHERE,
        or FEATURE_NONE with s = 0 where hits["prim"] is PRIM_NONE).  A numpy array -> (HIT_DTYPE (n,), SIDE_DTYPE (n,)), on
        return.  A torch float32 tensor on the tracer's device -> ((n, 4) float32 {t, u, v, prim bits}, (n, 2) float32 {s,
        feature bits}), enqueued on torch.cuda.current_stream() without a host synchronisation (the first signed query after
        an upload builds the scene's table on the host first)."""
        if type(points).__module__.startswith("torch"):
            import torch
            points, _, stream = self._points_tensor("SignedDistance", points, max_distance)
            hits = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
            sides = torch.empty((points.shape[0], 2), dtype=torch.float32, device=points.device)
            self._check(self._lib.rt_tracer_signed_distance_device(self._h, points.data_ptr(), points.shape[0], hits.data_ptr(),
                                                                   sides.data_ptr(), stream))
            return hits, sides
        p = self._points_array("SignedDistance", points, max_distance)
        hits = np.zeros(p.shape[0], HIT_DTYPE)
        sides = np.zeros(p.shape[0], SIDE_DTYPE)
        self._check(self._lib.rt_tracer_signed_distance(self._h, p.ctypes.data, p.shape[0], hits.ctypes.data, sides.ctypes.data))
        return hits, sides

    def ClosestSides(self, points, hits):
        """The sides of records ClosestPoint or ClosestAll returned for these points: hits of shape (n,) or (n, max_hits)
        HIT_DTYPE (torch: (n, 4) or (n, max_hits, 4) float32, contiguous) -> SIDE_DTYPE of the same shape (torch: (..., 2)
        float32 {s, feature bits}).  Unfilled records of a ClosestAll row come back as {0, FEATURE_NONE}.  points: (n, 3) or
        (n, 4); the radius column is not used."""
        if type(points).__module__.startswith("torch"):
            import torch
            points, _, stream = self._points_tensor("ClosestSides", points, np.inf)
            n = points.shape[0]
            if (not type(hits).__module__.startswith("torch") or hits.dtype != torch.float32 or hits.dim() not in (2, 3) or
                    hits.shape[0] != n or hits.shape[-1] != 4 or not hits.is_contiguous() or hits.device != points.device):
                raise ValueError("ClosestSides: hits must be a contiguous (n, 4) or (n, max_hits, 4) float32 tensor on the points' device")
            k = 1 if hits.dim() == 2 else self._max_hits("ClosestAll", hits.shape[1])
            sides = torch.empty(tuple(hits.shape[:-1]) + (2,), dtype=torch.float32, device=points.device)
            self._check(self._lib.rt_tracer_closest_sides_device(self._h, points.data_ptr(), hits.data_ptr(), n, k, sides.data_ptr(), stream))
            return sides
        p = self._points_array("ClosestSides", points, np.inf)
        h = np.ascontiguousarray(hits)
        if h.dtype != HIT_DTYPE or h.ndim not in (1, 2) or h.shape[0] != p.shape[0]:
            raise ValueError("ClosestSides: expected the HIT_DTYPE answers (n,) or (n, max_hits) of these %d points" % p.shape[0])
        k = 1 if h.ndim == 1 else self._max_hits("ClosestAll", h.shape[1])
        sides = np.zeros(h.shape, SIDE_DTYPE)
        self._check(self._lib.rt_tracer_closest_sides(self._h, p.ctypes.data, h.ctypes.data, p.shape[0], k, sides.ctypes.data))
        return sides

    def Contains(self, points):
        """(n,) bool: the point lies behind the nearest surface (SignedDistance's s < 0, unbounded radius) -- inside, for a
        CLOSED mesh whose triangles are wound consistently outward; meaningless for anything else.  A point on the surface
        (s == 0) is not contained.  numpy only."""
        return self.SignedDistance(np.asarray(points, np.float32)[..., :3])[1]["s"] < 0

    def SignedDistances(self, points):
        """(n,) float32: copysign(sqrt(t), s) of SignedDistance with an unbounded radius, formed on the host -- negative
        inside a closed, outward-wound mesh; NaN without a scene.  numpy only."""
        hits, sides = self.SignedDistance(np.asarray(points, np.float32)[..., :3])
        with np.errstate(invalid="ignore"):
            d = np.copysign(np.sqrt(hits["t"]), sides["s"]).astype(np.float32)
        d[hits["prim"] == PRIM_NONE] = np.nan
        return d

    def DistanceField(self, origin, spacing, shape):
        """SignedDistances on a regular grid: sample (i, j, k) is at origin + spacing * (i, j, k) (float64 on the host, rounded
        to fp32); spacing a scalar or one per axis -> float32 array of `shape` (three extents)."""
        shape = tuple(int(x) for x in shape)
        if len(shape) != 3 or min(shape) < 0:
            raise ValueError("DistanceField: shape = %r (three extents)" % (shape,))
        o = np.asarray(origin, np.float64).reshape(3)
        sp = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
        axes = [o[a] + sp[a] * np.arange(shape[a]) for a in range(3)]
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        return self.SignedDistances(pts).reshape(shape)

    def ClosestPositions(self, points, hits):
        """The nearest points themselves, (n, 3) float32: v0 + u*e1 + v*e2 of the winning triangle's record (fp32, from this
        object's host copy of the last uploaded scene), centre + radius * (p - centre) / |p - centre| for a sphere, NaN where
        hits["prim"] is PRIM_NONE.  points, hits: what ClosestPoint took and returned (numpy)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, np.shape(points)[-1])[:, :3])
        h = np.asarray(hits).reshape(-1)
        if h.dtype != HIT_DTYPE or h.shape[0] != p.shape[0]:
            raise ValueError("ClosestPositions: expected the points and the HIT_DTYPE answers of one ClosestPoint call")
        n_tris = 0 if self._scene_rows is None else self._scene_rows.shape[0] // 3
        out = np.full((p.shape[0], 3), np.nan, np.float32)
        prim = h["prim"].astype(np.int64)
        tri = (prim >= 0) & (prim < n_tris)
        if tri.any():
            r = self._scene_rows.reshape(-1, 3, 4)[prim[tri], :, :3]
            v0 = r[:, 0]
            e1, e2 = (r[:, 1], r[:, 2]) if self._scene_edges else (r[:, 1] - v0, r[:, 2] - v0)
            out[tri] = (v0 + h["u"][tri, None] * e1) + h["v"][tri, None] * e2
        sph = prim >= n_tris
        if sph.any():
            n_sph = 0 if self._sphere_rows is None else self._sphere_rows.shape[0]
            if (prim[sph] - n_tris >= n_sph).any():
                raise ValueError("ClosestPositions: a prim is beyond the scene this object uploaded")
            s = self._sphere_rows[prim[sph] - n_tris]
            w = p[sph] - s[:, :3]
            with np.errstate(all="ignore"):
                out[sph] = s[:, :3] + w * (s[:, 3] / np.sqrt((w * w).sum(axis=1, dtype=np.float32)))[:, None]
        return out

    def Visible(self, a, b, tmin=0.0, tmax=1.0):
        """Line of sight between the points a[i] and b[i] ((n, 3) each): ~Occluded of the rays o = a, d = b - a (fp32, on the
        host) over [tmin, tmax] in units of the segment.  A convenience: the caller chooses the interval that keeps the end
        points' own surfaces out (e.g. tmin=1e-3, tmax=1 - 1e-3)."""
        a = np.asarray(a, np.float32).reshape(-1, 3)
        b = np.asarray(b, np.float32).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError("Visible: %d start points, %d end points" % (a.shape[0], b.shape[0]))
        segs = np.empty((a.shape[0], 8), np.float32)
        segs[:, :3], segs[:, 3:6], segs[:, 6], segs[:, 7] = a, b - a, np.float32(tmin), np.float32(tmax)
        return ~self.Occluded(segs)

    # ---- swept queries (rt_tracer_sphere_cast / _device) ---------------------------------------------------------------

    def SphereCast(self, sweeps):
        """A moving sphere's first contact (rt_tracer_sphere_cast).  sweeps: (n, 8) float32 {origin, direction (used as given),
        radius, tmax}: the centre runs along o + t*d for 0 <= t <= tmax.  The answer's t is the time of first contact, u, v the
        barycentrics of the contact point on the winning triangle (0, 0 for a sphere), prim PRIM_NONE where nothing is touched;
        a reported contact is within RT_SWEEP_SLACK * (max|c| + r) of touching.  A numpy array -> HIT_DTYPE array, on return.
        A contiguous torch float32 tensor on the tracer's device -> (n, 4) float32 tensor {t, u, v, bits of prim}, enqueued on
        torch.cuda.current_stream() without a host synchronisation."""
        if type(sweeps).__module__.startswith("torch"):
            return self._sphere_cast_tensor(sweeps)
        s = self._segs_array("SphereCast", sweeps)
        hits = np.zeros(s.shape[0], HIT_DTYPE)
        self._check(self._lib.rt_tracer_sphere_cast(self._h, s.ctypes.data, s.shape[0], hits.ctypes.data))
        return hits

    def _sphere_cast_tensor(self, sweeps):
        import torch
        _, stream = self._segs_tensor("SphereCast", sweeps)
        hits = torch.empty((sweeps.shape[0], 4), dtype=torch.float32, device=sweeps.device)
        self._check(self._lib.rt_tracer_sphere_cast_device(self._h, sweeps.data_ptr(), sweeps.shape[0], hits.data_ptr(), stream))
        return hits

    def SphereCastContacts(self, sweeps, hits):
        """Where the contacts of a SphereCast call are (host numpy): the sphere's centre at contact c = o + t*d (fp32, the
        product, then the sum), the contact position on the surface (ClosestPositions' arithmetic at c) and the unit normal
        (centre - position) / |centre - position| pointing from the surface to the sphere, each (n, 3) float32; NaN where
        hits["prim"] is PRIM_NONE (and a NaN normal where centre and position coincide)."""
        s = self._segs_array("SphereCastContacts", sweeps)
        h = np.asarray(hits).reshape(-1)
        if h.dtype != HIT_DTYPE or h.shape[0] != s.shape[0]:
            raise ValueError("SphereCastContacts: expected the sweeps and the HIT_DTYPE answers of one SphereCast call")
        with np.errstate(all="ignore"):
            centre = s[:, 0:3] + h["t"][:, None] * s[:, 3:6]
            centre[h["prim"] < 0] = np.nan
            position = self.ClosestPositions(centre, h)
            w = centre - position
            normal = w / np.sqrt((w * w).sum(axis=1, dtype=np.float32))[:, None]
        return centre, position, normal

    def Clearance(self, a, b, radius):
        """Does a sphere of `radius` (a scalar or one per pair) fit along the segment from a[i] to b[i] ((n, 3) each)?  True
        where SphereCast of o = a, d = b - a (fp32, on the host), tmax = 1 reports no contact: the swept counterpart of Visible."""
        a = np.asarray(a, np.float32).reshape(-1, 3)
        b = np.asarray(b, np.float32).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError("Clearance: %d start points, %d end points" % (a.shape[0], b.shape[0]))
        sweeps = np.empty((a.shape[0], 8), np.float32)
        sweeps[:, :3], sweeps[:, 3:6], sweeps[:, 6], sweeps[:, 7] = a, b - a, np.asarray(radius, np.float32), np.float32(1.0)
        return self.SphereCast(sweeps)["prim"] < 0

    # ---- proximity of triangles (rt_tracer_triangle_distance / _device) ----------------------------------------------------

    def TriangleDistance(self, triangles, max_distance=np.inf):
        """The nearest primitive of the scene to each query triangle (rt_tracer_triangle_distance).  triangles: (n, 3, 3) or
        (n, 9) float32 corners, searched within max_distance (squared on the host in fp32, as ClosestPoint does), or (n, 12)
        {P0 xyz, d2max, P1 xyz, -, P2 xyz, -} with each triangle's SQUARED search radius in column 3 (+inf = unbounded).  ->
        (hits, witness): hits as ClosestPoint's (t the squared distance, u, v on the scene's record, prim or PRIM_NONE); witness
        the winning point on the query triangle and the index of the candidate that produced it (-1: none).  (t, u, v) is
        ClosestPoint's answer for the point witness.xyz on that prim, bit for bit.  A query with a non-finite coordinate accepts
        nothing.  numpy in -> (HIT_DTYPE (n,), WITNESS_DTYPE (n,)), on return.  A contiguous (n, 12) float32 torch tensor on the
        tracer's device -> two (n, 4) float32 tensors {t, u, v, prim bits}, {x, y, z, where bits}, enqueued on
        torch.cuda.current_stream() without a host synchronisation."""
        if type(triangles).__module__.startswith("torch"):
            return self._triangle_distance_tensor(triangles)
        t = self._distance_triangles("TriangleDistance", triangles, max_distance)
        hits = np.zeros(t.shape[0], HIT_DTYPE)
        witness = np.zeros(t.shape[0], WITNESS_DTYPE)
        self._check(self._lib.rt_tracer_triangle_distance(self._h, t.ctypes.data, t.shape[0], hits.ctypes.data, witness.ctypes.data))
        return hits, witness

    @staticmethod
    def _distance_triangles(who, triangles, max_distance):
        """_triangles_array, with _d2max(max_distance) in column 3 of triangles that came without a radius."""
        had_radius = np.ndim(triangles) >= 1 and np.shape(triangles)[-1] == 12
        t = RayTracer._triangles_array(who, triangles)
        if not had_radius:
            t[:, 3] = RayTracer._d2max(max_distance)
        return t

    def _triangle_distance_tensor(self, triangles):
        import torch
        if triangles.dtype != torch.float32 or triangles.dim() != 2 or triangles.shape[1] != 12 or not triangles.is_contiguous():
            raise ValueError("TriangleDistance: expected a contiguous (n, 12) float32 tensor")
        stream = self._stream_of("TriangleDistance", "triangles", triangles)
        n = triangles.shape[0]
        hits = torch.empty((n, 4), dtype=torch.float32, device=triangles.device)
        witness = torch.empty((n, 4), dtype=torch.float32, device=triangles.device)
        self._check(self._lib.rt_tracer_triangle_distance_device(self._h, triangles.data_ptr(), n, hits.data_ptr(), witness.data_ptr(), stream))
        return hits, witness

    def TriangleDistancePositions(self, hits, witness):
        """Both ends of TriangleDistance's answers (host numpy), each (n, 3) float32: the point on the query triangle (the
        witness) and the point on the scene (ClosestPositions at the witness); NaN where hits["prim"] is PRIM_NONE."""
        h = np.asarray(hits).reshape(-1)
        w = np.asarray(witness).reshape(-1)
        if h.dtype != HIT_DTYPE or w.dtype != WITNESS_DTYPE or h.shape != w.shape:
            raise ValueError("TriangleDistancePositions: expected the HIT_DTYPE and WITNESS_DTYPE answers of one TriangleDistance call")
        on_query = np.stack([w["x"], w["y"], w["z"]], axis=1).astype(np.float32)
        on_query[h["prim"] < 0] = np.nan
        return on_query, self.ClosestPositions(on_query, h)

    def MeshDistance(self, triangles, max_distance=np.inf):
        """The nearest pair between a whole query mesh and the scene, numpy only: TriangleDistance of every triangle, the
        smallest (t, query index) wins.  -> dict(distance (sqrt of t, float), query (the triangle's index), prim, on_query,
        on_scene ((3,) float32 each)), or None when nothing lies within max_distance."""
        hits, witness = self.TriangleDistance(triangles, max_distance)
        ok = np.nonzero(hits["prim"] >= 0)[0]
        if ok.size == 0:
            return None
        i = int(ok[np.argmin(hits["t"][ok])])                              # (argmin: the first of the smallest)
        a, b = self.TriangleDistancePositions(hits[i:i + 1], witness[i:i + 1])
        return {"distance": float(np.sqrt(np.float64(hits["t"][i]))), "query": i, "prim": int(hits["prim"][i]), "on_query": a[0], "on_scene": b[0]}

    def SetQueryAcceleration(self, mode):
        """How Intersect / Pick / FocusAt find their hits: QUERY_SCAN (0 / False, the default: every ray scans every triangle)
        or QUERY_BVH (1 / True: a bounding volume hierarchy over the uploaded scene, built by the next query).  Same answer
        for every ray whose scan winner is well conditioned (include/rt_mi355x.h, "ray queries")."""
        self._check(self._lib.rt_tracer_set_query_accel(self._h, int(mode)))

    def QueryAccelInfo(self):
        """rt_tracer_query_accel_info as a dict: mode, valid, nodes, leaves, depth, always_tested, build_us, device_bytes."""
        out = (C.c_uint64 * 8)()
        self._check(self._lib.rt_tracer_query_accel_info(self._h, out))
        return dict(zip(_ACCEL_KEYS, (int(x) for x in out)))

    def SetQueryAccelUpdate(self, policy):
        """What an upload does to the tree of QUERY_BVH: ACCEL_REBUILD (0, the default: the next query builds a new one on the
        host) or ACCEL_REFIT (1: an upload of the same number of triangles keeps the tree's topology and the next query refits
        its boxes on the device).  The answers obey the same contracts either way."""
        self._check(self._lib.rt_tracer_set_query_accel_update(self._h, int(policy)))

    def RebuildQueryAccel(self):
        """Drops the tree: the next QUERY_BVH query builds afresh, whatever the policy."""
        self._check(self._lib.rt_tracer_query_accel_rebuild(self._h))

    def QueryAccelUpdateInfo(self):
        """rt_tracer_query_accel_update_info as a dict: policy, refits (since the last build), fallbacks (refits that became
        builds), refit_us (device time of the last refit), cost and cost_built (floats: the tree's cost now and at its build),
        stack_entries (per lane, what the walks of the valid tree run with: 3 x depth unless DebugQueryStackCap lowered it)."""
        out = (C.c_uint64 * 8)()
        self._check(self._lib.rt_tracer_query_accel_update_info(self._h, out))
        cost = np.array([out[4], out[5]], np.uint64).view(np.float64)
        return {"policy": int(out[0]), "refits": int(out[1]), "fallbacks": int(out[2]), "refit_us": int(out[3]),
                "cost": float(cost[0]), "cost_built": float(cost[1]), "stack_entries": int(out[6])}

    def query_tree(self):
        """rt_dbg_query_tree_read: the device tree the queries walk now -> (nodes, records, info) as bvh_build returns them."""
        info = (C.c_uint64 * 8)()
        self._check(self._lib.rt_dbg_query_tree_read(self._h, None, 0, None, 0, info))
        nodes = np.zeros(int(info[2]), BVH_NODE_DTYPE)
        recs = np.zeros((int(info[7]) - nodes.nbytes) // BVH_RECORD_DTYPE.itemsize, BVH_RECORD_DTYPE)
        self._check(self._lib.rt_dbg_query_tree_read(self._h, nodes.ctypes.data, max(nodes.nbytes, 1), recs.ctypes.data,
                                                     max(recs.nbytes, 1), info))
        return nodes, recs, _tree_info(info)

    def DebugQueryAccelSlack(self, slack_milli):
        self._check(self._lib.rt_dbg_query_accel_slack(self._h, int(slack_milli)))

    def DebugQueryStackCap(self, cap=None):
        """rt_dbg_query_stack_cap (test-only): the following QUERY_BVH walks run with at most `cap` stack entries per lane --
        a lane that wants more answers from every leaf record, under the same contract.  None restores the product."""
        self._check(self._lib.rt_dbg_query_stack_cap(self._h, 0xFFFFFFFF if cap is None else int(cap)))

    def DebugGetRay(self, pixels, states):
        pix = np.ascontiguousarray(pixels, np.uint32).reshape(-1, 2)
        st = np.ascontiguousarray(states, np.uint32).reshape(-1, 6).copy()
        rays = np.zeros((pix.shape[0], 6), np.float32)
        self._check(self._lib.rt_dbg_get_ray(self._h, pix.shape[0], _u32p(pix), _u32p(st), _f32p(rays)))
        return rays, st

    def close(self):
        if self._h:
            self._lib.rt_tracer_destroy(self._h)
            self._h = C.c_void_p()
            self._retired.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- internals -------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise RtError("librt_mi355x error %d: %s" % (rc, self.LastError()))

    def _set_cb(self, key, callback, setter):
        # The render thread snapshots the callback per launch and may still hold the previous thunk (the
        # pipelined update hand-off keeps it across the next launch): a replaced thunk is retired, not freed,
        # until no render thread can be running (Wait(), close()).
        old = self._cbs.get(key)
        if old is not None:
            self._retired.append(old)
        if callback is None:
            self._cbs[key] = CALLBACK()
            setter(self._h, self._cbs[key], None)
            return

        me = weakref.ref(self)                 # no cycle self -> _cbs -> thunk -> closure -> self: a tracer that is dropped
                                               # without close() is still freed by its reference count

        def tramp(ptr, size, _user):
            n = size // 4
            img = np.ctypeslib.as_array(ptr, shape=(n,))
            owner = me()
            rows, width = (owner.rows, owner.width) if owner is not None else (0, 0)   # read per call: Resize changes them
            callback(img.reshape(rows, width) if n == rows * width and n else img, size)
        self._cbs[key] = CALLBACK(tramp)       # keep alive
        setter(self._h, self._cbs[key], None)


# ---- single-function device harnesses (parity tests) ------------------------------------
def dbg_hit_triangle(rays, tris, math_mode=MATH_FMA, eps_mode=0, device=0):
    L = load_library()
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = r.shape[0]
    hit = np.zeros(n, np.int32)
    tuv, nrm, pt = (np.zeros((n, 3), np.float32) for _ in range(3))
    rc = L.rt_dbg_hit_triangle(device, math_mode, n, _f32p(r), _f32p(t), eps_mode,
                               hit.ctypes.data_as(C.POINTER(C.c_int32)), _f32p(tuv), _f32p(nrm), _f32p(pt))
    if rc != 0:
        raise RtError("rt_dbg_hit_triangle failed (%d): %s" % (rc, L.rt_last_error().decode()))
    return hit.astype(bool), tuv, nrm, pt


def dbg_sincos(x, device=0):
    L = load_library()
    a = np.ascontiguousarray(x, np.float32).ravel()
    s, c = np.zeros_like(a), np.zeros_like(a)
    rc = L.rt_dbg_sincos(device, a.size, _f32p(a), _f32p(s), _f32p(c))
    if rc != 0:
        raise RtError("rt_dbg_sincos failed (%d): %s" % (rc, L.rt_last_error().decode()))
    return s, c


def dbg_valu_peak(device=0):
    """(attainable lane-FMA per second, shader clock GHz) measured on `device`."""
    L = load_library()
    r, g = C.c_double(), C.c_double()
    rc = L.rt_dbg_valu_peak(device, C.byref(r), C.byref(g))
    if rc != 0:
        raise RtError("rt_dbg_valu_peak failed (%d): %s" % (rc, L.rt_last_error().decode()))
    return r.value, g.value


def dbg_check_midrange(device=0):
    """Exhaustive device check of normalize's mid-range sqrt/reciprocal fast paths:
    (values checked, sqrt mismatches, reciprocal mismatches, a mismatching operand's bits or 0)."""
    L = load_library()
    out = (C.c_uint64 * 4)()
    L.rt_dbg_check_midrange.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    rc = L.rt_dbg_check_midrange(device, out)
    if rc != 0:
        raise RtError("rt_dbg_check_midrange failed (%d): %s" % (rc, L.rt_last_error().decode()))
    return tuple(int(x) for x in out)


def dbg_uniform(states, m, device=0):
    L = load_library()
    st = np.ascontiguousarray(states, np.uint32).reshape(-1, 6).copy()
    out = np.zeros((st.shape[0], m), np.float32)
    rc = L.rt_dbg_uniform(device, st.shape[0], m, _u32p(st), _f32p(out))
    if rc != 0:
        raise RtError("rt_dbg_uniform failed (%d): %s" % (rc, L.rt_last_error().decode()))
    return out, st


def dbg_rng_init_host(seed, subsequence):
    s = np.zeros(6, np.uint32)
    load_library().rt_dbg_rng_init_host(int(seed), int(subsequence), _u32p(s))
    return s


def dbg_rng_advance_host(state, n, use_table):
    """v0..v4 -- one state (5,) or several (k, 5) -- advanced by n draws on the host: with the window table of T^n, or by n
    steps (rt_dbg_rng_advance_host, _n)."""
    s = np.ascontiguousarray(state, np.uint32).copy()
    L = load_library()
    if s.ndim == 1:
        L.rt_dbg_rng_advance_host(_u32p(s.reshape(5)), int(n), int(bool(use_table)))
    else:
        L.rt_dbg_rng_advance_host_n(_u32p(s.reshape(-1, 5)), s.reshape(-1, 5).shape[0], int(n), int(bool(use_table)))
    return s
