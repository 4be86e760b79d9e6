"""The option matrix of the dense-scene kernels (4 096 ... 50 000 triangles), checked against the oracle by
tests/test_gpu_dense_options.py; tests/test_dense_cases.py checks on the CPU that the table below stays a valid cover.

Dense scenes run kernels of their own (rt_tracer.hpp: trace_path): per-wave candidate lists in HBM built by wave_lists_kernel
(DenseLists), or the classification inside the trace kernel (ClassifyForms, and Classify without the per-sample forms), behind
the macro and super-tile binning.  Every case renders one frame with one combination of

  math     RT_MATH_FMA | RT_MATH_STRICT
  hit      the reference's farthest hit | nearest_hit
  extras   none | spheres | smooth normals (edge-layout scene) | spheres + smooth normals
  path     dense      DenseLists, the default
           overflow   DenseLists with 32-entry lists (bin_list=32): overflowed tiles test by triangle index (hbm_overflow)
           forms      ClassifyForms (no_macro_bins)
           nofilter   Classify, unfiltered kernel (no_filter)
           nopretest  Classify, filtered kernel (RT_MI355X_NO_PRETEST=1)
  shape    unsplit    < 128 rows: one kernel
           split      1152 x 144: two half-frame kernels, each half with 9 x 2 macro tiles (> 16: super tiles)
           band       136 rows of a 300-row frame from row 83 (not a multiple of 8): a band that splits
  spp      1 (K = 1) | 3 (K = 2, a partial pass) | 7 (K = 4, a partial pass)
  iters    one        TraceEnqueue(1, spp): one launch
           fused      several iterations in one launch: Trace(n, spp, 0) (unsplit), TraceEnqueue(n, spp) (split frames)
           cadence    launches cut at update points: Trace(n, spp, 1) with an update callback (unsplit), one Launch per
                      iteration (split frames)

and compares all four buffers with the oracle's bit for bit.  CASES covers every pair of axis values at least once (an
all-pairs covering array) except the pairs in INFEASIBLE, and holds the ANCHORS below."""
import itertools

import numpy as np

AXES = {
    "math": ("fma", "strict"),
    "hit": ("far", "near"),
    "extras": ("none", "spheres", "smooth", "spheres+smooth"),
    "path": ("dense", "overflow", "forms", "nofilter", "nopretest"),
    "shape": ("unsplit", "split", "band"),
    "spp": (1, 3, 7),
    "iters": ("one", "fused", "cadence"),
}
# unfiltered kernels never fuse iterations (rt_kernels.hip: trace_can_fuse)
INFEASIBLE = {frozenset({("path", "nofilter"), ("iters", "fused")})}

# (W, rows, full_height, row_begin) of the tracer; the oracle renders the same band
SHAPES = {"unsplit": (128, 48, 0, 0), "split": (1152, 144, 0, 0), "band": (192, 136, 300, 83)}
CAMERA = dict(angles=(0.1, -0.05), fov=70.0, focal=3.0, aperture=0.05)
# behind the triangle cloud (z in [-12.15, -3.85]): the farthest hit wherever it is seen; in front of it: the nearest hit
# there; off to the side (55 degrees left), in tiles of the wide frames that no triangle reaches: their lists are empty
SPHERES = np.array([[0.0, 0.0, -30.0, 8.0], [0.6, 0.2, -3.5, 0.5], [-8.2, 0.0, -5.7, 1.2]], np.float32)
LIST_CAP = {"dense": 84, "overflow": 32}             # RT_PRETEST_LIST; the forced bin_list

_C = ("name", "math", "hit", "extras", "path", "shape", "spp", "iters", "n_tris", "extra")
CASES = [dict(zip(_C, row)) for row in (
    # anchors (ANCHORS) first, then the cases that complete the cover
    ("a1_strict_dense_split_spp7_rebuilt", "strict", "near", "spheres+smooth", "dense", "split", 7, "one", 4096, {"reuse": False}),
    ("a2_strict_dense_fused_spp1", "strict", "far", "smooth", "dense", "unsplit", 1, "fused", 6000, {"n": 20}),
    ("a3_spheres_far_fma", "fma", "far", "spheres", "dense", "band", 3, "cadence", 5000, {}),
    ("a3_spheres_near_fma", "fma", "near", "spheres", "dense", "unsplit", 1, "one", 9000, {}),
    ("a3_spheres_far_strict", "strict", "far", "spheres", "dense", "band", 7, "fused", 4096, {}),
    ("a3_spheres_near_strict", "strict", "near", "spheres", "dense", "unsplit", 3, "cadence", 6000, {}),
    ("a4_smooth_far", "fma", "far", "smooth", "dense", "split", 3, "one", 4096, {}),
    ("a4_smooth_near", "fma", "near", "smooth", "dense", "band", 7, "cadence", 4096, {}),
    ("a4_spheres_smooth_far", "fma", "far", "spheres+smooth", "dense", "band", 1, "cadence", 6000, {}),
    ("a4_spheres_smooth_near", "fma", "near", "spheres+smooth", "dense", "unsplit", 3, "fused", 9000, {}),
    ("a5_overflow_everything", "strict", "near", "spheres+smooth", "overflow", "unsplit", 7, "cadence", 9000, {}),
    ("a6_forms_fused_strict_near_spheres", "strict", "near", "spheres", "forms", "split", 1, "fused", 4096, {}),
    ("a7_strict_dense_band", "strict", "far", "none", "dense", "band", 3, "one", 5000, {}),
    ("nopretest_cadence", "fma", "near", "none", "nopretest", "unsplit", 1, "cadence", 5000, {}),
    ("overflow_band_fused", "fma", "far", "none", "overflow", "band", 7, "fused", 4096, {}),
    ("forms_band_cadence", "fma", "far", "none", "forms", "band", 3, "cadence", 5000, {}),
    ("nofilter_split_strict", "strict", "far", "none", "nofilter", "split", 1, "cadence", 4096, {}),
    ("forms_smooth_near", "fma", "near", "smooth", "forms", "unsplit", 7, "one", 6000, {}),
    ("nofilter_smooth_near", "fma", "near", "smooth", "nofilter", "unsplit", 7, "one", 9000, {}),
    ("nopretest_smooth_band", "strict", "far", "smooth", "nopretest", "band", 7, "one", 4096, {}),
    ("overflow_smooth_split", "strict", "far", "smooth", "overflow", "split", 1, "one", 4096, {}),
    ("nofilter_spheres_band", "strict", "near", "spheres", "nofilter", "band", 3, "one", 5000, {}),
    ("nopretest_spheres_fused", "strict", "near", "spheres", "nopretest", "unsplit", 3, "fused", 6000, {}),
    ("overflow_spheres_band", "strict", "far", "spheres", "overflow", "band", 3, "fused", 5000, {}),
    ("forms_spheres_smooth_band", "strict", "far", "spheres+smooth", "forms", "band", 1, "fused", 6000, {}),
    ("nofilter_spheres_smooth_cadence", "strict", "far", "spheres+smooth", "nofilter", "unsplit", 1, "cadence", 4096, {}),
    ("nopretest_spheres_smooth_split", "fma", "near", "spheres+smooth", "nopretest", "split", 1, "one", 4096, {}),
    # beyond the cover: fused iterations in split launches of the default kernel, and a forced samples_in_flight
    ("dense_split_fused", "fma", "far", "none", "dense", "split", 1, "fused", 4096, {}),
    ("dense_forced_k2", "strict", "near", "none", "dense", "unsplit", 7, "one", 5000, {"k": 2}),
)]

ANCHORS = {
    "1 strict DenseLists, split with super tiles, spp 7, lists rebuilt":
        lambda c: c["math"] == "strict" and c["path"] == "dense" and c["shape"] == "split" and c["spp"] == 7 and c["extra"].get("reuse") is False,
    "2 strict fused DenseLists at spp 1":
        lambda c: c["math"] == "strict" and c["path"] == "dense" and c["iters"] == "fused" and c["spp"] == 1,
    "3 spheres on DenseLists, fma / far": lambda c: c["path"] == "dense" and c["extras"] == "spheres" and (c["math"], c["hit"]) == ("fma", "far"),
    "3 spheres on DenseLists, fma / near": lambda c: c["path"] == "dense" and c["extras"] == "spheres" and (c["math"], c["hit"]) == ("fma", "near"),
    "3 spheres on DenseLists, strict / far": lambda c: c["path"] == "dense" and c["extras"] == "spheres" and (c["math"], c["hit"]) == ("strict", "far"),
    "3 spheres on DenseLists, strict / near": lambda c: c["path"] == "dense" and c["extras"] == "spheres" and (c["math"], c["hit"]) == ("strict", "near"),
    "4 smooth DenseLists, far": lambda c: c["path"] == "dense" and c["extras"] == "smooth" and c["hit"] == "far",
    "4 smooth DenseLists, near": lambda c: c["path"] == "dense" and c["extras"] == "smooth" and c["hit"] == "near",
    "4 smooth DenseLists with spheres, far": lambda c: c["path"] == "dense" and c["extras"] == "spheres+smooth" and c["hit"] == "far",
    "4 smooth DenseLists with spheres, near": lambda c: c["path"] == "dense" and c["extras"] == "spheres+smooth" and c["hit"] == "near",
    "5 overflow with spheres, smooth, nearest, strict":
        lambda c: c["path"] == "overflow" and c["extras"] == "spheres+smooth" and c["hit"] == "near" and c["math"] == "strict",
    "6 fused ClassifyForms, strict, nearest, spheres":
        lambda c: c["path"] == "forms" and c["iters"] == "fused" and c["math"] == "strict" and c["hit"] == "near" and "spheres" in c["extras"],
    "7 strict dense row band that splits":
        lambda c: c["math"] == "strict" and c["path"] == "dense" and c["shape"] == "band",
    "forced samples_in_flight": lambda c: "k" in c["extra"],
}


def pairs_of(case):
    names = list(AXES)
    return {frozenset({(a, case[a]), (b, case[b])}) for a, b in itertools.combinations(names, 2)}


def required_pairs():
    names = list(AXES)
    return {frozenset({(a, x), (b, y)}) for a, b in itertools.combinations(names, 2)
            for x in AXES[a] for y in AXES[b]} - INFEASIBLE


def split_row(rows):
    """first row of the lower half of a split launch (rt_tracer.hpp: split_row); 0 = one kernel"""
    return ((rows // 2 + 7) // 8) * 8 if rows >= 128 else 0


def halves(case):
    """row counts of the kernels one launch of the case runs (Trace() launches are never split)"""
    rows = SHAPES[case["shape"]][1]
    r0 = split_row(rows) if case["shape"] != "unsplit" else 0      # (the split shapes launch through TraceEnqueue / Launch)
    return [r0, rows - r0] if r0 else [rows]


def samples_in_flight(case):
    """K (rt_tracer.hpp: pick_k): forced, or 4 samples per pass for scenes of more than 128 triangles, fewer at low spp"""
    if "k" in case["extra"]:
        return case["extra"]["k"]
    return 4 if case["spp"] >= 4 else 2 if case["spp"] >= 2 else 1


def lds_bytes(case):
    """rt_tracer_info's lds_bytes (rt_kernels.hip: trace_lds_bytes with rt_tracer.hpp: params); DenseLists reports the
    ClassifyForms figure"""
    if case["path"] in ("dense", "overflow", "forms"):
        return 4 * LIST_CAP.get(case["path"], 84) * 104 + 448 * 4 + 160
    return 4 * 192 * 40 + 1024 * 4 + 160


def iterations(case):
    if case["iters"] == "one":
        return 1
    if "n" in case["extra"]:
        return case["extra"]["n"]
    return 2 if case["shape"] != "unsplit" else 3


def scene(case, seed):
    """(rows, edge layout?) of the case's scene: random triangles in the vertex layout, or with packed vertex normals"""
    from raytracertest_amd import meshes, scenes
    tris = scenes.random_triangles(case["n_tris"], seed)
    if "smooth" not in case["extras"]:
        return tris, False
    nrm = np.random.default_rng(seed).normal(size=(tris.shape[0], 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return meshes.to_edge_format(tris, normals=nrm), True
