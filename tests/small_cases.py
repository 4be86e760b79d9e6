"""The option matrix of the small-scene kernels (TracePath::SmallLists: scenes of up to 256 triangles, bench.py's headline C3),
checked against the oracle by tests/test_gpu_small_options.py; tests/test_small_cases.py checks on the CPU that the table below
stays a valid cover and that the frames and scenes are what the cases are named after.  A helper, not a test.

Small scenes trace from per-tile candidate lists that one of four builder kernels writes ahead of the launch
(rt_kernels.hip: launch_tile_lists), and tiles whose rays all see one triangle -- certain winners, 70 % of C3 -- are not traced
at all.  Every case renders one frame with one combination of

  math     RT_MATH_FMA | RT_MATH_STRICT
  hit      the reference's farthest hit | nearest_hit
  extras   none | spheres | smooth normals (edge-layout scene) | spheres + smooth normals
  builder  pair       region_pair_lists_kernel: up to 32 triangles, tile_curv > 0
           region     region_lists_kernel: 33 .. 256 triangles, tile_curv > 0
           tile32     tile_lists_kernel<., 32>: up to 32 triangles, tile_curv <= 0
           tile64     tile_lists_kernel<., 64>: 33 .. 256 triangles, tile_curv <= 0
           (tile_curv > 0 is granted by rt_tracer.hpp: tile_corner_bound where a = 14 tan(fov / 2) / H_full <= 0.1; the frames
           below keep a <= 0.08 or a >= 0.125)
  kernel   filtered   the default trace kernel
           unfiltered no_filter
           scan       no_binning: TracePath::FullScan, no lists and no builder (the case's builder is None)
  winners  table      certain-winner tiles take their pixels' words from the per-triangle table (the default)
           per_pixel  RT_MI355X_NO_SURE_TABLE=1: they accumulate per pixel
           no_owe     RT_MI355X_NO_OWE=1: they advance their RNG states in every launch
           traced     RT_FLAG_NO_SURE_HIT (no_sure_hit): the kernel traces them like every other tile
  shape    unsplit    < 128 rows: one kernel
           rows       >= 128 rows, RT_MI355X_ROW_INTERLEAVE=0: the upper and the lower rows on two streams
           interleaved  the same frames, RT_MI355X_ROW_INTERLEAVE=1: the even and the odd block rows
           band       136 rows of a taller frame from a row that is no multiple of 8: a band that splits
           ragged     236 x 134: a split frame whose width is no multiple of 32 (nor of 8) and whose rows are no multiple of 8
           (band and ragged: extra["interleave"] pins the halves where a case has it, the library chooses otherwise)
  spp      1 (K = 1) | 3 (K = 2, a partial pass) | 7 (K = 2 up to 128 triangles, K = 4 above: a partial pass either way)
  iters    one        TraceEnqueue(1, spp): one launch
           fused      several iterations in one launch: Trace(n, spp, 0) (unsplit), TraceEnqueue(n, spp) (split frames)
           cadence    launches cut at update points: Trace(n, spp, 1) with an update callback (unsplit), one Launch per
                      iteration (split frames)
           steps      TraceEnqueueN(1, spp, n_steps): bench.py's pattern; the steps after the first owe their RNG draws
  reuse    kept | rebuilt (SetListReuse(False): the first launch of every Trace builds its lists)

and compares all four buffers with the oracle's bit for bit.  CASES covers every pair of axis values at least once (an
all-pairs covering array, completed greedily) except the pairs in INFEASIBLE; its hot sub-table (hot()) alone covers every pair
among builder x shape x spp x iters x reuse and every math x builder; and it holds the ANCHORS below."""
import itertools

import numpy as np

AXES = {
    "math": ("fma", "strict"),
    "hit": ("far", "near"),
    "extras": ("none", "spheres", "smooth", "spheres+smooth"),
    "builder": ("pair", "region", "tile32", "tile64"),
    "kernel": ("filtered", "unfiltered", "scan"),
    "winners": ("table", "per_pixel", "no_owe", "traced"),
    "shape": ("unsplit", "rows", "interleaved", "band", "ragged"),
    "spp": (1, 3, 7),
    "iters": ("one", "fused", "cadence", "steps"),
    "reuse": ("kept", "rebuilt"),
}
HOT_AXES = ("builder", "shape", "spp", "iters", "reuse")


def _infeasible():
    out = set()
    # what the library refuses: unfiltered kernels and the full scan never fuse iterations (rt_kernels.hip:340, trace_can_fuse;
    # launch_trace, :429), and only SmallLists launches take interleaved halves (rt_kernels.hip:430: row_il off SmallLists)
    for k in ("unfiltered", "scan"):
        out.add(frozenset({("kernel", k), ("iters", "fused")}))
    out.add(frozenset({("kernel", "scan"), ("shape", "interleaved")}))
    # what makes an axis vacuous: the full scan has no lists, so no builder (rt_tracer.hpp: prepare_tile_lists) ...
    for b in AXES["builder"]:
        out.add(frozenset({("kernel", "scan"), ("builder", b)}))
    # ... and nearest hit, spheres and smooth normals have no certain winners for the switches to act on (rt_tracer.hpp:665,
    # owe_key_of's sure_ok; rt_trace.hpp:224)
    for w in AXES["winners"][1:]:
        out.add(frozenset({("winners", w), ("hit", "near")}))
        for e in AXES["extras"][1:]:
            out.add(frozenset({("winners", w), ("extras", e)}))
    return out


INFEASIBLE = _infeasible()

# name -> W, rows, full height (0: the rows), first row, fov, camera angles.  Per shape one frame in which tile_corner_bound
# grants the corner path (side "region": a <= 0.08) and one in which it does not (side "tile": a >= 0.125).  Every camera is
# turned to the left so far that the frame shows what lies 65 degrees off the room's axis: background, the side extras and
# the side sphere (EXTRA_SIDE_DEG, SPHERES).
FRAMES = {
    ("unsplit", "region"): dict(W=160, rows=124, full_h=0, row_begin=0, fov=70.0, angles=(0.0, 0.49)),
    ("unsplit", "tile"): dict(W=128, rows=72, full_h=0, row_begin=0, fov=70.0, angles=(0.0, 0.31)),
    ("rows", "region"): dict(W=256, rows=144, full_h=0, row_begin=0, fov=70.0, angles=(0.0, 0.31)),
    ("rows", "tile"): dict(W=256, rows=128, full_h=0, row_begin=0, fov=100.0, angles=(0.0, 0.14)),
    ("band", "region"): dict(W=256, rows=136, full_h=300, row_begin=83, fov=100.0, angles=(0.0, 0.42)),
    ("band", "tile"): dict(W=192, rows=136, full_h=160, row_begin=13, fov=112.0, angles=(0.0, 0.16)),
    ("ragged", "region"): dict(W=236, rows=134, full_h=0, row_begin=0, fov=70.0, angles=(0.0, 0.31)),
    ("ragged", "tile"): dict(W=236, rows=134, full_h=0, row_begin=0, fov=102.0, angles=(0.0, 0.09)),
}
FRAMES["interleaved", "region"] = FRAMES["rows", "region"]
FRAMES["interleaved", "tile"] = FRAMES["rows", "tile"]
FOCAL, APERTURE = 3.0, 0.05                          # scenes.CONFIGS["C3"]
A_REGION_MAX, A_TILE_MIN = 0.08, 0.125               # the margin around tile_corner_bound's 0.1
# the room is x, y in [-1, 1], z in [-3, -1], open towards the camera at the origin (scenes.cornell32): a ray more than 45 degrees
# off -z in the horizontal plane passes outside it.  Behind the room: the farthest hit wherever it is seen; in front of the
# room's opening: the nearest hit there; 62.5 degrees off to the left at y = 0 (60 .. 65 degrees), where no triangle reaches.
SPHERES = np.array([[0.3, 0.0, -6.0, 1.2], [-0.15, 0.0, -0.8, 0.1], [-2.661, 0.0, -1.385, 0.13]], np.float32)
EXTRA_SIDE_DEG = (47.3, 50.0)                        # where the side extras lie, off -z towards -x
LENS = np.array([(0.0, 0.0)] + [(np.cos(a), np.sin(a)) for a in np.arange(8) * np.pi / 4], np.float32)   # the tile probe's lens points

_C = ("name", "math", "hit", "extras", "builder", "kernel", "winners", "shape", "spp", "iters", "reuse", "n_tris", "extra")
CASES = [dict(zip(_C, row)) for row in (
    # anchors (ANCHORS) first ...
    ("a1_bench_pair", "fma", "far", "none", "pair", "filtered", "table", "rows", 3, "steps", "rebuilt", 32, {}),
    ("a2_bench_region_n129", "fma", "far", "none", "region", "filtered", "table", "rows", 7, "steps", "rebuilt", 129, {}),
    ("a3_strict_tile64_interleaved_fused_spp7", "strict", "far", "none", "tile64", "filtered", "table", "interleaved", 7, "fused", "kept", 128, {}),
    ("a4_smooth_region_band_cadence", "fma", "far", "smooth", "region", "filtered", "table", "band", 3, "cadence", "kept", 256, {}),
    ("a5_spheres_smooth_near_tile32_ragged", "strict", "near", "spheres+smooth", "tile32", "filtered", "table", "ragged", 1, "one", "kept", 32, {}),
    # ... then the hot sub-table: far, no extras, the filtered kernel, certain winners on ...
    ("h_tile32_unsplit_no_owe_cadence", "strict", "far", "none", "tile32", "filtered", "no_owe", "unsplit", 1, "cadence", "rebuilt", 5, {}),
    ("h_pair_band_per_pixel", "strict", "far", "none", "pair", "filtered", "per_pixel", "band", 1, "one", "kept", 32, {"interleave": 1}),
    ("h_tile64_ragged_no_owe_cadence", "fma", "far", "none", "tile64", "filtered", "no_owe", "ragged", 3, "cadence", "kept", 33, {"interleave": 1}),
    ("h_region_interleaved_no_owe", "strict", "far", "none", "region", "filtered", "no_owe", "interleaved", 3, "one", "rebuilt", 128, {}),
    ("h_tile32_rows_per_pixel_fused", "fma", "far", "none", "tile32", "filtered", "per_pixel", "rows", 1, "fused", "kept", 32, {}),
    ("h_pair_ragged_no_owe_fused_spp7", "strict", "far", "none", "pair", "filtered", "no_owe", "ragged", 7, "fused", "rebuilt", 5, {"interleave": 0}),
    ("h_region_unsplit_per_pixel_fused", "fma", "far", "none", "region", "filtered", "per_pixel", "unsplit", 3, "fused", "kept", 256, {}),
    ("h_tile64_band_per_pixel_steps", "fma", "far", "none", "tile64", "filtered", "per_pixel", "band", 1, "steps", "rebuilt", 129, {}),
    ("h_tile32_interleaved_no_owe_steps", "strict", "far", "none", "tile32", "filtered", "no_owe", "interleaved", 3, "steps", "kept", 32, {}),
    ("h_tile32_band_per_pixel_cadence_spp7", "fma", "far", "none", "tile32", "filtered", "per_pixel", "band", 7, "cadence", "kept", 5, {"interleave": 0}),
    ("h_tile64_unsplit_no_owe_spp7_n129", "fma", "far", "none", "tile64", "filtered", "no_owe", "unsplit", 7, "one", "kept", 129, {}),
    ("h_pair_interleaved_cadence", "fma", "far", "none", "pair", "filtered", "table", "interleaved", 1, "cadence", "rebuilt", 32, {}),
    ("h_region_ragged_no_owe_steps", "fma", "far", "none", "region", "filtered", "no_owe", "ragged", 1, "steps", "rebuilt", 33, {}),
    ("h_region_band_per_pixel_fused", "strict", "far", "none", "region", "filtered", "per_pixel", "band", 3, "fused", "kept", 129, {}),
    ("h_tile32_ragged_per_pixel", "strict", "far", "none", "tile32", "filtered", "per_pixel", "ragged", 1, "one", "rebuilt", 32, {}),
    ("h_tile64_rows_no_owe", "strict", "far", "none", "tile64", "filtered", "no_owe", "rows", 1, "one", "kept", 256, {}),
    ("h_pair_unsplit_no_owe_steps", "fma", "far", "none", "pair", "filtered", "no_owe", "unsplit", 1, "steps", "kept", 5, {}),
    ("h_region_rows_no_owe_cadence", "strict", "far", "none", "region", "filtered", "no_owe", "rows", 1, "cadence", "rebuilt", 33, {}),
    # ... and the cases that complete the cover
    ("spheres_near_pair_unfiltered_steps", "fma", "near", "spheres", "pair", "unfiltered", "table", "rows", 3, "steps", "rebuilt", 32, {}),
    ("scan_spheres_smooth_near_cadence", "strict", "near", "spheres+smooth", None, "scan", "table", "unsplit", 7, "cadence", "rebuilt", 129, {"side": "region"}),
    ("traced_tile32_unfiltered_ragged", "fma", "far", "none", "tile32", "unfiltered", "traced", "ragged", 7, "cadence", "kept", 32, {}),
    ("spheres_region_unfiltered_band", "strict", "far", "spheres", "region", "unfiltered", "table", "band", 1, "one", "kept", 128, {"interleave": 1}),
    ("scan_traced_rows_steps", "strict", "far", "none", None, "scan", "traced", "rows", 1, "steps", "kept", 33, {"side": "tile"}),
    ("spheres_smooth_near_tile64_unfiltered_steps", "fma", "near", "spheres+smooth", "tile64", "unfiltered", "table", "interleaved", 3, "steps", "kept", 256, {}),
    ("smooth_near_region_unfiltered", "strict", "near", "smooth", "region", "unfiltered", "table", "unsplit", 1, "one", "rebuilt", 129, {}),
    ("scan_no_owe_band", "fma", "far", "none", None, "scan", "no_owe", "band", 3, "one", "kept", 256, {"side": "region"}),
    ("traced_pair_unfiltered", "strict", "far", "none", "pair", "unfiltered", "traced", "unsplit", 3, "one", "rebuilt", 32, {}),
    ("spheres_near_tile32_interleaved_cadence", "strict", "near", "spheres", "tile32", "filtered", "table", "interleaved", 7, "cadence", "kept", 5, {}),
    ("smooth_near_tile32_rows_fused", "fma", "near", "smooth", "tile32", "filtered", "table", "rows", 7, "fused", "rebuilt", 32, {}),
    ("scan_smooth_ragged_steps", "strict", "far", "smooth", None, "scan", "table", "ragged", 7, "steps", "rebuilt", 32, {"side": "tile"}),
    ("spheres_smooth_near_pair_band_fused", "fma", "near", "spheres+smooth", "pair", "filtered", "table", "band", 1, "fused", "rebuilt", 32, {}),
    ("traced_tile64_band_fused", "fma", "far", "none", "tile64", "filtered", "traced", "band", 1, "fused", "kept", 128, {}),
    ("spheres_smooth_region_unfiltered_cadence", "fma", "far", "spheres+smooth", "region", "unfiltered", "table", "rows", 3, "cadence", "rebuilt", 33, {}),
    ("spheres_near_tile64_ragged_fused", "fma", "near", "spheres", "tile64", "filtered", "table", "ragged", 1, "fused", "kept", 129, {}),
    ("scan_spheres_steps", "fma", "far", "spheres", None, "scan", "table", "unsplit", 7, "steps", "kept", 128, {"side": "tile"}),
    ("smooth_near_tile64_interleaved_fused", "strict", "near", "smooth", "tile64", "filtered", "table", "interleaved", 7, "fused", "kept", 129, {}),
    ("per_pixel_tile64_unfiltered_interleaved", "fma", "far", "none", "tile64", "unfiltered", "per_pixel", "interleaved", 3, "cadence", "kept", 33, {}),
    ("traced_region_interleaved_steps", "fma", "far", "none", "region", "filtered", "traced", "interleaved", 7, "steps", "rebuilt", 128, {}),
    ("scan_near_ragged_steps", "strict", "near", "none", None, "scan", "table", "ragged", 3, "steps", "rebuilt", 5, {"side": "region"}),
    ("scan_per_pixel_ragged", "fma", "far", "none", None, "scan", "per_pixel", "ragged", 1, "one", "kept", 256, {"side": "tile"}),
    ("no_owe_tile64_unfiltered_cadence", "strict", "far", "none", "tile64", "unfiltered", "no_owe", "unsplit", 1, "cadence", "kept", 256, {}),
    ("smooth_near_pair_ragged", "strict", "near", "smooth", "pair", "filtered", "table", "ragged", 7, "one", "rebuilt", 5, {}),
    # beyond the cover: samples_in_flight forced to 1 and to 4 (a partial pass of 3 at K = 4 on the 32-triangle builders' side of
    # pick_k), region's K = 2 side of 128 | 129 at spp 7, and five owing steps
    ("forced_k1_region_spp3_steps", "fma", "far", "none", "region", "filtered", "table", "unsplit", 3, "steps", "kept", 256, {"k": 1}),
    ("forced_k4_tile32_spp7", "strict", "far", "none", "tile32", "filtered", "table", "rows", 7, "one", "kept", 32, {"k": 4}),
    ("region_n128_spp7_steps5", "strict", "far", "none", "region", "filtered", "table", "ragged", 7, "steps", "kept", 128, {"n_steps": 5}),
)]

# The scene of 5 triangles: the back wall, the left wall and half of the tall box's camera side -- not the box's first five
# triangles, which are walls alone: every ray hits at most one of them and the hit rule could not change the frame.
FIVE = (0, 1, 2, 3, 22)
N_TRIS = {"pair": (5, 32), "tile32": (5, 32), "region": (33, 128, 129, 256), "tile64": (33, 128, 129, 256)}


def hot(case):
    """certain winners decide the cost of these: far, no extras, the filtered kernel, certain-winner tiles not traced"""
    return case["hit"] == "far" and case["extras"] == "none" and case["kernel"] == "filtered" and case["winners"] != "traced"


ANCHORS = {
    "the benchmark's combination in small": lambda c: tuple(c[a] for a in ("math", "hit", "extras", "builder", "kernel", "winners", "shape", "iters", "reuse"))
        == ("fma", "far", "none", "pair", "filtered", "table", "rows", "steps", "rebuilt"),
    "its region twin at 129 triangles": lambda c: tuple(c[a] for a in ("math", "hit", "extras", "builder", "kernel", "winners", "shape", "iters", "reuse", "n_tris"))
        == ("fma", "far", "none", "region", "filtered", "table", "rows", "steps", "rebuilt", 129),
    "strict tile64, interleaved, fused, spp 7": lambda c: (c["math"], c["builder"], c["shape"], c["iters"], c["spp"]) == ("strict", "tile64", "interleaved", "fused", 7),
    "smooth region band at a cadence": lambda c: (c["extras"], c["builder"], c["shape"], c["iters"]) == ("smooth", "region", "band", "cadence"),
    "spheres + smooth, nearest, tile32, ragged": lambda c: (c["extras"], c["hit"], c["builder"], c["shape"]) == ("spheres+smooth", "near", "tile32", "ragged"),
    "K = 2 with a remainder of 1 (128 triangles, spp 7)": lambda c: c["n_tris"] == 128 and c["spp"] == 7 and c["kernel"] != "scan" and "k" not in c["extra"],
    "K = 4 with a remainder of 3 (129 triangles, spp 7)": lambda c: c["n_tris"] == 129 and c["spp"] == 7 and c["kernel"] != "scan" and "k" not in c["extra"],
    "samples_in_flight forced to 1": lambda c: c["extra"].get("k") == 1,
    "samples_in_flight forced to 4": lambda c: c["extra"].get("k") == 4,
}
HOT_ANCHORS = [c["name"] for c in CASES[:3]]         # run again under every winners switch (test_gpu_small_options.py)


# ---------------------------------------------------------------------------------------------------------------- the cover
def pairs_of(case, axes=None):
    """the pairs of axis values the case holds (a scan case has no builder: None pairs with nothing)"""
    names = [a for a in (axes or AXES) if case[a] is not None]
    return {frozenset({(a, case[a]), (b, case[b])}) for a, b in itertools.combinations(names, 2)}


def all_pairs(axes):
    return {frozenset({(a, x), (b, y)}) for a, b in itertools.combinations(list(axes), 2) for x in AXES[a] for y in AXES[b]}


def required_pairs():
    return all_pairs(AXES) - INFEASIBLE


def hot_required_pairs():
    return all_pairs(HOT_AXES) | {frozenset({("math", m), ("builder", b)}) for m in AXES["math"] for b in AXES["builder"]}


# ---------------------------------------------------------------------------------------------------------------- frames
def side(case):
    """which of the shape's two frames: the one with tile_curv > 0 ("region") or the other ("tile")"""
    if case["builder"] is None:
        return case["extra"]["side"]
    return "region" if case["builder"] in ("pair", "region") else "tile"


def frame(case):
    return FRAMES[case["shape"], side(case)]


def builder_kind(case):
    """the index launch_tile_lists gives the case's builder (rt_dbg_list_builds), None for the scan"""
    return None if case["builder"] is None else AXES["builder"].index(case["builder"])


def corner_bound(f, M):
    """rt_tracer.hpp: tile_corner_bound in float64 for the frame f and the camera's 4 x 4 matrix M: (granted, a, lmax / lmin)"""
    m = np.asarray(M, np.float64).reshape(4, 4)[:3, :3]
    G = m @ m.T
    off = np.abs(G).sum(axis=1) - np.abs(np.diag(G))
    lmax, lmin = float((np.diag(G) + off).max()), float((np.diag(G) - off).min())
    if not (lmin > 0.25 and lmax < 4.0):
        return False, float("nan"), float("nan")
    W, H = f["W"], f["full_h"] or f["rows"]
    hh = float(np.tan(np.radians(np.float64(f["fov"])) / 2.0))
    a, b = 14.0 * hh * (W / H) / W, 14.0 * hh / H
    return 0.5 * (a * a + b * b) * (lmax / lmin) <= 0.1 * min(a, b), b, lmax / lmin


def split_row(rows):
    """first row of the lower half of a split launch (rt_tracer.hpp: split_row); 0 = one kernel"""
    return ((rows // 2 + 7) // 8) * 8 if rows >= 128 else 0


def interleave(case):
    """what RT_MI355X_ROW_INTERLEAVE is set to while the tracer is created, or None"""
    if case["shape"] in ("rows", "interleaved"):
        return int(case["shape"] == "interleaved")
    return case["extra"].get("interleave")


def teeth_rows(case):
    """(first row, 16): the rows of the band around the frame's middle row, on which the cameras (no pitch) see y = 0: the tall
    box, the spheres and the first extras"""
    f = frame(case)
    return (f["full_h"] or f["rows"]) // 2 - f["row_begin"] - 8, 16


# ---------------------------------------------------------------------------------------------------------------- launches
def samples_in_flight(case):
    """K (rt_tracer.hpp: pick_k): forced, or 2 samples per pass up to 128 triangles and 4 above, fewer at low spp"""
    if "k" in case["extra"]:
        return case["extra"]["k"]
    want = 2 if case["n_tris"] <= 128 else 4
    return want if case["spp"] >= want else 2 if case["spp"] >= 2 else 1


def bin_list(case):
    return max(32, (case["n_tris"] + 31) // 32 * 32)


def lds_bytes(case):
    """rt_tracer_info's lds_bytes (rt_kernels.hip: trace_lds_bytes): four waves' lists of 40-byte records, or the scan's chunk
    of 36-byte records"""
    if case["kernel"] == "scan":
        return min(case["n_tris"], 1024) * 36
    return 4 * bin_list(case) * 40


def iterations(case):
    """iterations of one Trace (one step of a steps case)"""
    if case["iters"] in ("one", "steps"):
        return 1
    return 3 if case["shape"] == "unsplit" else 2


def n_steps(case):
    return case["extra"].get("n_steps", 3) if case["iters"] == "steps" else 1


def has_certain_winners(case):
    """rt_trace.hpp's sure_ok: the kernel skips the tiles whose list says certain"""
    return case["kernel"] != "scan" and case["hit"] == "far" and case["extras"] == "none" and case["winners"] != "traced"


def owed_draws(case):
    """what rt_dbg_owed_state reports after the case's launches, before a read-back settles it: every launch after the first owes
    3 draws per sample (rt_tracer.hpp: owe_key_of, RngDebt::add; fewer than RT_OWE_PERIOD = 16 owing launches: no settle).  The
    launches of a cadence: one per iteration on the split frames (Launch); Trace(3, spp, 1) runs iterations 0 and 1 -- up to its
    first update point -- as one launch where the kernel fuses, then iteration 2 (rt_tracer.hpp: trace_funct)."""
    if not has_certain_winners(case) or case["winners"] == "no_owe" or case["iters"] in ("one", "fused"):
        return 0
    if case["iters"] == "steps":
        return 3 * case["spp"] * (n_steps(case) - 1)
    first = 2 if case["shape"] == "unsplit" and case["kernel"] == "filtered" else 1
    return 3 * case["spp"] * (iterations(case) - first)


def list_builds(case):
    """builds of the case's kind: every step of a steps case whose lists are not kept, one otherwise (the later launches of one
    Trace keep the lists of its first)"""
    if case["kernel"] == "scan":
        return 0
    return n_steps(case) if case["reuse"] == "rebuilt" else 1


# ---------------------------------------------------------------------------------------------------------------- scenes
def _facing(c, s, turn):
    """a triangle of circumradius s around c, perpendicular to the line from the origin, counter-clockwise seen from there"""
    d = c / np.linalg.norm(c)
    u = np.cross(d, (0.0, 1.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(u, d)
    tri = np.array([c + s * (np.cos(turn + k * 2.0 * np.pi / 3.0) * u + np.sin(turn + k * 2.0 * np.pi / 3.0) * v) for k in range(3)])
    if np.dot(np.cross(tri[1] - tri[0], tri[2] - tri[0]), c) > 0.0:         # the normal has to point at the camera (det > 0)
        tri[[1, 2]] = tri[[2, 1]]
    return tri


def extra_kind(k):
    """of extra k (triangle 32 + k): side -- to the left of the room, where a ray sees nothing else: seen under both hit rules;
    inside -- in the room in front of its walls: seen under nearest hit only; behind -- behind the lower left of the back
    wall: the farthest hit there, hidden under nearest hit"""
    return ("side", "inside", "behind", "inside")[k % 4]


def extras(count):
    """(count, 3, 3): the first `count` extra triangles, the same for every scene (a scene of n triangles holds the first n - 32)"""
    r = np.random.default_rng(20261)
    out = np.zeros((224, 3, 3))
    for k in range(224):
        u = r.uniform(size=6)
        kind = extra_kind(k)
        if kind == "side":
            phi = np.radians(EXTRA_SIDE_DEG[0] + (EXTRA_SIDE_DEG[1] - EXTRA_SIDE_DEG[0]) * (0.5 if k == 0 else u[0]))
            dist = 1.6 + 0.8 * u[1]
            c = np.array([-dist * np.sin(phi), 0.0 if k == 0 else -0.5 + u[2], -dist * np.cos(phi)])
            s = dist * (0.031 if k == 0 else 0.02 + 0.011 * u[3])       # 1.15 .. 1.8 degrees: a tile's width short of the side sphere
        elif kind == "inside":
            y = (-0.15 + 0.3 * u[1]) if k < 8 else (-0.8 + 1.6 * u[1])
            c = np.array([-0.8 + 1.6 * u[0], y, -2.9 + 1.6 * u[2]])
            s = 0.06 + 0.08 * u[3]
        else:
            c = np.array([-0.95 + 0.8 * u[0], -0.9 + 0.8 * u[1], -3.5 + 0.4 * u[2]])
            s = 0.1 + 0.1 * u[3]
        out[k] = _facing(c, s, 2.0 * np.pi * u[4])
    return out[:count]


def scene(case, seed=0, with_extras=True):
    """(rows, edge layout?): the Cornell box (its triangles FIVE where n = 5) and, above 32, the extras (with_extras=False: the box
    alone); the smooth cases in the edge layout with packed vertex normals that are not the faces'"""
    from raytracertest_amd import meshes, scenes
    n = case["n_tris"]
    rows = scenes.cornell32()
    if n < 32:
        rows = rows.reshape(32, 3, 4)[list(FIVE)[:n]].reshape(-1, 4)
    if n > 32 and with_extras:
        more = np.zeros((3 * (n - 32), 4), np.float32)
        more[:, :3] = extras(n - 32).reshape(-1, 3)
        rows = np.concatenate([rows, more])
    if "smooth" not in case["extras"]:
        return rows, False
    nrm = np.random.default_rng(seed).normal(size=(rows.shape[0], 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return meshes.to_edge_format(rows, normals=nrm), True


def seed_of(case):
    return 7919 * (CASES.index(next(c for c in CASES if c["name"] == case["name"])) + 1) % 100003


def oracle(orc, case, *, math=None, hit=None, spheres=None, smooth=None, with_extras=True, row0=0, rows=None, trace=True):
    """the case's oracle over rows [row0, row0 + rows) of the tracer's band, with one option changed if asked; traced as the case's
    iters value says (a steps case: n_steps Traces, each of which clears the accumulators)"""
    f = frame(case)
    seed = seed_of(case)
    math = case["math"] if math is None else math
    hit = case["hit"] if hit is None else hit
    smooth = "smooth" in case["extras"] if smooth is None else smooth
    spheres = "spheres" in case["extras"] if spheres is None else spheres
    tris, edges = scene(case, seed, with_extras)
    o = orc.OracleTracer(f["W"], f["full_h"] or f["rows"], f["angles"], f["fov"], FOCAL, APERTURE, seed=seed,
                         row0=f["row_begin"] + row0, rows=f["rows"] if rows is None else rows, contract=1 if math == "fma" else 0,
                         nthreads=8, hit_mode=int(hit == "near"), smooth_normals=smooth)
    assert (o.upload_scene_edges if edges else o.upload_scene)(tris)
    if spheres:
        o.upload_spheres(SPHERES)
    for _ in range(n_steps(case) if trace else 0):
        o.trace(iterations(case), case["spp"])
    return o


# ---------------------------------------------------------------------------------------------------------------- tiles
NOTHING, CERTAIN, MIXED = 0, 1, 2
_KINDS = {}


def tile_kinds(orc, case):
    """(kind, winner, met) per 8 x 8 tile of the band, from the oracle's probe of the tile's pixels x LENS against the case's
    triangles (farthest hit, no spheres): NOTHING -- no ray hits a triangle; CERTAIN -- every ray hits one triangle and none that
    it hits is farther (winner: that triangle); MIXED -- anything else.  met: how many triangles the tile's rays hit."""
    f = frame(case)
    key = (case["shape"], side(case), case["n_tris"], case["math"])
    if key in _KINDS:
        return _KINDS[key]
    W, rows, r0 = f["W"], f["rows"], f["row_begin"]
    o = orc.OracleTracer(W, f["full_h"] or rows, f["angles"], f["fov"], FOCAL, APERTURE, seed=1, row0=r0, rows=rows,
                         contract=1 if case["math"] == "fma" else 0)
    assert o.upload_scene(scene(dict(case, extras="none"))[0])
    ny, nx = (rows + 7) // 8, (W + 7) // 8
    kind, winner, met = np.zeros((ny, nx), np.int8), np.full((ny, nx), -1, np.int32), np.zeros((ny, nx), np.int32)
    for ty in range(ny):
        for tx in range(nx):
            pix = [(x, r0 + y) for y in range(ty * 8, min(ty * 8 + 8, rows)) for x in range(tx * 8, min(tx * 8 + 8, W))]
            probe, nohit = o.tile_probe(pix, LENS)
            rays = len(pix) * len(LENS)
            met[ty, tx] = int((probe["hits"] > 0).sum())
            w = int(np.argmax(probe["wins"]))
            if nohit == rays:
                kind[ty, tx] = NOTHING
            elif nohit == 0 and probe["wins"][w] == rays and probe["hits"][w] == rays:
                kind[ty, tx], winner[ty, tx] = CERTAIN, w
            else:
                kind[ty, tx] = MIXED
    _KINDS[key] = (kind, winner, met)
    return _KINDS[key]
