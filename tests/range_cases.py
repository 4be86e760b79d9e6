"""The newer queries at the ends of fp32's range: a scene and its query populations multiplied by 2^k, which is exact in fp32,
and what the numpy restatements answer there.  ClosestPoint, ClosestAll, SignedDistance, TriangleDistance, SphereCast, Overlap,
OverlapTriangles and OverlapHexahedra use no absolute constant in the arithmetic of their answers (the walk of SphereCast grows
its boxes by 2^-72, which changes no answer), so for as long as no intermediate is rounded differently their answers at scale
2^k are the k = 0 answers exactly rescaled: a squared distance t by 2^(2k); a sweep's t by 2^k when its direction is kept and not
at all when the direction carries the scale (the Clearance(a, b, r) form); a signed distance and a witness position by 2^k; u,
v, prims, counts, rows, features and `where` bit for bit.  A helper, not a test.  Everything is deterministic and needs no device.

RANGE[query] = [KLO, KHI] is the invariance range for the "lattice" inputs: unit right triangles on quarter-integer planes,
queries in multiples of 1/8, so that every intermediate at k = 0 is a dyadic number of a few bits between about 2^-8 and 2^4.
fp32 holds 2^-126 .. 2^128 normally and, exactly for such numbers, some way into the subnormals (to 2^-149).  What bounds a
range is the highest power of the scale the arithmetic forms:
  fourth powers   closest_triangle's va, vb, vc (products of two dot products e . ap) and den = 1 / ((va + vb) + vc): with unit
                  edges the sum is 2^(4k), which is +inf from k = 32 and whose reciprocal is +inf from k = -32 (1 / 2^-128).
                  [-31, 31] for ClosestPoint, ClosestAll and SignedDistance; the same powers in TriangleDistance's segment pairs
                  (a * e - b * b) and in SphereCast's start test, certification, sweep_face (nn = |e1 x e2|^2 divides) and
                  sweep_entry (a * disc): [-31, 31] as well.  With the direction scaled too the sweep forms n . d and dp . dp of
                  one more factor of the scale below a quotient, and the low end is -30.
  cubes and the sphere rules   a separating axis is a cross product (a square) and a projection on it a cube: |k| <= 42 for the
                  triangle rules of the region queries.  Their sphere rules are what ends their ranges first: OverlapTriangles'
                  and OverlapHexahedra's go through closest_triangle (fourth powers; the lattice's coordinates reach 2.25, so
                  the hexahedron's d2min overflows one step early, at 31), Overlap's compares squares, |k| <= 63.  On the low
                  side the dyadic projections stay exact as subnormals, and the ranges end where the first of them is rounded:
                  -36 for triangles, -32 for hexahedra, -62 for boxes.
test_range_cases.py asserts the rescaled-bytes equality at every k of INVARIANCE_KS (all inside every range) and that one step
beyond either end some row of the lattice populations differs.  Outside its range a query still answers, and the device still
gives the restatement's bytes (test_gpu_query_range.py); what is lost first is named in DESIGN.md: the interior region of
closest_triangle and the face contacts of SphereCast.  On the "slivers" scene, whose inputs are not dyadic and span 2^-23 .. 2^10,
the first rows change at k = -26 and 32 (points), -24 and 24 (sweeps)."""
import numpy as np

import closest_expect as ce
import hexoverlap_expect as he
import nearest_expect as ne
import overlap_expect as oe
import signed_expect as sg
import spherecast_expect as se
import tridistance_expect as td
import trioverlap_expect as te

f32 = np.float32
INF = f32(np.inf)
QUERIES = ("closest", "nearest4", "signed", "tridistance", "spherecast_kept", "spherecast_scaled", "overlap", "trioverlap", "hexoverlap")
RANGE = {"closest": (-31, 31), "nearest4": (-31, 31), "signed": (-31, 31), "tridistance": (-31, 31), "spherecast_kept": (-31, 31),
         "spherecast_scaled": (-30, 31), "overlap": (-62, 63), "trioverlap": (-36, 31), "hexoverlap": (-32, 30)}
INVARIANCE_KS = (0, 8, -8, 24, -24, 30, -30)
TREE_KS = (0, 30, -30, 33, -33, 48, -48, 60, -60, 62, -64, -70, -76, -84)
MAX_HITS = 4
_cache = {}


def factor(k):
    s = f32(2.0) ** k
    assert s.dtype == f32 and s > 0 and np.isfinite(s)
    return s


# ---- the scene and the populations at k = 0 ----------------------------------------------------------------------------------

def scene(kind):
    """(rows, spheres).  "slivers": spherecast_expect.scene(300) -- every second triangle a sliver, a segment, a point and one
    record with a NaN (the always-tested list) -- and its three spheres: the scene of the tree and device checks.  "lattice":
    lattice_cases.rooms() and one sphere, unit edges on quarter-integer planes: every intermediate of every query is a small
    dyadic number, the inputs the stated ranges are for."""
    if kind == "lattice":
        import lattice_cases as lc
        return lc.rooms(), f32([[0.25, 0.25, 0.25, 0.5]])
    return se.scene(300), se.three_spheres()


def populations(kind):
    """{name: queries at k = 0} for scene(kind): points {x, y, z, d2max} (every third within a finite squared distance), query
    triangles (every third likewise), boxes, hexahedra, and sweeps."""
    if kind in _cache:
        return _cache[kind]
    rows, spheres = scene(kind)
    if kind == "lattice":
        import lattice_cases as lc
        v0, e1, e2 = (x[::20] for x in ce.records_of_rows(rows))         # a quarter up each edge and a quarter off the face: the
        n = np.cross(e1, e2)                                             # nearest point is interior, the region whose u, v divide
        p3 = np.concatenate([ce.lattice_points()[::3], (v0 + f32(0.25) * e1 + f32(0.25) * e2 + f32(0.25) * n).astype(f32)])
        pts = ce.with_radius(p3, np.where(np.arange(p3.shape[0]) % 3 == 2, f32(0.0625), INF))
        tris = td.lattice_queries()[::4].copy()
        tris[2::3, 3] = f32(0.0625)
        boxes = np.concatenate([oe.touching_boxes(rows, range(0, 480, 24))[0], oe.point_boxes(rows, range(0, 480, 16))])
        lo, hi = boxes[:, 0:3], boxes[:, 4:7]
        skew = he.box_corners(lo, hi)
        skew[:, 4:, 0] += f32(0.25)                                      # sheared by a quarter: still dyadic
        rays = np.concatenate([lc.axis_rays(), lc.in_plane_rays()])[::2]
        sweeps = np.concatenate([np.c_[rays, np.full(len(rays), r, f32), np.full(len(rays), np.inf, f32)] for r in (0.0, 0.125, 0.25, 0.5)]).astype(f32)
        sweeps[1::3, 7] = f32(1.0)
        out = {"points": pts, "tris": tris, "boxes": boxes, "trioverlap": np.concatenate([te.coplanar_queries(rows, range(0, 480, 12)), tris[:100]]),
               "hexa": he.queries_of(np.concatenate([he.box_corners(lo, hi), skew])), "sweeps": np.ascontiguousarray(sweeps)}
        _cache[kind] = out
        return out
    p3 = ce.points_for(rows, 600, 71, spread=4.0)
    t = ce.expected(ce.with_radius(p3, INF), rows, spheres=spheres)["t"]
    pts = ce.with_radius(p3, np.where(np.arange(600) % 3 == 2, f32(np.median(t)), INF))
    tris = td.mixed_queries(rows, 240, 72)
    with np.errstate(all="ignore"):
        tt = td.expected(tris, rows, spheres=spheres)[0]["t"]
    tris[2::3, 3] = f32(np.median(tt[np.isfinite(tt)]))
    out = {"points": pts, "tris": tris, "boxes": oe.random_boxes(rows, 400, 73, width=1.0), "trioverlap": te.mixed_queries(rows, 300, 74),
           "hexa": he.mixed_queries(rows, 300, 75), "sweeps": se.batch(rows, 2600, 7, spheres=spheres)}
    _cache[kind] = out
    return out


# ---- scaling, exact in fp32 --------------------------------------------------------------------------------------------------

def scaled_scene(rows, spheres, k):
    s = factor(k)
    return np.ascontiguousarray(np.asarray(rows, f32) * s), (None if spheres is None else np.ascontiguousarray(np.asarray(spheres, f32) * s))


def scaled_populations(pops, k):
    """The populations at scale 2^k: every length times s, every squared length (a d2max) times s * s -- in that order, one
    rounding each, which is exact until the product itself leaves the range; the sweeps in both forms: "sweeps_kept" keeps the
    direction (t and tmax scale) and "sweeps_scaled" scales it (t and tmax do not)."""
    s = factor(k)
    with np.errstate(all="ignore"):
        pts = pops["points"] * s
        pts[:, 3] = (pops["points"][:, 3] * s) * s
        tris = pops["tris"] * s
        tris[:, 3] = (pops["tris"][:, 3] * s) * s
        kept = pops["sweeps"] * s
        kept[:, 3:6] = pops["sweeps"][:, 3:6]
        scaled = pops["sweeps"] * s
        scaled[:, 7] = pops["sweeps"][:, 7]
    out = {"points": pts, "tris": tris, "boxes": pops["boxes"] * s, "trioverlap": pops["trioverlap"] * s, "hexa": pops["hexa"] * s,
           "sweeps_kept": kept, "sweeps_scaled": scaled}
    assert all(v.dtype == f32 for v in out.values())
    return {name: np.ascontiguousarray(v) for name, v in out.items()}


# ---- the restatements' answers -------------------------------------------------------------------------------------------------

def _flat(x):
    return list(x) if isinstance(x, tuple) else [x]


def brute_force(query, rows, spheres, pops):
    """One query's answer by its restatement's brute force, as a list of arrays."""
    with np.errstate(all="ignore"):
        if query == "closest":
            return [ce.expected(pops["points"], rows, spheres=spheres)]
        if query == "nearest4":
            return _flat(ne.expected_all(ce.table(pops["points"], rows, spheres=spheres), pops["points"][:, 3], MAX_HITS))
        if query == "signed":
            hits = ce.expected(pops["points"], rows, spheres=spheres)
            return [hits, sg.expected_sides(pops["points"], hits, rows, sg.feature_table64(rows), spheres=spheres)]
        if query == "tridistance":
            return _flat(td.expected(pops["tris"], rows, spheres=spheres))
        if query in ("spherecast_kept", "spherecast_scaled"):
            return [se.expected(pops["sweeps_" + query[11:]], rows, spheres=spheres)]
        if query == "overlap":
            return _flat(oe.expected(pops["boxes"], rows, MAX_HITS, spheres=spheres))
        if query == "trioverlap":
            return _flat(te.expected(pops["trioverlap"], rows, MAX_HITS, spheres=spheres))
        if query == "hexoverlap":
            return _flat(he.expected(pops["hexa"], rows, MAX_HITS, spheres=spheres))
    raise KeyError(query)


TREE_QUERIES = tuple(q for q in QUERIES if q != "signed")                 # SignedDistance's hit half is ClosestPoint's


def tree_walk(query, tree, rows, spheres, pops):
    """The same answer by the query's restated tree walk."""
    with np.errstate(all="ignore"):
        if query == "closest":
            return [ce.walk_tree_closest(*tree, pops["points"], rows, spheres=spheres)[0]]
        if query == "nearest4":
            return list(ne.walk_tree_nearest(*tree, pops["points"], rows, MAX_HITS, spheres=spheres)[:2])
        if query == "tridistance":
            return _flat(td.walk_tree_tridistance(*tree, pops["tris"], rows, spheres=spheres)[0])
        if query in ("spherecast_kept", "spherecast_scaled"):
            return [se.walk_tree_spherecast(*tree, pops["sweeps_" + query[11:]], rows, spheres=spheres)[0]]
        if query == "overlap":
            return list(oe.walk_tree_overlap(*tree, pops["boxes"], rows, MAX_HITS, spheres=spheres)[:2])
        if query == "trioverlap":
            return list(te.walk_tree_triangles(*tree, pops["trioverlap"], rows, MAX_HITS, spheres=spheres)[:2])
        if query == "hexoverlap":
            return list(he.walk_tree_hexahedra(*tree, pops["hexa"], rows, MAX_HITS, spheres=spheres)[:2])
    raise KeyError(query)


def rescaled(query, answer, k):
    """The k = 0 answer as it must read at scale 2^k while the query is inside its range."""
    s = factor(k)
    out = [np.array(a, copy=True) for a in answer]
    with np.errstate(all="ignore"):
        if query in ("closest", "nearest4", "signed", "tridistance"):
            out[0]["t"] = (out[0]["t"] * s) * s
        if query == "signed":
            out[1]["s"] = out[1]["s"] * s
        if query == "tridistance":
            for c in "xyz":
                out[1][c] = out[1][c] * s
        if query == "spherecast_kept":
            out[0]["t"] = out[0]["t"] * s
    return out


def differing_rows(a, b):
    """The rows in which two answers (lists of arrays of the same shapes) differ in any byte."""
    bad = np.zeros(a[0].shape[0], bool)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        xb = np.ascontiguousarray(x).reshape(x.shape[0], -1).view(np.uint8)
        yb = np.ascontiguousarray(y).reshape(y.shape[0], -1).view(np.uint8)
        bad |= (xb != yb).any(axis=1)
    return np.nonzero(bad)[0]


def found(query, answer):
    """How many queries of an answer found anything."""
    a = answer[0]
    if a.dtype.names and "prim" in a.dtype.names:
        return int((a["prim"].reshape(a.shape[0], -1)[:, 0] >= 0).sum())
    return int((answer[1] > 0).sum())
