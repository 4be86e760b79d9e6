"""The six tree-walk kernels at the BVH's depth bound and past their stack: on deep_cases' ladders, whose tree
has 16 levels and whose populations hold all 48 entries of the stack in each of the six kernels' orders (test_bvh_deep.py
asserts the restated marks, Exposure's included), every BVH query equals the scan on the same tracer under
that query's own check, in both layouts, both arithmetic modes and both hit rules; the device refit of 16 levels is the host's;
and with the stack shortened by DebugQueryStackCap every lane that needs one entry more answers from every leaf record -- the
overflow path, which no tree of the builder reaches on its own -- under the same checks.  The four newer walkers on the same
bvh_walk (region_bvh_kernel for boxes and triangles, spherecast_bvh_kernel, tridistance_bvh_kernel), each with an overflow
restart of its own and a restated walk whose marks say which lanes take it, go through every one of these cases with region_pops' boxes, query triangles and sweeps: they equal the
scan byte for byte by contract, every row, at every cap."""
import numpy as np
import pytest

import closest_expect as ce
import deep_cases as dc
import exposure_expect as ee
import lattice_cases as lc
import nearest_expect as ne
import overlap_expect as oe
import refit_cases as rc
import spherecast_expect as spe
import tridistance_expect as td
import trioverlap_expect as te
from allhits_expect import check_bvh_all_hits, same_rows, sets_from_oracle
from occluded_expect import check_bvh_occluded
from query_accel_expect import check_against_scan, check_tree, walk_tree
from query_expect import adversarial_rays, adversarial_scene, edge_rows, expected_hits, same_hits

pytestmark = pytest.mark.gpu

ONE_RAY = np.array([[0, 0, 0, 0.1, 0.2, -1]], np.float32)
ADV_SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
MAX_HITS = (1, 4, 16)
REGION_HITS = (0, 4, 16)                                                 # Overlap's and OverlapTriangles' three list capacities
BYTE_EQUAL = ("overlap", "trioverlap", "spherecast", "tridistance")      # tree == scan by contract: no exclusion
ROW_POPULATIONS = ("rays", "segs", "points", "exposure", "boxes", "tris", "sweeps")
_cache = {}


def _tracer(math_mode=0, nearest=False, refit=False, **kw):
    import raytracertest_amd as R
    g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)
    g.SetQueryAcceleration(True)
    if refit:
        g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    return g


def _upload(g, rows, edges=False):
    assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _row_bytes(a):
    return np.ascontiguousarray(a).reshape(a.shape[0], -1).view(np.uint8)


def deep_spheres(mirror):
    """Four spheres of the ladder's scales: a small one on the axis, and a middle one, its copy and a large one beside it (the
    rays along the axis pass them: a lane that a sphere finishes never walks the tree)."""
    s = dc.scales()
    z = -1.0 if mirror else 1.0
    axis = dc.AXIS * [1.0, 1.0, z]
    mid = s[len(s) // 2]
    return np.array([np.r_[s[8] * axis, 0.3 * s[8]], np.r_[mid * (axis + [0.0, 0.6, 0.0]), 0.25 * mid], np.r_[mid * (axis + [0.0, 0.6, 0.0]), 0.25 * mid],
                     np.r_[s[-3] * (axis + [0.0, 1.5, 0.0]), 0.5 * s[-3]]], np.float32)


def region_pops(rows, seed, n=160):
    """{boxes, tris, sweeps} for Overlap, OverlapTriangles / TriangleDistance and SphereCast: n boxes around and n query triangles
    beside the scene's own finite triangles, and n sweeps of spherecast_expect.random_sweeps(rel=True), all in units of the
    chosen triangle's extent (the ladder spans 2^69).  A box's half widths and a query's size are 2^-2 .. 2^5 extents: the small
    ones touch a leaf or nothing, the large ones reach every root child and, on the ladder, cover the origin and with it every
    smaller cluster.  Every sixteenth box and query triangle spans the whole scene, by a different margin each: its walk enters all
    four children at every level, the fullest stack there is (48 of 48 entries on the ladder), beside neighbours in the wave that
    hold a few; sixteen sweeps of 3 .. 30 extents' radius start in overlap with many records, which all tie at t = 0, and the four
    of spherecast_expect.whole_scene_sweeps, at the end, with most of the scene (48 of 48 entries on the ladder).  A quarter
    of the query triangles search within half an extent.  Then the rows that accept nothing: an inverted and a NaN box, a NaN corner, a
    negative and a NaN radius, and spherecast_expect.bad_sweeps."""
    rng = np.random.default_rng(seed)
    t = np.asarray(rows, np.float64).reshape(-1, 3, 4)[:, :, :3]
    with np.errstate(invalid="ignore"):
        fin = np.nonzero(np.isfinite(t).all(axis=(1, 2)) & (np.abs(t) < 1e30).all(axis=(1, 2)))[0]
    k = fin[rng.integers(0, fin.size, n)]
    cen = t[k].mean(axis=1)
    ext = np.abs(t[k] - cen[:, None, :]).max(axis=(1, 2))[:, None]
    c = cen + ext * rng.uniform(-1.0, 1.0, (n, 3))
    half = ext * 2.0 ** rng.uniform(-2.0, 5.0, (n, 1)) * rng.uniform(0.25, 1.0, (n, 3))
    boxes = oe.boxes_of(c - half, c + half)
    boxes[0, 0], boxes[0, 4] = boxes[0, 4], boxes[0, 0]                  # inverted on x
    boxes[1, 5] = np.nan
    size = (ext * 2.0 ** rng.uniform(-2.0, 5.0, (n, 1)))[:, :, None]
    tris = te.queries_of((cen + ext * rng.uniform(-1.5, 1.5, (n, 3)))[:, None, :] + size * rng.uniform(-1.0, 1.0, (n, 3, 3)))
    tris = td.with_radius(tris, np.where(np.arange(n) % 4 == 3, (0.5 * ext[:, 0]) ** 2, np.inf))
    lo, hi = t[fin].min(axis=(0, 1)), t[fin].max(axis=(0, 1))
    for j in range(8, n, 16):                                            # the whole scene
        d = (hi - lo) * 2.0 ** (j // 16 - 3)
        boxes[j] = oe.boxes_of(lo - d, hi + d)[0]
        tris[j] = td.with_radius(te.queries_of([[lo - d, hi + d, [lo[0] - d[0], hi[1] + d[1], 0.5 * (lo[2] + hi[2])]]]), np.inf)[0]
    tris[0, 5], tris[1, 3], tris[2, 3] = np.nan, -1.0, np.nan
    with np.errstate(over="ignore"):
        sweeps = np.concatenate([spe.random_sweeps(rows, n - 16, seed + 1, rel=True),
                                 spe.random_sweeps(rows, 16, seed + 2, rmin=0.5, rmax=1.5, rel=True)])
        whole = spe.whole_scene_sweeps(rows)                             # the fullest stack the sweep walk can hold
    return {"boxes": boxes, "tris": np.ascontiguousarray(tris, np.float32),
            "sweeps": np.ascontiguousarray(np.concatenate([sweeps, spe.bad_sweeps(sweeps[0]), whole]), np.float32)}


def deep_pops(mirror):
    """The ladder's populations as the queries take them, once per session."""
    key = ("deep", mirror)
    if key not in _cache:
        from raytracertest_amd import api
        rays = dc.rays(mirror=mirror)
        _cache[key] = {"rays": rays, "segs": dc.segments(rays), "points": dc.points(mirror=mirror),
                       "exposure": dc.exposure_points(mirror=mirror), "dirs": ee.as_dirs4(api.hemisphere_directions(64)),
                       **region_pops(dc.deep_scene(mirror=mirror), 43)}
    return _cache[key]


def scene_pops(rows, seed, n=200):
    """Populations for an ordinary scene: adversarial rays (non-finite and zero-direction ones included), their segments by
    turns and eight inactive ones, points near and far with every radius family, exposure points on triangle centroids."""
    from raytracertest_amd import api
    rng = np.random.default_rng(seed)
    rays = adversarial_rays(rows, n, seed)[-(n + 60):]
    segs = lc.ray_segments(rays)
    dead = segs[:8].copy()
    dead[:, 6], dead[:, 7] = 1.0, 0.5
    p3 = ce.points_for(rows, n, seed + 1)
    fam = ce.radius_families(p3[:40], rows)
    pts = np.concatenate([ce.with_radius(p3, ce.INF)] + [fam[k] for k in ("half", "zero", "nan", "negative")])
    tris = np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3]
    fin = np.isfinite(tris).all(axis=(1, 2))
    cen = tris[fin][rng.integers(0, int(fin.sum()), 24)].mean(axis=1)
    nrm = rng.normal(0, 1, (24, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    expo = np.ascontiguousarray(np.c_[cen, nrm, np.full(24, 1e-3), np.full(24, np.inf)], np.float32)
    return {"rays": rays, "segs": np.ascontiguousarray(np.concatenate([segs, dead]), np.float32), "points": np.ascontiguousarray(pts, np.float32),
            "exposure": expo, "dirs": ee.as_dirs4(api.hemisphere_directions(64)), **region_pops(rows, seed + 2, min(n, 160))}


def answers(g, pops, intersect=True):
    """Every tree-walking query of the populations on the tracer's current mode, as {name: answer}."""
    out = {}
    with np.errstate(all="ignore"):
        if intersect:
            out["intersect"] = g.Intersect(pops["rays"])
        out["occluded"] = g.Occluded(pops["segs"])
        for m in MAX_HITS:
            out["all%d" % m] = g.IntersectAll(pops["segs"], m)
        out["closest"] = g.ClosestPoint(pops["points"])
        out["signed"] = g.SignedDistance(pops["points"])
        for m in MAX_HITS:
            first = g.ClosestAll(pops["points"], m)
            after = np.ascontiguousarray(first[0][:, m - 1])              # the cursor, chained once (prim -1: none)
            after[3]["t"] = np.nan                                        # ... and one NaN cursor: that point accepts nothing
            after[3]["prim"] = 0
            out["nearest%d" % m] = first
            out["nearest%d_after" % m] = g.ClosestAll(pops["points"], m, after=after)
        out["exposure64"] = g.Exposure(pops["exposure"], pops["dirs"])
        out["exposure5"] = g.Exposure(pops["exposure"], dc.SHORT_TABLE, world=True)
        out["exposure64_occluded"] = g.Occluded(ee.exposure_segments(pops["exposure"], pops["dirs"]))
        out["exposure5_occluded"] = g.Occluded(ee.exposure_segments(pops["exposure"], dc.SHORT_TABLE, world=True))
        for name, query, batch in (("overlap", g.Overlap, pops["boxes"]), ("trioverlap", g.OverlapTriangles, pops["tris"])):
            for m in REGION_HITS:
                out["%s%d" % (name, m)] = query(batch, m)
            out[name + "4_after"] = query(batch, 4, after=np.ascontiguousarray(out[name + "4"][0][:, 3]))    # the cursor, chained once
        out["spherecast"] = g.SphereCast(pops["sweeps"])
        out["tridistance"] = g.TriangleDistance(pops["tris"])
    return out


def same_answers(a, b):
    return a.keys() == b.keys() and all(_bits(np.asarray(x)) == _bits(np.asarray(y)) if not isinstance(x, tuple)
                                        else all(_bits(p) == _bits(q) for p, q in zip(x, y)) for x, y in ((a[k], b[k]) for k in a))


def check_answers(got, scan, pops, rows, orc, spheres=None, contract=None, label="", exact=False, edges=False):
    """The BVH answers `got` against the scan's under each query's own check (exact: byte equality throughout -- the lattice
    populations); the point queries byte for byte; Exposure = the packed complement of Occluded over the same segments in the
    same mode."""
    with np.errstate(all="ignore"):
        if exact:
            assert same_answers(*({k: v for k, v in a.items() if not k.startswith("exposure")} for a in (got, scan))), label
        if "intersect" in got:
            check_against_scan(got["intersect"], scan["intersect"], pops["rays"], edge_rows(rows) if edges else rows, edges, label=label)
        check_bvh_occluded(got["occluded"], scan["occluded"], pops["segs"], rows, orc, spheres, contract, label=label)
        E, W = sets_from_oracle(orc, pops["segs"], rows, spheres, contract)
        for m in MAX_HITS:
            check_bvh_all_hits(got["all%d" % m], scan["all%d" % m], E, W, m, label="%s max_hits=%d" % (label, m))
    assert ce.same_hits(got["closest"], scan["closest"]), (label, ce.differing(got["closest"], scan["closest"]))
    assert ce.same_hits(got["signed"][0], got["closest"]) and _bits(got["signed"][1]) == _bits(scan["signed"][1]), label
    for m in MAX_HITS:
        for key in ("nearest%d" % m, "nearest%d_after" % m):
            assert ne.differing_rows(got[key][0], scan[key][0], got[key][1], scan[key][1]).size == 0, (label, key)
        assert got["nearest%d_after" % m][1][3] == 0, label             # the NaN cursor
    assert_region_bytes(got, scan, label)                                # the four newer walkers: the scan's bytes, every row
    for key, dirs, world in (("exposure64", pops["dirs"], False), ("exposure5", dc.SHORT_TABLE, True)):
        for ans in (got, scan):
            want = ee.pack_masks(~ans[key + "_occluded"].reshape(-1, dirs.shape[0]))
            assert np.array_equal(ans[key], want), (label, key)
        segs = ee.exposure_segments(pops["exposure"], dirs, world=world)
        check_bvh_occluded(got[key + "_occluded"], scan[key + "_occluded"], segs, rows, orc, spheres, contract, label="%s %s" % (label, key))


def assert_region_bytes(got, want, label):
    """The answers of Overlap, OverlapTriangles, SphereCast and TriangleDistance in `got` against those in `want`, byte for byte."""
    keys = [k for k in got if k.startswith(BYTE_EQUAL)]
    assert len(keys) == 2 * (len(REGION_HITS) + 1) + 2, keys
    for key in keys:
        parts = [(got[key], want[key])] if not isinstance(got[key], tuple) else list(zip(got[key], want[key]))
        for a, b in parts:
            bad = np.nonzero((_row_bytes(a) != _row_bytes(b)).any(axis=1))[0]
            assert a.dtype == b.dtype and a.shape == b.shape and bad.size == 0, (label, key, bad[:5], a[bad[:3]], b[bad[:3]])


def restated_regions(pops, rows, edges, spheres):
    """What answers() must give for the four newer queries, by brute force over the numpy restatements' tables."""
    up = edge_rows(rows) if edges else rows
    out = {}
    with np.errstate(all="ignore"):
        for name, acc in (("overlap", oe.table(pops["boxes"], up, edges, spheres)), ("trioverlap", te.table(pops["tris"], up, edges, spheres))):
            for m in REGION_HITS:
                out["%s%d" % (name, m)] = oe.rows_of_table(acc, m)
            out[name + "4_after"] = oe.rows_of_table(acc, 4, out[name + "4"][0][:, 3])
        out["spherecast"] = spe.expected(pops["sweeps"], up, edges, spheres)
        out["tridistance"] = td.expected(pops["tris"], up, edges, spheres)
    return out


def scan_and_tree(g, pops, intersect=True):
    g.SetQueryAcceleration(False)
    scan = answers(g, pops, intersect)
    g.SetQueryAcceleration(True)
    return scan, answers(g, pops, intersect)


# ---- 1. a full stack ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math_mode", [0, 1])
@pytest.mark.parametrize("name", ["mirror", "plain"])
def test_every_query_on_the_deep_tree_equals_the_scan(orc, name, math_mode):
    mirror = name == "mirror"
    rows, pops = dc.deep_scene(mirror=mirror), deep_pops(mirror)
    contract = orc.FMA if math_mode == 0 else orc.STRICT
    spheres = deep_spheres(mirror) if (mirror and math_mode == 0) else None
    for edges in (False, True):
        label = "%s mm=%d edges=%d" % (name, math_mode, edges)
        g = _tracer(math_mode)
        _upload(g, rows, edges)
        if spheres is not None:
            g.UploadSpheres(spheres)
        scan, got = scan_and_tree(g, pops)
        info = g.QueryAccelInfo()
        assert info["depth"] == dc.DEPTH_BOUND and info["valid"] == 1 and info["always_tested"] == 0
        check_answers(got, scan, pops, rows, orc, spheres, contract, label, edges=edges)
        assert scan["occluded"].any() and not scan["occluded"].all() and (scan["all16"][1] == 16).any()
        assert 0 < ee.popcount(scan["exposure64"]).sum() < 64 * pops["exposure"].shape[0]
        for n in (1, 63, 65):                                            # partial waves: the last rays and points decide nothing
            r, s, p = pops["rays"][-n:], pops["segs"][-n - 8:-8], pops["points"][:n]
            assert same_hits(g.Intersect(r), got["intersect"][-n:]) and np.array_equal(g.Occluded(s), got["occluded"][-n - 8:-8])
            assert same_rows(g.IntersectAll(s, 16), (got["all16"][0][-n - 8:-8], got["all16"][1][-n - 8:-8]))
            assert ce.same_hits(g.ClosestPoint(p), got["closest"][:n])
            few = g.ClosestAll(p, 4)
            assert ne.differing_rows(few[0], got["nearest4"][0][:n], few[1], got["nearest4"][1][:n]).size == 0
            many = np.tile(pops["exposure"][::-1], (3, 1))[:n]            # (25 points, the undeciding ones first; four to a block)
            assert np.array_equal(g.Exposure(many, pops["dirs"]), np.tile(got["exposure64"][::-1], 3)[:n])
        # the scan is not the only witness: brute force for the points, the oracle for every sixth ray
        assert ce.same_hits(got["closest"], ce.expected(pops["points"], edge_rows(rows) if edges else rows, edges, spheres)), label
        if not edges:
            sub = pops["rays"][::6]
            with np.errstate(all="ignore"):
                check_against_scan(got["intersect"][::6], expected_hits(orc, sub, rows, spheres, contract), sub, rows, label=label + " oracle")
        g.close()
        g = _tracer(math_mode, nearest=True)                              # the other hit rule: Intersect alone names one
        _upload(g, rows, edges)
        if spheres is not None:
            g.UploadSpheres(spheres)
        g.SetQueryAcceleration(False)
        with np.errstate(all="ignore"):
            near_scan = g.Intersect(pops["rays"])
            g.SetQueryAcceleration(True)
            check_against_scan(g.Intersect(pops["rays"]), near_scan, pops["rays"], edge_rows(rows) if edges else rows, edges, label=label + " nearest")
        assert (near_scan["prim"] >= 0).sum() > pops["rays"].shape[0] // 8
        g.close()


# ---- 2. the refit at 16 levels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mirror", "plain"])
def test_device_refit_of_sixteen_levels_equals_the_host_refit(orc, name):
    from raytracertest_amd import api
    mirror = name == "mirror"
    rows, pops = dc.deep_scene(mirror=mirror), deep_pops(mirror)
    twice, moved = dc.doubled(rows), dc.jittered(rows)
    for edges in (False, True):                                          # the layout of the moved uploads; the first is the other one
        g = _tracer(refit=True)
        _upload(g, rows, not edges)
        g.Intersect(ONE_RAY)
        built, u0 = g.query_tree(), g.QueryAccelUpdateInfo()
        assert rc.same_tree(built, api.bvh_build(edge_rows(rows) if not edges else rows, not edges)) and built[2]["depth"] == dc.DEPTH_BOUND
        assert np.bincount(rc.node_levels(built[0])).shape[0] == dc.DEPTH_BOUND          # one launch per level, sixteen of them
        _upload(g, twice, edges)
        g.Intersect(ONE_RAY)
        tree, u1 = g.query_tree(), g.QueryAccelUpdateInfo()
        up = edge_rows(twice) if edges else twice
        assert rc.same_tree(tree, api.bvh_refit(up, *built, edges=edges)), (name, edges)
        assert tree[0].tobytes() == dc.doubled_boxes(built[0]).tobytes()
        check_tree(*tree, up, edges)
        assert u1["refits"] == 1 and u1["fallbacks"] == 0 and tree[2] == built[2]
        host_cost = api.tree_cost(tree[0])
        assert abs(u1["cost"] - host_cost) <= 1e-12 * host_cost and u1["cost_built"] == u0["cost_built"]
        _upload(g, moved, edges)                                          # the jittered move, a refit of the refitted tree
        g.Intersect(ONE_RAY)
        tree2, u2 = g.query_tree(), g.QueryAccelUpdateInfo()
        up = edge_rows(moved) if edges else moved
        assert rc.same_tree(tree2, api.bvh_refit(up, *tree, edges=edges)) and u2["refits"] == 2 and u2["fallbacks"] == 0
        host_cost = api.tree_cost(tree2[0])
        assert abs(u2["cost"] - host_cost) <= 1e-12 * host_cost
        print("%s edges=%d: refits of 16 levels %d and %d us, cost %.6g -> %.6g -> %.6g" % (name, edges, u1["refit_us"], u2["refit_us"], u0["cost"], u1["cost"], u2["cost"]))
        sub = {k: (v[::3] if k in ROW_POPULATIONS else v) for k, v in pops.items()}
        scan, got = scan_and_tree(g, sub)
        check_answers(got, scan, sub, moved, orc, label="%s edges=%d after two refits" % (name, edges), edges=edges)
        g.DebugQueryStackCap(1)                                           # the refit walks no stack: the hook leaves it alone
        _upload(g, rows, edges)
        g.Intersect(ONE_RAY)
        assert rc.same_tree(g.query_tree(), api.bvh_refit(edge_rows(rows) if edges else rows, *tree2, edges=edges))
        assert g.QueryAccelUpdateInfo()["refits"] == 3
        g.close()


# ---- 3. the overflow fallback ---------------------------------------------------------------------------------------------------

def _bad_vertices(rows):
    """Non-finite triangles: the always-tested list behind the leaves' records."""
    r = rows.copy().reshape(-1, 3, 4)
    r[3, 1, 0] = np.nan
    r[10, 2, 2] = np.inf
    r[11, 0, 1] = -np.inf
    r[20, 0, :3] = 3.0e38                                                 # finite vertices whose edges overflow
    r[20, 1, :3] = -3.0e38
    return r.reshape(-1, 4)


def _fallback_case(orc, name):
    """-> rows, populations, spheres, exact (the populations are the lattice's: byte equality with the scan)."""
    if name == "deep":
        return dc.deep_scene(mirror=True), deep_pops(True), deep_spheres(True), False
    if name == "adversarial":
        rows = adversarial_scene(300, 11)
        return rows, scene_pops(rows, 5), ADV_SPHERES, False
    if name == "bad_vertices":
        rows = _bad_vertices(adversarial_scene(37, 3))
        return rows, scene_pops(rows, 7, 200), None, False
    from raytracertest_amd import api
    rows = lc.rooms()
    lattice, _ = lc.rooms_populations(orc, rows, api.bvh_build(rows)[0])
    rays = np.concatenate([lattice[k] for k in lc.LATTICE])
    pts = ce.lattice_points()
    pops = {"rays": rays, "segs": lc.ray_segments(rays), "points": np.concatenate([ce.with_radius(pts, ce.INF), ce.with_radius(pts, 0.25)]),
            "exposure": np.ascontiguousarray(np.c_[pts[:24] + np.float32(0.125), np.tile([0.0, 0.0, 1.0], (24, 1)), np.zeros(24), np.full(24, np.inf)], np.float32),
            "dirs": ee.as_dirs4(lc.DIRECTIONS), **region_pops(rows, 13)}
    pops["tris"] = np.ascontiguousarray(np.concatenate([pops["tris"], td.lattice_queries()[::8]]))   # and the lattice's own: ties by the dozen
    return rows, pops, None, True


@pytest.mark.parametrize("name", ["deep", "adversarial", "bad_vertices", "rooms"])
def test_a_shortened_stack_answers_from_every_leaf_record(orc, name):
    """Caps 0, 1, 3, 3 x depth - 1 (one entry short) and 3 x (depth - 1) (one level short: on the ladder only the lanes with
    the fullest stacks overflow).  A lane whose restated walk holds more entries than the cap overflows: the counts are printed
    per cap and walk -- ClosestPoint's and ClosestAll's over every point, Intersect's, Occluded's and IntersectAll's over about
    fifty rays spread over the batch, Exposure's over every sixteenth segment.  With cap 0 every lane that meets an inner node
    with two live children overflows, and on every scene that must be most of the batch in each of the six walks: more than
    half of ALL lanes, the inactive ones, the bad radii and the lanes a sphere finishes before the root included (the
    batches are sized so that these stay the minority).  The any-hit walks' share among the lanes that stay open is printed
    beside it."""
    rows, pops, spheres, exact = _fallback_case(orc, name)
    from raytracertest_amd import api
    nodes, recs, info = api.bvh_build(rows)
    marks = restated_marks(orc, nodes, recs, info, pops, rows, spheres)
    share = {k: float((m > 0).mean()) for k, m in marks.items()}
    print("%s: share of each restated walk's lanes that hold an entry at all: %s" % (name, {k: round(v, 2) for k, v in share.items()}))
    assert all(v > 0.5 for k, v in share.items() if not k.endswith("open lanes")), share
    newer, wide = region_marks(nodes, recs, info, pops, rows, spheres)
    print("%s: the fullest stacks of the newer walks' restatements (every fourth lane, every sweep): %s; sweeps whose box meets more than one root child: %d of %d"
          % (name, {k: int(m.max()) for k, m in newer.items()}, int(wide.sum()), wide.shape[0]))
    assert all((m > 0).any() for m in newer.values())
    if name == "deep":                                                   # lanes that only the one-entry-short cap overflows
        assert all(m.max() == 3 * info["depth"] and (m < 3 * (info["depth"] - 1)).any() for m in newer.values()), newer
    marks.update(newer)
    for math_mode, edges in ((0, False), (1, True)):
        contract = orc.FMA if math_mode == 0 else orc.STRICT
        g = _tracer(math_mode)
        _upload(g, rows, edges)
        if spheres is not None:
            g.UploadSpheres(spheres)
        scan, before = scan_and_tree(g, pops)
        depth = g.QueryAccelInfo()["depth"]
        assert depth == info["depth"]
        check_answers(before, scan, pops, rows, orc, spheres, contract, "%s product" % name, exact, edges)
        assert_region_bytes(scan, restated_regions(pops, rows, edges, spheres), "%s scan against the restatement" % name)
        try:
            for cap in (0, 1, 3, 3 * (depth - 1), 3 * depth - 1):
                g.DebugQueryStackCap(cap)
                label = "%s mm=%d edges=%d cap=%d" % (name, math_mode, edges, cap)
                print("%s: lanes whose restated walk holds more than %d entries: %s"
                      % (label, cap, ", ".join("%s %d of %d" % (k, int((m > cap).sum()), m.shape[0]) for k, m in marks.items())))
                assert g.QueryAccelUpdateInfo()["stack_entries"] == min(cap, 3 * depth)
                got = answers(g, pops)
                check_answers(got, scan, pops, rows, orc, spheres, contract, label, exact, edges)
        finally:
            g.DebugQueryStackCap(None)
        assert same_answers(answers(g, pops), before), name             # the product again, byte for byte
        g.close()


def region_marks(nodes, recs, info, pops, rows, spheres):
    """({walk: the most stack entries each lane's restated walk holds}, every fourth box and query triangle, for region_bvh_kernel
    (boxes, triangles) and tridistance_bvh_kernel, every sweep for spherecast_bvh_kernel; and, as a cross-check of the sweep
    walk's marks that no restated walk is needed for, the sweeps whose box (both ends, widened by the radius) meets more than one
    child of the root)."""
    from query_accel_expect import EMPTY
    out = {}
    boxes, tris, sw = pops["boxes"][::4], pops["tris"][::4], pops["sweeps"]
    with np.errstate(all="ignore"):
        for key, walk in (("overlap16", lambda st: oe.walk_tree_overlap(nodes, recs, info, boxes, rows, 16, spheres=spheres, stats=st)),
                          ("trioverlap16", lambda st: te.walk_tree_triangles(nodes, recs, info, tris, rows, 16, spheres=spheres, stats=st)),
                          ("tridistance", lambda st: td.walk_tree_tridistance(nodes, recs, info, tris, rows, spheres=spheres, stats=st)),
                          ("spherecast", lambda st: spe.walk_tree_spherecast(nodes, recs, info, sw, rows, spheres=spheres, stats=st))):
            stats = {}
            walk(stats)
            out[key] = np.asarray(stats["high_water_per"])
        a, b = sw[:, :3], sw[:, :3] + sw[:, 3:6]
        lo, hi = np.minimum(a, b) - sw[:, 6:7], np.maximum(a, b) + sw[:, 6:7]
        root = nodes[0]
        met = ((root["lo"][None] <= hi[:, :, None]) & (root["hi"][None] >= lo[:, :, None])).all(axis=1) & (root["child"] != EMPTY)[None]
    return out, met.sum(axis=1) > 1


def restated_marks(orc, nodes, recs, info, pops, rows, spheres):
    """{walk: the most stack entries each lane's restated walk holds}: a device lane whose capacity is below its mark overflows."""
    from allhits_expect import walk_tree_all_hits
    from occluded_expect import walk_tree_occluded
    out = {}
    rays, segs = pops["rays"][::max(1, pops["rays"].shape[0] // 48)], pops["segs"][::max(1, pops["segs"].shape[0] // 48)]
    expo = ee.exposure_segments(pops["exposure"], pops["dirs"])[::16]
    with np.errstate(all="ignore"):
        for key, walk in (("closest", lambda st: ce.walk_tree_closest(nodes, recs, info, pops["points"], rows, spheres=spheres, stats=st)),
                          ("nearest16", lambda st: ne.walk_tree_nearest(nodes, recs, info, pops["points"], rows, 16, spheres=spheres, stats=st)),
                          ("intersect", lambda st: walk_tree(orc, nodes, recs, info, rays, rows, stats=st)),
                          ("occluded", lambda st: walk_tree_occluded(orc, nodes, recs, info, segs, rows, spheres, stats=st, kernel_order=True)),
                          ("all16", lambda st: walk_tree_all_hits(orc, nodes, recs, info, segs, rows, 16, spheres, stats=st)),
                          ("exposure", lambda st: walk_tree_occluded(orc, nodes, recs, info, expo, rows, spheres, stats=st, kernel_order=True))):
            stats = {}
            got = walk(stats)
            out[key] = np.asarray(stats["high_water_per"])
            if key in ("occluded", "exposure"):                          # an any-hit lane ends at its first occluder, a sphere's
                batch = segs if key == "occluded" else expo              # before the root: the lanes that stay open walk the tree
                out[key + ", open lanes"] = out[key][~got[0] & (batch[:, 6] <= batch[:, 7])]
    return out


def test_a_shortened_stack_on_an_empty_scene_and_on_spheres_alone(orc):
    pops = scene_pops(adversarial_scene(37, 3), 9, 40)
    for spheres in (None, ADV_SPHERES):
        g = _tracer()                                                     # no upload: no triangle, no node
        if spheres is not None:
            g.UploadSpheres(spheres)
        scan, before = scan_and_tree(g, pops)
        assert same_answers(before, scan) and g.QueryAccelInfo()["nodes"] == 0
        if spheres is None:
            assert (scan["intersect"]["prim"] == -1).all() and not scan["occluded"].any() and (scan["closest"]["prim"] == -1).all()
        else:
            assert (scan["intersect"]["prim"] >= 0).any() and scan["occluded"].any() and (scan["closest"]["prim"] >= 0).any()
        for cap in (0, 1):
            g.DebugQueryStackCap(cap)
            assert same_answers(answers(g, pops), scan), cap
        g.DebugQueryStackCap(None)
        assert same_answers(answers(g, pops), scan)
        g.close()


# ---- 4. a multi-device handle ------------------------------------------------------------------------------------------------------

def test_the_hook_forwards_through_a_multi_device_handle(orc):
    import raytracertest_amd as R
    rows, pops = dc.deep_scene(mirror=True), deep_pops(True)
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    scan, before = scan_and_tree(m, pops)
    assert m.QueryAccelInfo()["depth"] == dc.DEPTH_BOUND
    assert m.QueryAccelUpdateInfo()["stack_entries"] == 3 * dc.DEPTH_BOUND     # what the first band's walks run with
    check_answers(before, scan, pops, rows, orc, label="two bands, product")
    m.DebugQueryStackCap(0)
    assert m.QueryAccelUpdateInfo()["stack_entries"] == 0                      # the cap reached the band that answers
    check_answers(answers(m, pops), scan, pops, rows, orc, label="two bands, cap 0")
    m.DebugQueryStackCap(5)
    assert m.QueryAccelUpdateInfo()["stack_entries"] == 5
    m.DebugQueryStackCap(None)
    assert m.QueryAccelUpdateInfo()["stack_entries"] == 3 * dc.DEPTH_BOUND
    assert same_answers(answers(m, pops), before)
    m.close()
