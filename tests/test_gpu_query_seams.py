"""The six scan-mode query kernels (query_kernel, occluded_kernel, exposure_kernel, allhits_kernel, closest_kernel,
nearest_kernel) at the seams of their LDS chunks of kQueryChunk = 1024 records, on the scenes of seam_cases.py: 1023, 1024,
1025, 2048 and 2049 triangles, whose decisive records are the last of a chunk, the first of the next and the last of the scene
(test_seam_cases.py asserts that without a device, with a reference that loses such a record as its teeth).  Every scan-mode
answer is compared byte for byte with the oracle's brute force or the numpy restatement, no ray excluded; then the same
populations go through the BVH kernels on the same tracer under each query's own check, the targeted ones without an exclusion.
spherecast_kernel and tridistance_kernel carry a running best through the same chunk loop: their sweeps and query triangles
(seam_cases.sweep_batch, triangle_batch) are compared with the numpy restatements' winners through the scan and the tree, which
equal each other by construction, so no row has an exclusion.  Last, the K that query_k() picks on its own at 524 288 and
1 048 576 rays, which every other test forces."""
import numpy as np
import pytest

import closest_expect as ce
import exposure_expect as ee
import nearest_expect as ne
import seam_cases as sc
import signed_expect as se
import spherecast_expect as spe
import tridistance_expect as td
from allhits_expect import check_bvh_all_hits, expected_all_hits, hit_table_uv, same_rows, sets_from_table, truncated
from lattice_cases import ray_segments
from occluded_expect import check_bvh_occluded, expected_occluded, interval_families
from query_accel_expect import EXCLUSION_CAP, check_against_scan
from query_expect import HIT_DTYPE, adversarial_rays, adversarial_scene, edge_rows, expected_hits, same_hits
from trioverlap_expect import queries_of

pytestmark = pytest.mark.gpu

MAX_HITS = (1, 3, 4, 5, 8, 16)
NEAREST_HITS = (1, 4, 5, 16)
_cache = {}

sizes = pytest.mark.parametrize("n_tris", sc.SIZES)
modes = pytest.mark.parametrize("math_mode", [0, 1])
uploads = pytest.mark.parametrize("edges", [False, True])


def oc(orc, math_mode):
    return orc.FMA if math_mode == 0 else orc.STRICT


def _tracer(math_mode=0, nearest=False, **kw):
    import raytracertest_amd as R
    return R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)


def _upload(g, rows, edges):
    assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _with_spheres(table, sph):
    return tuple(np.c_[a, b] for a, b in zip(table, sph))


def case(orc, n_tris, math_mode):
    """The scene in both layouts, its populations and the oracle's hit tables under one arithmetic contract, made once per
    session.  The tables are the stack layout's; the tie layout's follow from them (seam_cases.tie_table: record S is record
    S - 1 again, which test_seam_cases.py checks against the oracle itself)."""
    key = (n_tris, math_mode)
    if key in _cache:
        return _cache[key]
    from raytracertest_amd import api
    contract = oc(orc, math_mode)
    c = {"contract": contract, "n_tris": n_tris, "rows": {}, "info": {}, "table": {}, "expo_table": {}, "hits": {}}
    for layout in sc.layouts(n_tris):
        c["rows"][layout], c["info"][layout] = sc.seam_scene(n_tris, layout)
        c["rows"][layout].setflags(write=False)
    rows = c["rows"]["stack"]
    c["rays"], c["idx"], c["distinct"], c["tags"] = sc.ray_batch(n_tris, rows)
    c["segs"], c["sidx"], c["stags"] = sc.segment_batch(n_tris, rows)
    c["pts"], c["ptags"] = sc.point_batch(n_tris, rows)
    c["expo"] = sc.exposure_points(n_tris)
    c["dirs"] = ee.as_dirs4(api.hemisphere_directions(64))
    c["expo_segs"] = ee.exposure_segments(c["expo"][:4], c["dirs"])      # (the fifth point is the first again)
    c["table"]["stack"] = hit_table_uv(orc, c["distinct"], rows, None, contract)
    c["expo_table"]["stack"] = hit_table_uv(orc, c["expo_segs"], rows, None, contract)
    if "tie" in c["rows"]:
        c["table"]["tie"] = sc.tie_table(c["table"]["stack"], c["info"]["tie"])
        c["expo_table"]["tie"] = sc.tie_table(c["expo_table"]["stack"], c["info"]["tie"])
    _cache[key] = c
    return c


def sphere_tables(orc, c):
    """The stack layout's tables with the columns of seam_cases.SPHERES appended, once per case."""
    if "sph" not in c:
        none = c["rows"]["stack"][:0]
        c["sph"] = {"table": _with_spheres(c["table"]["stack"], hit_table_uv(orc, c["distinct"], none, sc.SPHERES, c["contract"])),
                    "expo_table": _with_spheres(c["expo_table"]["stack"], hit_table_uv(orc, c["expo_segs"], none, sc.SPHERES, c["contract"]))}
    return c["sph"]


def hits_of(orc, c, layout, nearest, spheres=None):
    """expected_hits of the distinct rays, once per (case, layout, hit rule)."""
    key = (layout, nearest, spheres is not None)
    if key not in c["hits"]:
        c["hits"][key] = expected_hits(orc, c["distinct"], c["rows"][layout], spheres, c["contract"], nearest)
        c["hits"][key].setflags(write=False)
    return c["hits"][key]


def targeted(tags, idx=None):
    """The batch positions whose ray (or segment, or point) is aimed at a seam."""
    kinds = [tags[j][0] for j in idx] if idx is not None else [t[0] for t in tags]
    return np.array([k not in ("adversarial", "general") for k in kinds])


# ---- Intersect --------------------------------------------------------------------------------------------------------------

@uploads
@modes
@sizes
def test_intersect_names_the_records_on_the_seams(orc, n_tris, math_mode, edges):
    c = case(orc, n_tris, math_mode)
    rays, idx, tags = c["rays"], c["idx"], c["tags"]
    aimed = targeted(tags, idx)
    for layout in sc.layouts(n_tris):
        rows, info = c["rows"][layout], c["info"][layout]
        up = edge_rows(rows) if edges else rows
        for nearest in (False, True):
            exp = hits_of(orc, c, layout, nearest)[idx]
            for K in (1, 2, 4):
                label = "n=%d %s mm=%d edges=%d nearest=%d K=%d" % (n_tris, layout, math_mode, edges, nearest, K)
                g = _tracer(math_mode, nearest, samples_in_flight=K)
                _upload(g, rows, edges)
                with np.errstate(all="ignore"):
                    for n in (sc.N_RAYS_LONG, sc.N_RAYS, 1):             # a partial last block for every K
                        got = g.Intersect(rays[:n])
                        bad = np.nonzero((_bits(got).reshape(-1, 4) != _bits(exp[:n]).reshape(-1, 4)).any(axis=1))[0]
                        assert got.dtype == HIT_DTYPE and bad.size == 0, (label, n, bad[:5], rays[bad[:5]], got[bad[:5]], exp[bad[:5]])
                    got = g.Intersect(rays)
                    assert same_hits(got, exp), label
                    # the designated winners, by name
                    for j in np.nonzero(aimed)[0]:
                        kind, S, i = tags[idx[j]]
                        twin = info["seams"][S]["tie"]
                        if kind in ("front", "centroid") and not (twin and i == S):
                            assert got["prim"][j] == i, (label, kind, i, got[j])          # S - 1 of a twin pair, n_tris - 1, ...
                        elif kind in ("front", "centroid"):
                            assert got["prim"][j] == -1, (label, "the twin's empty place", got[j])
                        elif kind == "behind" and not (twin and i == S):
                            assert got["prim"][j] == (-1 if nearest else i), (label, kind, i, got[j])
                    assert (got["prim"][aimed] == info["last"]).any() == info["applies"]["last"], label
                    if K == 1:                                           # the same tracer through the tree
                        g.SetQueryAcceleration(True)
                        bvh = g.Intersect(rays[:sc.N_RAYS])
                        check_against_scan(bvh, got[:sc.N_RAYS], rays[:sc.N_RAYS], up, edges, label="bvh " + label)
                        a = aimed[:sc.N_RAYS]
                        assert same_hits(bvh[a], got[:sc.N_RAYS][a]), (label, "a targeted ray used the exclusion")
                        assert g.QueryAccelInfo()["valid"] == 1
                g.close()


# ---- Occluded ---------------------------------------------------------------------------------------------------------------

@uploads
@modes
@sizes
def test_occluded_finishes_in_the_chunk_the_occluder_is_in(orc, n_tris, math_mode, edges):
    c = case(orc, n_tris, math_mode)
    contract = c["contract"]
    segs, sidx, stags = c["segs"], c["sidx"], c["stags"]
    aimed = targeted(stags)
    for layout in sc.layouts(n_tris):
        rows, (hit, t) = c["rows"][layout], c["table"][layout][:2]
        exp = expected_occluded(orc, segs, rows, None, contract, (hit[sidx], t[sidx]))
        fams = interval_families(c["rays"][:sc.N_RAYS], 5 + n_tris)
        ridx = c["idx"][:sc.N_RAYS]
        for K in (1, 2, 4):
            label = "n=%d %s mm=%d edges=%d K=%d" % (n_tris, layout, math_mode, edges, K)
            g = _tracer(math_mode, samples_in_flight=K)
            _upload(g, rows, edges)
            with np.errstate(all="ignore"):
                for n in (segs.shape[0], 257, 1):
                    got = g.Occluded(segs[:n])
                    bad = np.nonzero(got != exp[:n])[0]
                    assert bad.size == 0, (label, n, bad[:5], segs[bad[:5]], [stags[j] for j in bad[:5]])
                for name, s in fams.items():
                    want = expected_occluded(orc, s, rows, None, contract, (hit[ridx], t[ridx]))
                    assert np.array_equal(g.Occluded(s), want), (label, name)
                if layout == "stack":
                    # one open ray per block that only the scene's last record finishes; every other ray finishes in chunk 0
                    B = 256 * K
                    b = min(1, sc.LATE // B - 1)
                    for position in (300, b * B, b * B + B - 1, None):   # somewhere, the first and the last lane of a block, nowhere
                        late, lidx = sc.late_finisher(n_tris, rows, position)
                        want = expected_occluded(orc, late, rows, None, contract, (hit[lidx], t[lidx]))
                        got = g.Occluded(late)
                        assert want.all() and np.array_equal(got, want), (label, position, np.nonzero(got != want)[0][:5])
                if K == 1:                                               # the same tracer through the tree
                    scan = g.Occluded(segs)
                    g.SetQueryAcceleration(True)
                    bvh = g.Occluded(segs)
                    check_bvh_occluded(bvh, scan, segs, rows, orc, None, contract, table=(hit[sidx], t[sidx]), cap=EXCLUSION_CAP, label="bvh " + label)
                    assert np.array_equal(bvh[aimed], scan[aimed]), (label, "a targeted segment used the exclusion")
            g.close()


# ---- IntersectAll -----------------------------------------------------------------------------------------------------------

@uploads
@modes
@sizes
def test_intersect_all_merges_the_hits_of_two_chunks(orc, n_tris, math_mode, edges):
    c = case(orc, n_tris, math_mode)
    segs, sidx, stags = c["segs"], c["sidx"], c["stags"]
    aimed = targeted(stags)
    stack_rows = [j for j, tg in enumerate(stags) if tg[0] == "turns" and c["tags"][sidx[j]][0] == "stack_front" and segs[j, 7] == np.inf]
    assert stack_rows
    for layout in sc.layouts(n_tris):
        rows, info, table = c["rows"][layout], c["info"][layout], c["table"][layout]
        label = "n=%d %s mm=%d edges=%d" % (n_tris, layout, math_mode, edges)
        exp16 = expected_all_hits(table, segs, 16, sidx)
        g = _tracer(math_mode)
        _upload(g, rows, edges)
        got = {}
        with np.errstate(all="ignore"):
            for m in MAX_HITS:
                exp = truncated(exp16, m)
                got[m] = g.IntersectAll(segs, m)
                bad = ne.differing_rows(got[m][0], exp[0], got[m][1], exp[1])
                assert same_rows(got[m], exp), (label, m, bad[:5], [stags[j] for j in bad[:5]], got[m][0][bad[:2]], exp[0][bad[:2]])
            for n in (257, 1):
                assert same_rows(g.IntersectAll(segs[:n], 5), (exp16[0][:n, :5], np.minimum(exp16[1][:n], 5))), (label, n)
            for j in stack_rows:                                         # by name: a stack's row, the cut on the seam, the twins
                S = c["tags"][sidx[j]][1]
                mem = [i for i in sc.members(n_tris, S)]
                twin = info["seams"][S]["tie"]
                prims = got[16][0]["prim"][j, :got[16][1][j]].tolist()
                ts = got[16][0]["t"][j, :got[16][1][j]]
                if not twin:
                    assert prims == mem[::-1] and (np.diff(ts) > 0).all(), (label, prims)    # ascending t = descending index
                    if len(mem) == 8:
                        assert got[4][0]["prim"][j].tolist() == [S + 3, S + 2, S + 1, S], (label, got[4][0][j])
                else:
                    assert sorted(prims) == mem and prims.index(S) == prims.index(S - 1) + 1 and ts[prims.index(S)] == ts[prims.index(S - 1)], (label, prims)
            for j, tg in enumerate(stags):
                if tg[0] == "closed_tie" and info["seams"][tg[1]]["tie"] and tg[2] == tg[1] - 1:
                    assert got[16][1][j] == 2 and got[16][0]["prim"][j, :2].tolist() == [tg[1] - 1, tg[1]], (label, got[16][0][j, :3])
                    assert got[1][0]["prim"][j, 0] == tg[1] - 1
            g.SetQueryAcceleration(True)                                 # the same tracer through the tree
            E, W = sets_from_table(table, segs, rows, sidx)
            for m in (4, 16):
                bvh = g.IntersectAll(segs, m)
                check_bvh_all_hits(bvh, got[m], E, W, m, cap=EXCLUSION_CAP, label="bvh %s max_hits=%d" % (label, m))
                assert same_rows((bvh[0][aimed], bvh[1][aimed]), (got[m][0][aimed], got[m][1][aimed])), (label, m, "a targeted segment used the exclusion")
        g.close()


# ---- ClosestPoint, ClosestAll, SignedDistance ---------------------------------------------------------------------------------

def point_refs(n_tris, layout, edges):
    """What the point queries must answer on one layout and upload format, from the numpy restatements, once per session (the
    point queries do not depend on the arithmetic mode): ClosestPoint's records, the cursor on the twins, ClosestAll's rows
    without and with it, and the sides of ClosestPoint's records from the table the library reports for the upload."""
    key = ("points", n_tris, layout, edges)
    if key not in _cache:
        from raytracertest_amd import api
        pts, tags = sc.point_batch(n_tris, sc.seam_scene(n_tris)[0])
        rows, info = sc.seam_scene(n_tris, layout)
        up = edge_rows(rows) if edges else rows
        tab = ce.table(pts, up, edges)
        order = ne.presort(tab)
        exp = ce.winners(tab, pts[:, 3])
        after = sc.tie_cursor(pts, tags, exp)
        rows_of = {(m, cur): ne.expected_all(tab, pts[:, 3], m, after if cur else None, order) for m in NEAREST_HITS for cur in (False, True)}
        sides = se.expected_sides(pts, exp, up, api.feature_normals(up, edges), edges)
        _cache[key] = {"rows": rows, "info": info, "pts": pts, "tags": tags, "exp": exp, "after": after, "all": rows_of, "sides": sides}
    return _cache[key]


@uploads
@modes
@sizes
def test_point_queries_find_the_records_on_the_seams(n_tris, math_mode, edges):
    for layout in sc.layouts(n_tris):
        r = point_refs(n_tris, layout, edges)
        rows, info, pts, tags, exp, after = r["rows"], r["info"], r["pts"], r["tags"], r["exp"], r["after"]
        label = "n=%d %s mm=%d edges=%d" % (n_tris, layout, math_mode, edges)
        assert (after["prim"] >= 0).any() == (n_tris > 1023)            # (at 1023 there is no record S - 1: every cursor is none)
        g = _tracer(math_mode)
        _upload(g, rows, edges)
        with np.errstate(all="ignore"):
            for accel in (False, True):                                  # the scan, then the same tracer through the tree: the same bytes
                g.SetQueryAcceleration(accel)
                lab = "%s accel=%d" % (label, accel)
                got = g.ClosestPoint(pts)
                assert ce.same_hits(got, exp), (lab, ce.differing(got, exp)[:5], [tags[j] for j in ce.differing(got, exp)[:5]])
                for n in (257, 1):
                    assert ce.same_hits(g.ClosestPoint(pts[:n]), exp[:n]), (lab, n)
                for j, (kind, S, i) in enumerate(tags):                  # by name
                    if kind in ("near", "under"):
                        twin = info["seams"][S]["tie"]
                        want = S - 1 if (twin and i == S - 1) else (None if (twin and i == S) else i)
                        assert want is None or got["prim"][j] == want, (lab, kind, i, got[j])
                for m in NEAREST_HITS:
                    for cur in (False, True):
                        want = r["all"][(m, cur)]
                        rows_, counts = g.ClosestAll(pts, m, after=after if cur else None)
                        bad = ne.differing_rows(rows_, want[0], counts, want[1])
                        assert bad.size == 0, (lab, m, cur, bad[:5], [tags[j] for j in bad[:5]], rows_[bad[:2]], want[0][bad[:2]])
                        if cur:                                          # the continuation starts with the twin, from the next chunk
                            for j in np.nonzero(after["prim"] >= 0)[0]:
                                S = tags[j][1]
                                if info["seams"][S]["tie"]:
                                    assert rows_["prim"][j, 0] == S and rows_["t"][j, 0] == after["t"][j], (lab, m, rows_[j, :2])
                hits, sides = g.SignedDistance(pts)
                assert ce.same_hits(hits, got), lab                      # ClosestPoint's bytes
                bad = np.nonzero((_bits(sides).reshape(-1, 2) != _bits(r["sides"]).reshape(-1, 2)).any(axis=1))[0]
                assert se.same_sides(sides, r["sides"]), (lab, bad[:5], [tags[j] for j in bad[:5]])
        g.close()


# ---- SphereCast, TriangleDistance -------------------------------------------------------------------------------------------

def _append_columns(tab, more):
    return tuple(np.concatenate([a, b], axis=1) for a, b in zip(tab, more))


def swept_refs(n_tris, edges):
    """The sweeps and query triangles of the seams and the restatements' tables of the STACK layout in one upload format, once
    per session (neither query depends on the arithmetic mode); the tie layout's tables follow from them (seam_cases.tie_table,
    which test_seam_cases.py checks against the restatement itself)."""
    key = ("swept", n_tris, edges)
    if key not in _cache:
        rows = sc.seam_scene(n_tris)[0]
        up = edge_rows(rows) if edges else rows
        sw, stags = sc.sweep_batch(n_tris, rows)
        q, qtags = sc.triangle_batch(n_tris, rows)
        for a in (sw, q):
            a.setflags(write=False)
        _cache[key] = {"sweeps": sw, "stags": stags, "queries": q, "qtags": qtags, "sweep_table": sc.sweep_table(sw, up, edges),
                       "triangle_table": sc.triangle_table(q, up, edges)}
    return _cache[key]


def _named(kind, S, i, twin):
    """The primitive a targeted sweep or query triangle must name (None: no claim): its tag's on the stack layout; on the tie
    layout the twin's own place is empty for a sweep, and a stack whose highest petal was the twin has S - 1 on top."""
    if kind == "general":
        return None
    if twin and i == S:
        return -1 if kind in ("down", "up", "start", "cut") else S - 1 if kind in ("axis_down", "beside") else None
    return i


def _check_names(prim, tags, info, label):
    for j, (kind, S, i) in enumerate(tags):
        want = _named(kind, S, i, kind != "general" and info["seams"][S]["tie"])
        assert want is None or prim[j] == want, (label, kind, S, i, prim[j])


def _swept_case(n_tris, edges, query):
    """-> per layout: rows, info, the batch, its tags and the layout's table."""
    r = swept_refs(n_tris, edges)
    batch, tags, tab = (r["sweeps"], r["stags"], r["sweep_table"]) if query == "sweep" else (r["queries"], r["qtags"], r["triangle_table"])
    for layout in sc.layouts(n_tris):
        rows, info = sc.seam_scene(n_tris, layout)
        yield layout, rows, info, batch, tags, (tab if layout == "stack" else sc.tie_table(tab, info))


@uploads
@sizes
def test_sphere_cast_finds_the_records_on_the_seams(n_tris, edges):
    for layout, rows, info, sw, tags, tab in _swept_case(n_tris, edges, "sweep"):
        exp = sc.sweep_winners(tab, sw)
        _check_names(exp["prim"], tags, info, "the restatement")
        blobs = set()
        for math_mode in ((0, 1) if n_tris == 2049 else (0,)):           # the arithmetic mode must not change a byte
            g = _tracer(math_mode)
            _upload(g, rows, edges)
            with np.errstate(all="ignore"):
                for accel in (False, True):                              # the scan, then the same tracer through the tree: the same bytes
                    g.SetQueryAcceleration(accel)
                    lab = "n=%d %s mm=%d edges=%d accel=%d" % (n_tris, layout, math_mode, edges, accel)
                    got = g.SphereCast(sw)
                    bad = ce.differing(got, exp)
                    assert got.dtype == HIT_DTYPE and bad.size == 0, (lab, bad[:5], [tags[j] for j in bad[:5]], got[bad[:3]], exp[bad[:3]])
                    for n in (257, 1):
                        assert ce.same_hits(g.SphereCast(sw[:n]), exp[:n]), (lab, n)
                    _check_names(got["prim"], tags, info, lab)
                    blobs.add(got.tobytes())
            g.close()
        assert len(blobs) == 1


@uploads
@sizes
def test_triangle_distance_finds_the_records_on_the_seams(n_tris, edges):
    for layout, rows, info, q, tags, tab in _swept_case(n_tris, edges, "triangle"):
        exp = sc.triangle_winners(tab, q[:, 3])
        _check_names(exp[0]["prim"], tags, info, "the restatement")
        blobs = set()
        for math_mode in ((0, 1) if n_tris == 2049 else (0,)):
            g = _tracer(math_mode)
            _upload(g, rows, edges)
            with np.errstate(all="ignore"):
                for accel in (False, True):
                    g.SetQueryAcceleration(accel)
                    lab = "n=%d %s mm=%d edges=%d accel=%d" % (n_tris, layout, math_mode, edges, accel)
                    got = g.TriangleDistance(q)
                    bad = td.differing(got, exp)
                    assert got[0].dtype == HIT_DTYPE and got[1].dtype == td.WITNESS_DTYPE and td.same(got, exp), \
                        (lab, bad[:5], [tags[j] for j in bad[:5]], got[0][bad[:3]], exp[0][bad[:3]], got[1][bad[:3]], exp[1][bad[:3]])
                    for n in (257, 1):
                        assert td.same(g.TriangleDistance(q[:n]), (exp[0][:n], exp[1][:n])), (lab, n)
                    _check_names(got[0]["prim"], tags, info, lab)
                    blobs.add(got[0].tobytes() + got[1].tobytes())
            g.close()
        assert len(blobs) == 1


def over_the_third_sphere():
    """One query triangle whose nearest corner is 1/16 above the top of seam_cases.SPHERES[2]."""
    x, y, z, r = sc.SPHERES[2].tolist()
    return td.with_radius(queries_of([[[x, y, z + r + 0.0625], [x + 0.03125, y, z + r + 0.125], [x, y + 0.03125, z + r + 0.125]]]), np.inf)


# ---- Exposure ---------------------------------------------------------------------------------------------------------------

@uploads
@modes
@sizes
def test_exposure_masks_are_the_oracles_complement(orc, n_tris, math_mode, edges):
    c = case(orc, n_tris, math_mode)
    contract, pts, dirs, segs = c["contract"], c["expo"], c["dirs"], c["expo_segs"]
    which = np.array([0, 1, 2, 3, 0])                                    # the fifth point is the first
    for layout in sc.layouts(n_tris):
        rows, (hit, t) = c["rows"][layout], c["expo_table"][layout][:2]
        label = "n=%d %s mm=%d edges=%d" % (n_tris, layout, math_mode, edges)
        occ = expected_occluded(orc, segs, rows, None, contract, (hit, t)).reshape(4, 64)       # the oracle's, not the device's
        g = _tracer(math_mode)
        _upload(g, rows, edges)
        with np.errstate(all="ignore"):
            for n_dirs in (1, 63, 64):
                for batch in (1, 3, 4, 5):                               # four points to a block: padding waves still stage
                    want = ee.pack_masks(~occ[which[:batch], :n_dirs])
                    got = g.Exposure(pts[:batch], dirs[:n_dirs])
                    assert got.dtype == np.uint64 and np.array_equal(got, want), (label, n_dirs, batch, got, want)
            if c["info"][layout]["applies"]["last"]:
                last_only = (hit & (segs[:, 6:7] <= t) & (t <= segs[:, 7:8])).reshape(4, 64, -1)[0]
                assert (last_only[:, c["info"][layout]["last"]] & (last_only.sum(axis=1) == 1)).any() and (~occ[0]).any(), label
            g.SetQueryAcceleration(True)                                 # the same tracer through the tree: Exposure == ~Occluded
            all5 = ee.exposure_segments(pts, dirs)
            bvh_occ = g.Occluded(all5)
            assert np.array_equal(g.Exposure(pts, dirs), ee.pack_masks(~bvh_occ.reshape(5, 64))), label
            table5 = (hit.reshape(4, 64, -1)[which].reshape(320, -1), t.reshape(4, 64, -1)[which].reshape(320, -1))
            check_bvh_occluded(bvh_occ, occ[which].reshape(-1), all5, rows, orc, None, contract, table=table5, cap=EXCLUSION_CAP, label="bvh " + label)
            inside = table5[0] & (all5[:, 6:7] <= table5[1]) & (table5[1] <= all5[:, 7:8])
            filler = np.setdiff1d(np.arange(n_tris), sorted(c["info"][layout]["seam_of"]))
            aimed = ~inside[:, filler].any(axis=1)                       # open, or blocked by petals alone
            assert np.array_equal(bvh_occ[aimed], occ[which].reshape(-1)[aimed]), (label, "a targeted direction used the exclusion")
        g.close()


# ---- spheres behind a seam-sized n_tris -----------------------------------------------------------------------------------------

@modes
@pytest.mark.parametrize("n_tris", [1025, 2049])
def test_spheres_are_numbered_from_a_seam_sized_n_tris(orc, n_tris, math_mode):
    c = case(orc, n_tris, math_mode)
    contract, rows, sph = c["contract"], c["rows"]["stack"], sc.SPHERES
    st = sphere_tables(orc, c)
    table, (ehit, et) = st["table"], st["expo_table"][:2]
    rays, idx, segs, sidx, pts = c["rays"], c["idx"], c["segs"], c["sidx"], c["pts"]
    label = "n=%d mm=%d spheres" % (n_tris, math_mode)
    with np.errstate(all="ignore"):
        for nearest in (False, True):
            exp = hits_of(orc, c, "stack", nearest, sph)[idx]
            # of two coincident spheres the first; they lie in front of the stack, so only the nearest-hit rule names them
            assert (exp["prim"] == n_tris).any() == nearest and not (exp["prim"] == n_tris + 1).any()
            for K in (1, 4):
                g = _tracer(math_mode, nearest, samples_in_flight=K)
                _upload(g, rows, False)
                g.UploadSpheres(sph)
                assert same_hits(g.Intersect(rays), exp), (label, nearest, K)
                if nearest or K == 4:
                    g.close()
                    continue
                want = expected_occluded(orc, segs, rows, sph, contract, (table[0][sidx], table[1][sidx]))
                assert np.array_equal(g.Occluded(segs), want), label
                exp16 = expected_all_hits(table, segs, 16, sidx)
                assert (exp16[0]["prim"] >= n_tris).any()
                for m in (4, 16):
                    assert same_rows(g.IntersectAll(segs, m), truncated(exp16, m)), (label, m)
                tab = ce.table(pts, rows, False, sph)
                assert ce.same_hits(g.ClosestPoint(pts), ce.winners(tab, pts[:, 3])), label
                near4 = ne.expected_all(tab, pts[:, 3], 4)
                got4 = g.ClosestAll(pts, 4)
                assert ne.differing_rows(got4[0], near4[0], got4[1], near4[1]).size == 0 and (near4[0]["prim"] >= n_tris).any(), label
                occ = expected_occluded(orc, c["expo_segs"], rows, sph, contract, (ehit, et)).reshape(4, 64)
                assert np.array_equal(g.Exposure(c["expo"], c["dirs"]), ee.pack_masks(~occ[[0, 1, 2, 3, 0]])), label
                # the sweeps and query triangles: the down sweep of petal 1020 meets the third sphere first, the sweep down the axis
                # of seam 1024 the first of the coincident pair; one more triangle sits 1/16 above the third sphere
                r = swept_refs(n_tris, False)
                sw, q = r["sweeps"], np.concatenate([r["queries"], over_the_third_sphere()])
                swept = sc.sweep_winners(_append_columns(r["sweep_table"], spe.table(sw, None, spheres=sph)), sw)
                assert ce.same_hits(g.SphereCast(sw), swept) and {n_tris, n_tris + 2} <= set(swept["prim"].tolist()), label
                assert swept["prim"][sc.find(r["stags"], "down", 1024, 1020)[0]] == n_tris + 2
                tab = _append_columns(tuple(np.concatenate([a, b]) for a, b in zip(r["triangle_table"], sc.triangle_table(q[-1:], rows))),
                                      sc.triangle_table(q, None, spheres=sph))
                near = sc.triangle_winners(tab, q[:, 3])
                assert td.same(g.TriangleDistance(q), near), label
                assert near[0]["prim"][-1] == n_tris + 2 and near[0]["t"][-1] == np.float32(0.0625) ** 2, label
                g.close()


# ---- the K nobody asks for ------------------------------------------------------------------------------------------------------

def test_the_automatic_k_answers_like_the_forced_ones(orc):
    """query_k() (csrc/rt_query_api.hpp): kResidentLanes = 256 * 4 * 256 = 262 144; K = 2 from 2 * kResidentLanes = 524 288 rays,
    K = 4 from 4 * kResidentLanes = 1 048 576.  The tracer is made with the default samples_in_flight, and the batch lengths
    sit on and beside both thresholds; 4099 is prime, so over the tiles every ray of the population lands in many lanes and
    many of a lane's K slots."""
    rows = adversarial_scene(3, 17, behind=False)
    assert rows.shape[0] == 9
    rays = adversarial_rays(rows, 4099, 19)[-4099:]
    segs = ray_segments(rays)
    table = hit_table_uv(orc, rays, rows)
    occ = expected_occluded(orc, segs, rows, None, None, (table[0], table[1]))
    assert occ.any() and not occ.all()
    for nearest in (False, True):
        exp = expected_hits(orc, rays, rows, None, None, nearest)
        assert (exp["prim"] >= 0).any() and (exp["prim"] < 0).any()
        g = _tracer(0, nearest)                                          # samples_in_flight: the default, 0
        assert g.UploadScene(rows)
        with np.errstate(all="ignore"):
            for n in (524287, 524288, 1048575, 1048576, 1048577):
                tile = np.arange(n) % 4099
                got = g.Intersect(np.ascontiguousarray(rays[tile]))
                bad = np.nonzero((_bits(got).reshape(-1, 4) != _bits(exp[tile]).reshape(-1, 4)).any(axis=1))[0]
                assert bad.size == 0, (nearest, n, bad.size, bad[:5], got[bad[:5]], exp[tile][bad[:5]])
                if not nearest:                                          # (the hit rule plays no part in Occluded)
                    got = g.Occluded(np.ascontiguousarray(segs[tile]))
                    bad = np.nonzero(got != occ[tile])[0]
                    assert bad.size == 0, (n, bad.size, bad[:5])
        g.close()
