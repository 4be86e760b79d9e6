"""The eight newer queries on the device at the ends of fp32's range (tests/range_cases.py): one scene of 300 triangles (slivers,
a segment, a point, one record with a NaN), three spheres and its query populations, all multiplied by 2^k.  At every k of
range_cases.TREE_KS -- inside the invariance ranges, beyond them, down to where squared distances are subnormal or zero and up
to where they are +inf -- in both layouts and both math modes: the device scan gives the numpy restatement's bytes, every row
(denormals are kept: correctly rounded division and square root on subnormal operands and results, fminf and fmaxf), and the
device tree gives the device scan's bytes, every row, SphereCast's included (its walk's range guard)."""
import numpy as np
import pytest

import closest_expect as ce
import range_cases as rc
import signed_expect as sg
from query_expect import edge_rows

pytestmark = pytest.mark.gpu

TINY = np.float32(np.finfo(np.float32).tiny)


def _tracer(math_mode):
    import raytracertest_amd as R
    return R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode)


def device_answers(g, pops):
    """{query: list of arrays}, in range_cases.brute_force's shapes."""
    m = rc.MAX_HITS
    with np.errstate(all="ignore"):
        return {"closest": [g.ClosestPoint(pops["points"])], "nearest4": list(g.ClosestAll(pops["points"], m)),
                "signed": list(g.SignedDistance(pops["points"])), "tridistance": list(g.TriangleDistance(pops["tris"])),
                "spherecast_kept": [g.SphereCast(pops["sweeps_kept"])], "spherecast_scaled": [g.SphereCast(pops["sweeps_scaled"])],
                "overlap": list(g.Overlap(pops["boxes"], m)), "trioverlap": list(g.OverlapTriangles(pops["trioverlap"], m)),
                "hexoverlap": list(g.OverlapHexahedra(pops["hexa"], m))}


def restated_answers(up, edges, spheres, pops):
    """The same by brute force over the restatements' tables, for the records of one layout; SignedDistance's sides with the
    table the library builds on the host."""
    import hexoverlap_expect as he
    import nearest_expect as ne
    import overlap_expect as oe
    import spherecast_expect as se
    import tridistance_expect as td
    import trioverlap_expect as te
    from raytracertest_amd import api
    m = rc.MAX_HITS
    with np.errstate(all="ignore"):
        tab = ce.table(pops["points"], up, edges, spheres)
        hits = ce.winners(tab, pops["points"][:, 3])
        return {"closest": [hits], "nearest4": list(ne.expected_all(tab, pops["points"][:, 3], m)),
                "signed": [hits, sg.expected_sides(pops["points"], hits, up, api.feature_normals(up, edges), edges, spheres)],
                "tridistance": list(td.expected(pops["tris"], up, edges, spheres)),
                "spherecast_kept": [se.expected(pops["sweeps_kept"], up, edges, spheres)],
                "spherecast_scaled": [se.expected(pops["sweeps_scaled"], up, edges, spheres)],
                "overlap": list(oe.expected(pops["boxes"], up, m, None, edges, spheres)),
                "trioverlap": list(te.expected(pops["trioverlap"], up, m, None, edges, spheres)),
                "hexoverlap": list(he.expected(pops["hexa"], up, m, None, edges, spheres))}


def _assert_same(got, want, label):
    assert got.keys() == want.keys()
    for query in got:
        assert len(got[query]) == len(want[query]), (label, query)
        for a, b in zip(got[query], want[query]):
            assert a.dtype == b.dtype and a.shape == b.shape, (label, query, a.dtype, b.dtype, a.shape, b.shape)
        bad = rc.differing_rows(got[query], want[query])
        assert bad.size == 0, (label, query, bad.size, bad[:5], [a[bad[:3]] for a in got[query]], [b[bad[:3]] for b in want[query]])


@pytest.mark.parametrize("k", rc.TREE_KS)
def test_scan_equals_the_restatement_and_tree_equals_scan_at_scale(k):
    rows, spheres = rc.scene("slivers")
    rows, spheres = rc.scaled_scene(rows, spheres, k)
    pops = rc.scaled_populations(rc.populations("slivers"), k)
    for edges in (False, True):
        up = edge_rows(rows) if edges else rows
        want = restated_answers(up, edges, spheres, pops)
        _reaches(want, pops, k)
        for math_mode in (0, 1):
            label = "k=%d edges=%d mm=%d" % (k, edges, math_mode)
            g = _tracer(math_mode)
            assert (g.UploadSceneEdges(up) if edges else g.UploadScene(up))
            g.UploadSpheres(spheres)
            scan = device_answers(g, pops)
            _assert_same(scan, want, label + " scan against the restatement")
            g.SetQueryAcceleration(True)
            tree = device_answers(g, pops)
            assert g.QueryAccelInfo()["valid"] == 1 and g.QueryAccelInfo()["always_tested"] >= 1
            _assert_same(tree, scan, label + " tree against scan")
            g.close()


def _reaches(want, pops, k):
    """The populations reach what they are for at this scale."""
    n = {q: a[0].shape[0] for q, a in want.items()}
    found = {q: rc.found(q, a) for q, a in want.items()}
    print("k = %d: found / queries: %s" % (k, ", ".join("%s %d/%d" % (q, found[q], n[q]) for q in want)))
    cast = want["spherecast_kept"][0]
    assert ((cast["prim"] >= 0) & (cast["t"] == 0)).any() and (cast["prim"] < 0).any()       # a start overlap and a miss
    if k == 0:
        assert all(found[q] >= n[q] // 3 and n[q] - found[q] >= n[q] // 10 for q in want), (found, n)
        assert ((cast["prim"] >= 0) & (cast["t"] == 0)).sum() >= 100
    if -74 <= k <= -60:                                                  # squared distances in the subnormals, kept
        for q in ("closest", "nearest4", "tridistance"):
            t = want[q][0]["t"]
            assert ((t > 0) & (t < TINY)).sum() >= 50, (q, k)
    if k <= -76:                                                         # ... and flushed by the arithmetic itself, to 0
        t = want["closest"][0]
        assert ((t["prim"] >= 0) & (t["t"] == 0)).sum() >= 100
    if k >= 60:                                                          # radii whose square is +inf
        with np.errstate(over="ignore"):
            assert np.isinf(pops["sweeps_kept"][:, 6] * pops["sweeps_kept"][:, 6]).any()
