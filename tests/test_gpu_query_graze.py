"""The ray queries' BVH at its conditioning bound, on the device: the grazing populations of graze_cases.py through Intersect
(both hit rules, both arithmetic modes), Occluded, IntersectAll and Exposure, tree against scan on the same tracer (the scan is
pinned to the oracle elsewhere; the oracle is asked only about rows that differ).  Above the bound (`above`, `rivals`) the
contracts' ordinary checks with the exclusion capped, and no exclusion at all where the targeted triangle wins; below it the
one-sided contract.  With bare boxes (slack 0) the same rows must differ -- the population reaches the pad -- and a refitted
tree and a two-band handle give what a built tree on one band gives."""
import numpy as np
import pytest

import exposure_expect as ee
import graze_cases as gc
import refit_cases as rc
from allhits_expect import check_bvh_all_hits, sets_from_oracle
from occluded_expect import check_bvh_occluded
from query_accel_expect import EXCLUSION_CAP, WELL_CONDITIONED, check_against_scan, conditioning
from query_expect import edge_rows, same_hits

pytestmark = pytest.mark.gpu

N_TRIS = 2000
N_RAYS = 81 * 809                                # 65 529 <= 2^16: every class combination with every interval kind
N_PAIRS = 999
SCENES = ["general", "flat", "slivers", "pairs"]
_cache = {}


def case(name):
    """Scene and populations, made once per session."""
    if name in _cache:
        return _cache[name]
    c = {}
    if name == "pairs":
        c["rows"], c["rivals"] = gc.pairs(N_PAIRS)
    else:
        c["rows"] = gc.SCENES[name](N_TRIS, size=0.6) if name != "slivers" else gc.slivers(N_TRIS)
        c["above"] = gc.rays(c["rows"], "above", N_RAYS, seed=51)
        c["below"] = gc.rays(c["rows"], "below", N_RAYS, seed=52)
    c["top"] = "rivals" if name == "pairs" else "above"
    _cache[name] = c
    return c


def _tracer(math_mode=0, nearest=False, **kw):
    import raytracertest_amd as R
    return R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)


def _upload(g, rows, edges):
    assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))


def _both(g, query):
    """(scan, tree) answers of one query on the tracer; the tree stays switched on."""
    g.SetQueryAcceleration(False)
    scan = query()
    g.SetQueryAcceleration(True)
    got = query()
    info = g.QueryAccelInfo()
    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0, info
    return scan, got


def _differ(a, b):
    return (np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4) != np.ascontiguousarray(b).view(np.uint32).reshape(-1, 4)).any(axis=1)


@pytest.mark.parametrize("math_mode", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_intersect_above_the_bound_is_the_scan(name, math_mode):
    c = case(name)
    rows, pop = c["rows"], c[c["top"]]
    rays = pop["rays"]
    for nearest in (False, True):
        for edges in (False, True):
            g = _tracer(math_mode, nearest)
            _upload(g, rows, edges)
            scan, got = _both(g, lambda: g.Intersect(rays))
            label = "%s %s mm=%d nearest=%d edges=%d" % (name, c["top"], math_mode, nearest, edges)
            up = edge_rows(rows) if edges else rows
            check_against_scan(got, scan, rays, up, edges, label)      # (the exclusions are capped at EXCLUSION_CAP there)
            won = gc.targeted_wins(pop, scan)
            print("%s: the targeted triangle wins the scan on %d rows" % (label, int(won.sum())))
            assert won.sum() >= 0.01 * rays.shape[0] and not (_differ(got, scan) & won).any()
            for n in (1, 63, 65):                                        # partial waves
                assert same_hits(g.Intersect(rays[:n]), got[:n])
            g.close()


@pytest.mark.parametrize("name", SCENES)
def test_occluded_all_hits_and_exposure_above_the_bound(orc, name):
    c = case(name)
    rows, pop = c["rows"], c[c["top"]]
    segs = gc.segments(pop)
    groups = gc.exposure_groups(pop, 12)
    for edges in (False, True):
        g = _tracer(0)
        _upload(g, rows, edges)
        label = "%s %s edges=%d" % (name, c["top"], edges)
        scan, got = _both(g, lambda: g.Occluded(segs))
        assert scan.any() and (~scan).any()
        check_bvh_occluded(got, scan, segs, rows, orc, None, orc.FMA, cap=EXCLUSION_CAP, label=label + " occluded")
        E, W = sets_from_oracle(orc, segs, rows, None, orc.FMA)
        for max_hits in (1, 4, 16):
            scan, got = _both(g, lambda: g.IntersectAll(segs, max_hits))
            check_bvh_all_hits(got, scan, E, W, max_hits, cap=EXCLUSION_CAP, label="%s all hits" % label)
        lost = 0
        for pts, dirs in groups:                                         # Exposure with a world-space table, against Occluded's scan
            rays8 = ee.exposure_segments(pts, dirs, world=True)
            g.SetQueryAcceleration(False)
            occ = g.Occluded(rays8)
            assert np.array_equal(g.Exposure(pts, dirs, world=True), ee.pack_masks(~occ.reshape(64, 64)))
            g.SetQueryAcceleration(True)
            masks = g.Exposure(pts, dirs, world=True)
            lost += check_bvh_occluded(~ee.unpack_masks(masks).reshape(-1), occ, rays8, rows, orc, None, orc.FMA, label=label + " exposure")
        assert lost <= EXCLUSION_CAP * 4096 * len(groups)
        g.close()


@pytest.mark.parametrize("name", ["general", "flat", "slivers"])
def test_below_the_bound_only_the_one_sided_contract(orc, name):
    c = case(name)
    rows, pop = c["rows"], c["below"]
    rays = pop["rays"]
    segs = gc.segments(pop)
    for nearest in (False, True):
        g = _tracer(0, nearest)
        _upload(g, rows, False)
        scan, got = _both(g, lambda: g.Intersect(rays))
        gc.check_one_sided(orc, got, scan, rays, rows, orc.FMA, nearest, "%s below nearest=%d" % (name, nearest))
        if not nearest:
            scan, got = _both(g, lambda: g.Occluded(segs))
            check_bvh_occluded(got, scan, segs, rows, orc, None, orc.FMA, label=name + " below occluded")
            few = segs[:8192]
            E, W = sets_from_oracle(orc, few, rows, None, orc.FMA)
            for max_hits in (1, 4, 16):
                scan, got = _both(g, lambda: g.IntersectAll(few, max_hits))
                check_bvh_all_hits(got, scan, E, W, max_hits, label="%s below all hits" % name)
        g.close()


@pytest.mark.parametrize("name", ["general", "flat", "slivers"])
def test_bare_boxes_lose_well_conditioned_rows_of_the_farthest_class(name):
    """The teeth on the device: with the pad taken away (slack 0) at least one row of the 2^21 class whose scan winner is well
    conditioned gets another answer.  If none does, the population no longer reaches the pad and the checks above prove nothing
    about it."""
    c = case(name)
    rows, pop = c["rows"], c["above"]
    rays = pop["rays"]
    g = _tracer(0)
    _upload(g, rows, False)
    scan, product = _both(g, lambda: g.Intersect(rays))
    g.DebugQueryAccelSlack(0)
    try:
        bare = g.Intersect(rays)
    finally:
        g.DebugQueryAccelSlack(1000)
    well = _differ(bare, scan) & (conditioning(rays, rows, scan["prim"]) >= WELL_CONDITIONED)
    per = [int((well & (pop["L"] == k)).sum()) for k in range(3)]
    print("%s, bare boxes: %d well-conditioned rows differ from the scan, by distance class %s" % (name, int(well.sum()), per))
    assert per[2] >= 1
    assert ((bare["prim"] >= -1) & (bare["prim"] < rows.shape[0] // 3)).all()
    assert same_hits(g.Intersect(rays), product)                         # slack 1000 again: the product
    g.close()


@pytest.mark.parametrize("name", ["flat", "pairs"])
def test_a_refitted_tree_and_a_two_band_handle(orc, name):
    import raytracertest_amd as R
    c = case(name)
    rows, pop = c["rows"], c[c["top"]]
    rays, segs = pop["rays"][:1 << 14], gc.segments(pop)[:1 << 14]
    g = _tracer(0)
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    _upload(g, rows, False)
    scan, got = _both(g, lambda: g.Intersect(rays))
    check_against_scan(got, scan, rays, rows, label=name + " built")
    moved, moved_rays = rc.dyadic(rows), rc.dyadic_rays(rays)            # (the shift is rounded into a far origin: other rays, same kind)
    moved_segs = np.ascontiguousarray(np.c_[moved_rays, segs[:, 6:]], np.float32)
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = g.Intersect(moved_rays)
    info = g.QueryAccelUpdateInfo()
    assert info["refits"] == 1 and info["fallbacks"] == 0, info
    occ = g.Occluded(moved_segs)
    g.SetQueryAcceleration(False)
    check_against_scan(got, g.Intersect(moved_rays), moved_rays, moved, label=name + " refitted")
    check_bvh_occluded(occ, g.Occluded(moved_segs), moved_segs, moved, orc, None, orc.FMA, cap=EXCLUSION_CAP, label=name + " refitted occluded")
    g.close()
    m = _tracer(0, devices=[0, 0])
    _upload(m, rows, False)
    scan, got = _both(m, lambda: m.Intersect(rays))
    check_against_scan(got, scan, rays, rows, label=name + " two bands")
    scan, got = _both(m, lambda: m.Occluded(segs))
    check_bvh_occluded(got, scan, segs, rows, orc, None, orc.FMA, cap=EXCLUSION_CAP, label=name + " two bands occluded")
    m.close()
