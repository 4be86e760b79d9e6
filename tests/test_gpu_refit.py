"""The device refit of the ray queries' BVH (RT_ACCEL_REFIT): the refitted device tree against the host's rtb::refit byte for
byte and its cost against rtb::tree_cost; the answers of Intersect, Occluded and IntersectAll after refits -- bit-exact on the
moved lattice scenes, under the contracts' checks on jittered adversarial scenes with spheres; the policy (default rebuilds, a
changed triangle count and RebuildQueryAccel rebuild); the fallback to a build when a triangle changes its class; a running
Trace left alone; multi-device forwarding; and that a refit is not a rebuild in disguise (a relative speed gate)."""
import time

import numpy as np
import pytest

import lattice_cases as lc
import refit_cases as rc
from allhits_expect import check_bvh_all_hits, expected_all_hits, hit_table_uv, same_rows, sets_from_oracle
from occluded_expect import check_bvh_occluded, expected_occluded
from query_accel_expect import check_against_scan, check_tree
from query_expect import adversarial_rays, adversarial_scene, edge_rows, expected_hits, same_hits

pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
ONE_RAY = np.array([[0, 0, 0, 0.1, 0.2, -1]], np.float32)
_cache = {}


def _tracer(math_mode=0, nearest=False, size=(64, 48), refit=True, **kw):
    import raytracertest_amd as R
    g = R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)
    g.SetQueryAcceleration(True)
    if refit:
        g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    return g


def _upload(g, rows, edges=False):
    assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))


def _same_info(a, b):
    return {k: v for k, v in a.items() if k != "build_us"} == {k: v for k, v in b.items() if k != "build_us"}


@pytest.mark.parametrize("move", ["dyadic", "jitter", "collapse"])
@pytest.mark.parametrize("scene", ["rooms", "copies", "adversarial37", "adversarial1100"])
def test_device_refit_equals_host_refit(scene, move):
    from raytracertest_amd import api
    rows = rc.scenes()[scene]
    moved = rc.MOVES[move](rows)
    for edges in (False, True):                                          # the layout of the SECOND upload; the first is the other one
        g = _tracer()
        _upload(g, rows, not edges)
        g.Intersect(ONE_RAY)
        built, u0 = g.query_tree(), g.QueryAccelUpdateInfo()
        host = api.bvh_build(edge_rows(rows) if not edges else rows, not edges)
        assert rc.same_tree(built, host) and _same_info(built[2], host[2])
        assert u0["policy"] == 1 and u0["refits"] == 0 and u0["fallbacks"] == 0
        assert u0["cost"] == u0["cost_built"] == api.tree_cost(built[0])
        _upload(g, moved, edges)
        assert g.QueryAccelInfo()["valid"] == 0
        g.Intersect(ONE_RAY)
        tree, u1, info = g.query_tree(), g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
        up2 = edge_rows(moved) if edges else moved
        expect = api.bvh_refit(up2, *built, edges=edges)
        assert rc.same_tree(tree, expect), (scene, move, edges)
        check_tree(*tree, up2, edges)
        assert info["valid"] == 1 and tree[2] == built[2]                 # build_us included: nothing was built
        assert u1["refits"] == 1 and u1["fallbacks"] == 0 and u1["cost_built"] == u0["cost_built"]
        host_cost = api.tree_cost(tree[0])
        print("%s %s edges=%d: refit %d us on the device, cost %.6g -> %.6g" % (scene, move, edges, u1["refit_us"], u0["cost"], u1["cost"]))
        assert abs(u1["cost"] - host_cost) <= 1e-12 * host_cost, (u1["cost"], host_cost)
        if move == "collapse":
            assert u1["cost"] == 0.0
        g.close()


def _lattice_case(orc, scene, math_mode):
    """The moved lattice scene, its moved populations, their hit tables and segments, once per session."""
    key = (scene, math_mode)
    if key in _cache:
        return _cache[key]
    from raytracertest_amd import api
    contract = orc.FMA if math_mode == 0 else orc.STRICT
    c = {"contract": contract}
    if scene == "rooms":
        c["rows"] = lc.rooms()
        pops, _ = lc.rooms_populations(orc, c["rows"], api.bvh_build(c["rows"])[0], contract)
        c["exact"] = lc.LATTICE
    else:
        c["rows"] = lc.copies()[0]
        pops = {"copies": lc.copies_rays(), "control": lc.control_rays(c["rows"])}
        c["exact"] = ("copies",)
    c["moved"] = rc.dyadic(c["rows"])
    c["pops"] = {k: rc.dyadic_rays(r) for k, r in pops.items() if k in c["exact"]}
    c["table"] = {k: hit_table_uv(orc, r, c["moved"], None, contract) for k, r in c["pops"].items()}
    c["segs"] = {k: lc.segments(k, r, c["table"][k]) for k, r in c["pops"].items()}
    _cache[key] = c
    return c


@pytest.mark.parametrize("math_mode", [0, 1])
@pytest.mark.parametrize("scene", ["rooms", "copies"])
def test_answers_after_three_refits_are_bit_exact_on_the_moved_lattice(orc, scene, math_mode):
    """One tree, three refits in a row -- jittered, collapsed to a point, then the dyadic move -- and the three queries give
    the oracle's bits for the moved lattice populations: both hit rules, both layouts, max_hits 4 and 16."""
    c = _lattice_case(orc, scene, math_mode)
    rows, moved, contract = c["rows"], c["moved"], c["contract"]
    for edges in (False, True):
        for nearest in (False, True):
            g = _tracer(math_mode, nearest)
            _upload(g, rows, edges)
            g.Intersect(ONE_RAY)
            built = g.QueryAccelInfo()
            for step in (rc.jitter(rows, 5), rc.collapse(rows), moved):
                _upload(g, step, edges)
                g.Intersect(ONE_RAY)
            u, info = g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
            assert u["refits"] == 3 and u["fallbacks"] == 0 and info["build_us"] == built["build_us"] and info["valid"] == 1
            if scene == "rooms":                                         # an exact similarity of the built scene keeps the cost
                assert u["cost"] == pytest.approx(u["cost_built"], rel=1e-12)
            for name, rays in c["pops"].items():
                label = "%s %s mm=%d nearest=%d edges=%d" % (scene, name, math_mode, nearest, edges)
                exp = expected_hits(orc, rays, moved, None, contract, nearest)
                assert (exp["prim"] >= 0).any(), label
                for accel in (True, False):
                    g.SetQueryAcceleration(accel)
                    assert same_hits(g.Intersect(rays), exp), (label, accel)
                if nearest:
                    continue                                             # the other two queries name no hit rule
                segs, idx = c["segs"][name]
                table = c["table"][name]
                exp_occ = expected_occluded(orc, segs, moved, None, contract, (table[0][idx], table[1][idx]))
                assert exp_occ.any() and (~exp_occ).any(), label
                for accel in (True, False):
                    g.SetQueryAcceleration(accel)
                    assert np.array_equal(g.Occluded(segs), exp_occ), (label, accel)
                    for max_hits in (4, 16):
                        assert same_rows(g.IntersectAll(segs, max_hits), expected_all_hits(table, segs, max_hits, idx)), (label, accel, max_hits)
            assert g.QueryAccelUpdateInfo()["refits"] == 3               # the queries refitted nothing more
            g.close()


@pytest.mark.parametrize("n_tris", [37, 1100])
def test_answers_on_jittered_adversarial_scenes_with_spheres(orc, n_tris):
    rows = adversarial_scene(n_tris, n_tris)
    g = _tracer()
    _upload(g, rows)
    g.UploadSpheres(SPHERES)
    g.Intersect(ONE_RAY)
    for k in range(3):                                                   # three refits in a row on one tree
        moved = rc.jitter(rows, 40 + k, 0.05 * (k + 1))
        _upload(g, moved, edges=bool(k % 2))
        rays = adversarial_rays(moved, 200, 7 + k)
        segs = lc.ray_segments(rays)
        g.SetQueryAcceleration(False)
        scan, scan_occ = g.Intersect(rays), g.Occluded(segs)
        scan_all = {m: g.IntersectAll(segs, m) for m in (4, 16)}
        g.SetQueryAcceleration(True)
        label = "jittered adversarial%d step %d" % (n_tris, k)
        with np.errstate(all="ignore"):
            check_against_scan(g.Intersect(rays), scan, rays, moved, label=label)
            assert g.QueryAccelUpdateInfo()["refits"] == k + 1
            check_bvh_occluded(g.Occluded(segs), scan_occ, segs, moved, orc, SPHERES, label=label)
            E, W = sets_from_oracle(orc, segs, moved, SPHERES)
            for m in (4, 16):
                check_bvh_all_hits(g.IntersectAll(segs, m), scan_all[m], E, W, m, label="%s max_hits=%d" % (label, m))
    u = g.QueryAccelUpdateInfo()
    assert u["refits"] == 3 and u["fallbacks"] == 0 and u["cost"] > 0
    g.close()


def test_policy_default_rebuilds_and_so_do_a_new_count_and_an_explicit_rebuild():
    from raytracertest_amd import api
    rows = adversarial_scene(37, 3)
    moved = rc.jitter(rows.reshape(-1, 3, 4)[::-1].reshape(-1, 4), 9)    # the upload order reversed: a build sorts it out, a refit cannot
    g = _tracer(refit=False)                                             # the default policy
    _upload(g, rows)
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["policy"] == 0
    _upload(g, moved)
    assert g.QueryAccelInfo()["valid"] == 0
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 0
    assert rc.same_tree(g.query_tree(), api.bvh_build(moved))
    assert not rc.same_tree(g.query_tree(), api.bvh_refit(moved, *api.bvh_build(rows)))       # (the two differ on this scene)
    import raytracertest_amd as R
    with pytest.raises(R.RtError, match="unknown policy"):
        g.SetQueryAccelUpdate(2)
    g.SetQueryAccelUpdate(api.ACCEL_REFIT)
    _upload(g, rows)
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 1                       # the tree built under the other policy is refitted
    assert rc.same_tree(g.query_tree(), api.bvh_refit(rows, *api.bvh_build(moved)))
    other = adversarial_scene(38, 3)                                     # a changed triangle count builds
    _upload(g, other)
    g.Intersect(ONE_RAY)
    u = g.QueryAccelUpdateInfo()
    assert u["refits"] == 0 and u["fallbacks"] == 0 and rc.same_tree(g.query_tree(), api.bvh_build(other))
    _upload(g, rc.jitter(other, 2))
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 1
    g.RebuildQueryAccel()                                                # drops the tree at once
    assert g.QueryAccelInfo()["valid"] == 0
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and rc.same_tree(g.query_tree(), api.bvh_build(rc.jitter(other, 2)))
    _upload(g, other)                                                    # an upload and an explicit rebuild before the query: a build
    g.RebuildQueryAccel()
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and rc.same_tree(g.query_tree(), api.bvh_build(other))
    g.UploadSpheres(SPHERES)                                             # spheres touch nothing
    assert g.QueryAccelInfo()["valid"] == 1
    _upload(g, rc.jitter(other, 3))                                      # several uploads without a query: the last one counts
    _upload(g, rc.jitter(other, 4), edges=True)
    g.Intersect(ONE_RAY)
    assert g.QueryAccelUpdateInfo()["refits"] == 1
    assert rc.same_tree(g.query_tree(), api.bvh_refit(edge_rows(rc.jitter(other, 4)), *api.bvh_build(other), edges=True))
    g.close()


def test_a_class_change_falls_back_to_a_build():
    from raytracertest_amd import api
    rows = adversarial_scene(37, 3)
    rays = adversarial_rays(rows, 400, 4)
    g = _tracer()
    _upload(g, rows)
    g.Intersect(ONE_RAY)
    assert g.QueryAccelInfo()["always_tested"] == 0
    bad = rows.copy().reshape(-1, 3, 4)
    bad[int(g.query_tree()[1]["index"][0]), 1, 0] = np.nan               # a leaf's triangle
    bad = bad.reshape(-1, 4)
    _upload(g, bad)
    got = g.Intersect(rays)
    u, info = g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
    assert u["fallbacks"] == 1 and u["refits"] == 0 and info["always_tested"] == 1 and info["valid"] == 1
    assert rc.same_tree(g.query_tree(), api.bvh_build(bad))
    g.SetQueryAcceleration(False)
    with np.errstate(all="ignore"):
        check_against_scan(got, g.Intersect(rays), rays, bad, label="after the fallback")
    g.SetQueryAcceleration(True)
    _upload(g, rows)                                                     # and back: the always-tested triangle became finite
    got = g.Intersect(rays)
    u, info = g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
    assert u["fallbacks"] == 2 and u["refits"] == 0 and info["always_tested"] == 0
    assert rc.same_tree(g.query_tree(), api.bvh_build(rows))
    g.SetQueryAcceleration(False)
    check_against_scan(got, g.Intersect(rays), rays, rows, label="after the second fallback")
    g.close()


def test_a_refit_does_not_disturb_a_running_trace():
    """test_bvh_picks_do_not_disturb_a_running_trace with a refit in place of the build: the picks that run while the Trace
    does refit the tree of an earlier upload, and the Trace's buffers are those of a run without any query."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    earlier = rc.jitter(rows, 1, 0.01)
    pix = np.array([[1000, 500], [17, 3], [1919, 1079]], np.uint32)

    def run(picks, refit):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        if refit:
            g.SetQueryAcceleration(True)
            g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
            assert g.UploadScene(earlier)
            g.Pick(pix)                                                  # the tree of the earlier scene
            g.SetQueryAcceleration(False)
        assert g.UploadScene(rows)
        idle = g.Pick(pix)                                               # the scan
        got = []
        g.Trace(24, 4, 2)
        if refit:
            g.SetQueryAcceleration(True)                                 # the tree is refitted while the Trace runs
        for _ in range(picks):
            got.append(g.Pick(pix))
        assert g.Wait() == 1
        if refit:
            u = g.QueryAccelUpdateInfo()
            assert u["refits"] == 1 and u["fallbacks"] == 0
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(20, True)
    assert len(got) == 20 and all(same_hits(x, idle) for x in got)
    _, _, ref = run(0, False)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_forwards_to_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import api, scenes
    rows = scenes.cornell32()
    moved = rc.jitter(rows, 3, 0.02)
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    m.SetQueryAcceleration(True)
    m.SetQueryAccelUpdate(api.ACCEL_REFIT)
    assert m.UploadScene(rows)
    pix = lc.frame_pixels(96, 64)
    m.Pick(pix)
    built = m.query_tree()
    assert m.UploadScene(moved)
    got, rays = m.Pick(pix, return_rays=True)
    u = m.QueryAccelUpdateInfo()
    assert u["policy"] == 1 and u["refits"] == 1 and u["cost"] > 0
    assert rc.same_tree(m.query_tree(), api.bvh_refit(moved, *built))
    m.SetQueryAcceleration(False)
    check_against_scan(got, m.Pick(pix), rays, moved, label="two bands after a refit")
    m.SetQueryAcceleration(True)
    m.RebuildQueryAccel()
    assert m.QueryAccelInfo()["valid"] == 0
    m.Pick(pix)
    assert m.QueryAccelUpdateInfo()["refits"] == 0 and rc.same_tree(m.query_tree(), api.bvh_build(moved))
    m.close()


def test_a_refit_is_no_rebuild_in_disguise():
    """Relative, one run: on 200 000 triangles with jittered vertices, the median over 5 of the first one-ray Intersect after an
    upload under RT_ACCEL_REFIT is below a quarter of the same median under RT_ACCEL_REBUILD (a read-back of 7 MB, the host
    build and the upload of the tree against about ten small launches and a 16-byte copy).  The factor guards against a refit
    that quietly rebuilds; it is no performance claim."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(200000, 77)
    rng = np.random.default_rng(3)
    jittered = [rows]
    for _ in range(5):
        r = rows.copy()
        r[:, :3] += rng.uniform(-0.01, 0.01, (r.shape[0], 3)).astype(np.float32)
        jittered.append(r)
    g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    g.SetQueryAcceleration(True)
    medians = {}
    for policy in (R.api.ACCEL_REFIT, R.api.ACCEL_REBUILD):
        g.SetQueryAccelUpdate(policy)
        assert g.UploadScene(jittered[0])
        g.RebuildQueryAccel()
        g.Intersect(ONE_RAY)                                             # the tree both arms start from, built
        times = []
        for r in jittered[1:]:
            assert g.UploadScene(r)
            t0 = time.perf_counter()
            g.Intersect(ONE_RAY)
            times.append((time.perf_counter() - t0) * 1e3)
        medians[policy] = float(np.median(times))
        u = g.QueryAccelUpdateInfo()
        assert u["refits"] == (5 if policy == R.api.ACCEL_REFIT else 0) and u["fallbacks"] == 0
        if policy == R.api.ACCEL_REFIT:
            device_us, cost = u["refit_us"], (u["cost"], u["cost_built"])
    print("first one-ray Intersect after an upload, 200 000 triangles: refit %.3f ms (device %d us, cost %.4g from %.4g), rebuild %.3f ms, ratio %.1f"
          % (medians[1], device_us, cost[0], cost[1], medians[0], medians[0] / medians[1]))
    assert medians[1] < 0.25 * medians[0]
    g.close()
