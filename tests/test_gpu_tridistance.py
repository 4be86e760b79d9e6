"""The triangle distance query on the device (RayTracer.TriangleDistance / TriangleDistancePositions / MeshDistance): the scan
and the BVH walk against the numpy restatement of tridistance_expect, both arrays byte for byte, for both upload layouts, both
arithmetic modes (which must not change a byte), with and without spheres, every family of search radii and batches that end in
partial waves and blocks; the BVH walk against the scan kernel byte for byte on 16 384 queries with any slack; the overflow path;
the collapsed query against ClosestPoint; the certification by the witness; zero-area and non-finite records, empty scenes; the
torch path, argument errors, a refitted tree, a running Trace left alone, multi-device forwarding; and two cubes at a known gap."""
import functools
import hashlib

import numpy as np
import pytest

import closest_expect as ce
import lattice_cases as lc
import tridistance_expect as td
import trioverlap_expect as te
from query_accel_expect import records_of_rows
from query_expect import HIT_DTYPE, edge_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = f32(np.inf)
SPHERES = f32([[0.5, 0.3, -1.0, 0.8], [0.5, 0.3, -1.0, 0.8], [40.0, -35.0, 20.0, 6.0]])   # two coincident, one far away
COUNTS = (1, 63, 64, 65)                                                 # partial waves; 4097 is a partial last block as well


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _assert_same(got, exp, label):
    assert got[0].dtype == HIT_DTYPE and got[1].dtype == td.WITNESS_DTYPE and got[0].shape == exp[0].shape and got[1].shape == exp[1].shape, label
    bad = td.differing(got, exp)
    assert bad.size == 0, (label, bad[:5], [(got[0][i], got[1][i], exp[0][i], exp[1][i]) for i in bad[:2]])


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, the mixed queries (4097 of them, 257 on the scene that crosses the LDS chunk seam: 1100 x 4097 pairs of 27 point
    evaluations each are minutes of numpy), and the table with SPHERES' columns: one table for all."""
    rows = ce.random_scene(n_tris, 100 + n_tris)
    queries = td.mixed_queries(rows, 257 if n_tris > 100 else 4097, 200 + n_tris)
    queries[:2, :] = td.with_radius(te.queries_of([[[0.5, 0.3, -1.9], [1.4, 0.3, -1.0], [0.5, 1.2, -1.0]],     # cuts the twin spheres
                                                   [[0.5, 0.3, -1.0], [0.6, 0.3, -1.0], [0.5, 0.4, -0.9]]]), INF)  # inside them
    tab = td.table(queries, rows, spheres=SPHERES)
    for x in (rows, queries) + tuple(tab.values()):
        x.setflags(write=False)
    return rows, queries, tab


def _without_spheres(tab, n_tris):
    return {k: v[:, :n_tris] for k, v in tab.items()}


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_radius_and_count(n_tris, spheres):
    rows, queries, tab = _reference(n_tris)
    tab = tab if spheres else _without_spheres(tab, n_tris)
    fams = td.radius_families(queries, rows, tab=tab)
    exp = {fam: td.winners(tab, q[:, 3]) for fam, q in fams.items()}
    assert (exp["inf"][0]["prim"] >= 0).any() and (exp["inf"][0]["prim"] < 0).any()          # (the non-finite queries)
    if spheres:
        assert tab["t"][0, n_tris] == 0 and tab["t"][0, n_tris + 1] == 0 and tab["t"][1, n_tris] > 0
        assert (exp["inf"][0]["prim"] == n_tris).any() and not (exp["inf"][0]["prim"] == n_tris + 1).any()
    for a, b in zip(records_of_rows(rows, False), records_of_rows(edge_rows(rows), True)):
        assert a.tobytes() == b.tobytes()                                # the edge layout's records are the same records
    digests = {}
    for edges in (False, True):
        for mm in (0, 1):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            if spheres:
                g.UploadSpheres(SPHERES)
            blob = hashlib.sha256()
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for fam, q in fams.items():
                    label = "n_tris=%d spheres=%d edges=%d mm=%d accel=%d %s" % (n_tris, spheres, edges, mm, accel, fam)
                    got = g.TriangleDistance(q)
                    _assert_same(got, exp[fam], label)
                    blob.update(got[0].tobytes())
                    blob.update(got[1].tobytes())
                for n in COUNTS:
                    _assert_same(g.TriangleDistance(fams["half"][:n]), tuple(x[:n] for x in exp["half"]), "n=%d accel=%d" % (n, accel))
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


def _big_scene(name):
    from raytracertest_amd import scenes
    if name == "random10000":
        return scenes.random_triangles(10000, 12345)
    if name == "layered":
        from allhits_expect import layered_scene
        return layered_scene(48, 16, 5)
    return lc.rooms()


@pytest.mark.parametrize("scene", ["random10000", "layered", "rooms"])
def test_bvh_equals_scan_byte_for_byte_whatever_the_slack(scene):
    rows = _big_scene(scene)
    queries = td.mixed_queries(rows, 16384, 7)
    if scene == "rooms":
        tie = td.lattice_queries()
        queries[:tie.shape[0]] = tie
    g = _tracer()
    assert g.UploadScene(rows)
    scan_inf = g.TriangleDistance(queries)
    fin = scan_inf[0]["t"][scan_inf[0]["prim"] >= 0]
    bounded = td.with_radius(queries, f32(np.median(fin)))
    scan = {"inf": scan_inf, "half": g.TriangleDistance(bounded)}
    assert (scan["half"][0]["prim"] < 0).sum() > (scan["inf"][0]["prim"] < 0).sum() and (scan["half"][0]["prim"] >= 0).any()
    _assert_same(tuple(x[:24] for x in scan_inf), td.expected(queries[:24], rows), "the scan against the helper")
    g.SetQueryAcceleration(True)
    for slack in (None, 1000, 3000):
        if slack is not None:
            g.DebugQueryAccelSlack(slack)
        for fam, q in (("inf", queries), ("half", bounded)):
            got = g.TriangleDistance(q)
            bad = td.differing(got, scan[fam])
            assert bad.size == 0, (scene, slack, fam, bad.size, bad[:5])
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_a_shortened_stack_gives_the_same_answer():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    queries = td.with_radius(np.concatenate([te.queries_near(rows, 600, 3, edge=0.5), te.queries_near(rows, 200, 4, edge=40.0)]), INF)
    g = _tracer()
    assert g.UploadScene(rows)
    scan = g.TriangleDistance(queries)
    assert (scan[0]["prim"] >= 0).any()
    g.SetQueryAcceleration(True)
    try:
        for cap in (None, 0, 1, 3):
            g.DebugQueryStackCap(cap)
            _assert_same(g.TriangleDistance(queries), scan, "deep cap=%r" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


@pytest.mark.parametrize("scene", ["random37", "rooms"])
def test_a_collapsed_query_is_closest_point_on_the_device(scene):
    rows = ce.random_scene(37, 137) if scene == "random37" else lc.rooms()
    pts = ce.points_for(rows, 4097, 8) if scene == "random37" else ce.lattice_points()
    g = _tracer()
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for fam, p in ce.radius_families(pts, rows).items():
            point_hits = g.ClosestPoint(p)
            hits, wit = g.TriangleDistance(td.with_radius(td.point_queries(p[:, :3]), p[:, 3]))
            assert ce.same_hits(hits, point_hits), (scene, accel, fam, ce.differing(hits, point_hits)[:5])
            ok = hits["prim"] >= 0
            assert (wit["where"][ok] == 0).all() and (wit["where"][~ok] == -1).all()
            w = np.stack([wit["x"], wit["y"], wit["z"]], axis=1)
            assert w[ok].view(np.uint32).tobytes() == np.ascontiguousarray(p[ok, :3]).view(np.uint32).tobytes()
    g.close()


def test_the_witness_certifies_the_answer():
    """(t, u, v) is the point rule at witness.xyz on record prim, bit for bit, and ClosestPoint at the witness within t finds
    something at least that near."""
    rows, queries, tab = _reference(37)
    g = _tracer()
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        hits, wit = g.TriangleDistance(queries)
        ok = hits["prim"] >= 0
        pts = np.stack([wit["x"], wit["y"], wit["z"]], axis=1)[ok]
        T, U, V, _ = ce.table(pts, rows)
        i = np.arange(pts.shape[0])
        for name, col in (("t", T), ("u", U), ("v", V)):
            assert hits[name][ok].view(np.uint32).tobytes() == np.ascontiguousarray(col[i, hits["prim"][ok]]).view(np.uint32).tobytes(), (accel, name)
        again = g.ClosestPoint(ce.with_radius(pts, hits["t"][ok]))
        assert (again["prim"] >= 0).all() and (again["t"] <= hits["t"][ok]).all()
        same = again["prim"] == hits["prim"][ok]
        assert same.mean() > 0.5 and ce.same_hits(again[same], hits[ok][same])
        on_query, on_scene = g.TriangleDistancePositions(hits, wit)
        assert np.isnan(on_query[~ok]).all() and np.isnan(on_scene[~ok]).all()
        d = np.linalg.norm(on_query[ok].astype(np.float64) - on_scene[ok], axis=1)
        assert np.allclose(d, np.sqrt(hits["t"][ok].astype(np.float64)), rtol=1e-4, atol=1e-5)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                    # (inf - inf and overflow are what the scene is made of)
def test_zero_area_and_non_finite_records_empty_scenes_and_spheres_alone():
    deg = ce.degenerate_scene()
    rows = ce.random_scene(37, 3).reshape(-1, 3, 4).copy()
    rows[5, 1, 0] = np.nan
    rows[11, 0, 1] = -np.inf
    rows[20, 0, :3], rows[20, 1, :3] = 3.0e38, -3.0e38                   # finite vertices whose edge overflows
    rows[30, 2] = rows[30, 1] = rows[30, 0]                              # a point: a finite record like any other
    rows = rows.reshape(-1, 4)
    for scene, always in ((deg, 0), (rows, 2), (np.full_like(rows, np.nan), 37)):
        queries = np.concatenate([td.mixed_queries(deg if scene is deg else ce.random_scene(37, 3), 300, 4),
                                  td.with_radius(td.parallel_queries(deg, range(3, 8)), INF)])   # needles, points, zero-area records as queries
        for edges in (False, True):
            r = edge_rows(scene) if edges else scene
            exp = td.expected(queries, r, edges=edges, spheres=SPHERES)
            assert not np.isnan(exp[0]["t"]).any()                       # never a NaN winner
            if scene is rows:
                assert not np.isin(exp[0]["prim"], (5, 11)).any() and (exp[0]["prim"] >= 0).any()
            g = _tracer()
            assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
            g.UploadSpheres(SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                _assert_same(g.TriangleDistance(queries), exp, "always=%d edges=%d accel=%d" % (always, edges, accel))
            assert g.QueryAccelInfo()["always_tested"] >= always
            g.close()
    queries = td.mixed_queries(ce.random_scene(37, 3), 300, 4)
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        hits, wit = g.TriangleDistance(queries)                          # no scene: nothing is near
        assert (hits["prim"] == -1).all() and (wit["where"] == -1).all() and not hits["t"].any() and not wit["x"].any()
        hits, wit = g.TriangleDistance(np.zeros((0, 12), f32))
        assert hits.shape == (0,) and wit.shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        exp = td.expected(queries, None, spheres=SPHERES)
        assert (exp[0]["prim"] >= 0).any()
        _assert_same(g.TriangleDistance(queries), exp, "spheres only accel=%d" % accel)
        g.close()


def test_argument_errors_leave_the_outputs_untouched_and_triangle_forms_agree():
    import raytracertest_amd as R
    rows, queries, tab = _reference(37)
    L = R.api.load_library()
    g = _tracer()
    assert g.UploadScene(rows)
    q = np.ascontiguousarray(queries[:70])
    hits = np.full((70, 4), 77, np.int32)
    wit = np.full((70, 4), 99, np.int32)
    for args in ((None, 70, hits.ctypes.data, wit.ctypes.data), (q.ctypes.data, 70, None, wit.ctypes.data), (q.ctypes.data, 70, hits.ctypes.data, None)):
        assert L.rt_tracer_triangle_distance(g._h, *args) == 1 and "null" in g.LastError()
    assert (hits == 77).all() and (wit == 99).all()
    assert L.rt_tracer_triangle_distance(g._h, None, 0, None, None) == 0                      # n = 0 is a no-op
    assert L.rt_tracer_triangle_distance(None, q.ctypes.data, 70, hits.ctypes.data, wit.ctypes.data) == 1
    for bad in (np.zeros((4, 5), f32), f32(1.0), np.zeros((4, 8), f32)):
        with pytest.raises(ValueError):
            g.TriangleDistance(bad)
    c = te.corners_of(q)
    want = g.TriangleDistance(td.with_radius(q, INF))
    for form in (c, c.reshape(-1, 9)):
        _assert_same(g.TriangleDistance(form), want, "triangle forms")
    near = g.TriangleDistance(c, max_distance=0.5)                       # squared on the host in fp32
    _assert_same(near, g.TriangleDistance(td.with_radius(q, f32(0.5) * f32(0.5))), "max_distance")
    assert (g.TriangleDistance(c, max_distance=-1.0)[0]["prim"] == -1).all()
    g.close()


def test_torch_path_on_a_side_stream_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, queries, tab = _reference(1100)
    exp = td.winners(tab, queries[:, 3])
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(queries)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        th, tw = g.TriangleDistance(t)
        assert th.dtype == torch.float32 and th.shape == (queries.shape[0], 4) and tw.shape == (queries.shape[0], 4)
        assert th.cpu().numpy().tobytes() == exp[0].tobytes() and tw.cpu().numpy().tobytes() == exp[1].tobytes()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                       # on the caller's current stream
            th2, tw2 = g.TriangleDistance(t)
        s.synchronize()
        assert th2.cpu().numpy().tobytes() == exp[0].tobytes() and tw2.cpu().numpy().tobytes() == exp[1].tobytes()
        th0, tw0 = g.TriangleDistance(t[:0])
        assert th0.shape == (0, 4) and tw0.shape == (0, 4)
    for bad in (t.cpu(), t.double(), t[:, :9].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.TriangleDistance(bad)
    flat = t.reshape(-1)
    out = torch.full((9 * 4,), 77, dtype=torch.int32, device="cuda:0")
    wit = torch.full((9 * 4,), 99, dtype=torch.int32, device="cuda:0")
    P, O, W = flat.data_ptr(), out.data_ptr(), wit.data_ptr()
    for args in ((P + 4, 8, O, W), (P, 8, O + 4, W), (P, 8, O, W + 8)):  # misaligned triangles, hits, witness
        assert L.rt_tracer_triangle_distance_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, 8, O, W), (P, 8, None, W), (P, 8, O, None)):
        assert L.rt_tracer_triangle_distance_device(g._h, *args, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (wit == 99).all()                       # the outputs are untouched
    assert L.rt_tracer_triangle_distance_device(g._h, None, 0, None, None, None) == 0
    assert L.rt_tracer_triangle_distance_device(g._h, P, 8, O, W, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:32].tobytes() == exp[0][:8].tobytes() and wit.cpu().numpy()[:32].tobytes() == exp[1][:8].tobytes()
    assert (out[32:] == 77).all() and (wit[32:] == 99).all()
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    queries = td.mixed_queries(moved, 4096, 9)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.TriangleDistance(queries)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = g.TriangleDistance(queries)                                    # refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    _assert_same(got, g.TriangleDistance(queries), "after the refit")
    assert td.differing(first, got).size > 0                             # the scene did move
    _assert_same(tuple(x[:64] for x in got), td.expected(queries[:64], moved), "the moved scene against the helper")
    g.close()


def test_triangle_distance_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    queries = td.mixed_queries(rows, 2048, 7)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.TriangleDistance(queries)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.TriangleDistance(queries))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(6)
    assert len(got) == 6 and (idle[0]["prim"] >= 0).any()
    for pair in got:
        _assert_same(pair, idle, "during the Trace")
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    queries = td.mixed_queries(rows, 1500, 3)
    exp = td.expected(queries, rows)
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_same(one.TriangleDistance(queries), exp, "one band against the helper")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_same(m.TriangleDistance(queries), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_same(m.TriangleDistance(queries), exp, "two bands, bvh")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()


@pytest.mark.parametrize("edges", [False, True])
def test_mesh_distance_of_two_cubes_at_a_known_gap(edges):
    scene = te.cube_rows(-1.0, 1.0)
    other = scene.reshape(-1, 3, 4)[:, :, :3] + f32([2.5, 0.0, 0.0])     # face against face, 1/2 apart
    shifted = other + f32([0.0, 3.0, 3.0])                               # corner against corner: (1/2, 1, 1) from the corner (1, 1, 1)
    g = _tracer()
    assert g.MeshDistance(other) is None                                 # no scene
    assert (g.UploadSceneEdges(te.to_edges(scene)) if edges else g.UploadScene(scene))
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        m = g.MeshDistance(other)
        assert m["distance"] == 0.5 and m["on_query"][0] == 1.5 and m["on_scene"][0] == 1.0 and m["prim"] in (2, 3)
        assert np.array_equal(m["on_query"][1:], m["on_scene"][1:])
        hits = g.TriangleDistance(other)[0]
        assert m["query"] == int(np.argmin(hits["t"])) and hits["t"].min() == 0.25
        m = g.MeshDistance(shifted)
        assert m["distance"] == 1.5 and m["on_scene"].tolist() == [1.0, 1.0, 1.0] and m["on_query"].tolist() == [1.5, 2.0, 2.0]
        assert g.MeshDistance(shifted, max_distance=1.0) is None and g.MeshDistance(shifted, max_distance=1.5) is not None
    g.close()
