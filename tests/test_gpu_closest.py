"""The point query on the device (RayTracer.ClosestPoint): the scan and the BVH walk against the numpy restatement of
closest_expect, bit for bit, for both upload layouts, both arithmetic modes (which must not change a byte), with and without
spheres, five search radii and batches that end in partial waves and blocks; the BVH walk against the scan kernel, bit for bit
with no exclusion, on a scene of stacked sheets, on 10 000 random triangles and on a lattice; non-finite and zero-area
triangles; the torch path, argument checks, a refitted tree, a running Trace left alone and multi-device forwarding."""
import functools

import numpy as np
import pytest

import closest_expect as ce
from query_expect import HIT_DTYPE, edge_rows

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
# two coincident spheres (a tie between spheres goes to the lower prim), one the points are inside or near, one far away
SPHERES = np.array([[0.5, 0.3, -1.0, 0.8], [0.5, 0.3, -1.0, 0.8], [40.0, -35.0, 20.0, 6.0]], np.float32)
COUNTS = (1, 63, 64, 65)                                                 # partial waves; 4097 is a partial last block as well


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _assert_same(got, exp, label):
    assert got.dtype == HIT_DTYPE and got.shape == exp.shape, label
    bad = ce.differing(got, exp)
    assert bad.size == 0, (label, bad.size, bad[:5], got[bad[:3]], exp[bad[:3]])


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, 4097 points, the five radius families and the expected answers without and with SPHERES: one table for all."""
    rows = ce.random_scene(n_tris, seed=100 + n_tris)
    pts = ce.points_for(rows, 4097, seed=200 + n_tris)
    tab = ce.table(pts, rows, spheres=SPHERES)
    bare = tuple(x[:, :n_tris] for x in tab)
    fams = ce.radius_families(pts, rows)
    exp = {(fam, sph): ce.winners(tab if sph else bare, p[:, 3]) for fam, p in fams.items() for sph in (False, True)}
    for v in exp.values():
        v.setflags(write=False)
    return rows, fams, exp


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_radius_and_count(n_tris, spheres):
    rows, fams, exp = _reference(n_tris)
    share = float((exp[("half", False)]["prim"] >= 0).mean())
    assert 0.3 < share < 0.7, share                                      # "half" cuts about half
    assert (exp[("inf", spheres)]["prim"] >= 0).all() and (exp[("zero", spheres)]["prim"] >= 0).any()
    assert not (exp[("nan", spheres)]["prim"] >= 0).any() and not (exp[("negative", spheres)]["prim"] >= 0).any()
    if spheres:
        assert (exp[("inf", True)]["prim"] >= n_tris).any() and not (exp[("inf", True)]["prim"] == n_tris + 1).any()
    blobs = {}
    for edges in (False, True):
        for mm in (0, 1):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            if spheres:
                g.UploadSpheres(SPHERES)
            blob = []
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for fam, p in fams.items():
                    label = "n_tris=%d spheres=%d edges=%d mm=%d accel=%d %s" % (n_tris, spheres, edges, mm, accel, fam)
                    got = g.ClosestPoint(p)
                    _assert_same(got, exp[(fam, spheres)], label)
                    blob.append(got.tobytes())
                    if fam in ("inf", "half"):
                        for n in COUNTS:
                            _assert_same(g.ClosestPoint(p[:n]), exp[(fam, spheres)][:n], label + " n=%d" % n)
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            blobs[(edges, mm)] = b"".join(blob)
            g.close()
    assert len(set(blobs.values())) == 1                                 # neither the layout nor the arithmetic mode changes a byte


@pytest.mark.parametrize("scene", ["layered", "c4_10k", "lattice"])
def test_bvh_equals_the_scan_bit_for_bit_on_65536_points(scene):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    if scene == "layered":
        from allhits_expect import layered_scene
        rows = layered_scene(48, 16, 5)
    elif scene == "c4_10k":
        rows = scenes.random_triangles(10000, 12345)
    else:
        import lattice_cases as lc
        rows = lc.rooms()
    n = 1 << 16
    pts = ce.points_for(rows, n, seed=61, spread=4.0)
    if scene == "lattice":                                               # the exact ties, several times over, among the others
        lat = ce.lattice_points()
        pts[:lat.shape[0] * 8] = np.tile(lat, (8, 1))
    g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert g.UploadScene(rows)
    scan_inf = g.ClosestPoint(pts)
    assert (scan_inf["prim"] >= 0).all() and not np.isnan(scan_inf["t"]).any()
    half = np.float32(np.median(scan_inf["t"]))
    batches = {"inf": ce.with_radius(pts, INF), "half": ce.with_radius(pts, half), "zero": ce.with_radius(pts, 0.0)}
    scan = {k: g.ClosestPoint(p) for k, p in batches.items()}
    assert ce.same_hits(scan["inf"], scan_inf) and 0.3 < (scan["half"]["prim"] >= 0).mean() < 0.7
    # the scan's own answers: the reported squared distance is the distance to the reported point
    q = g.ClosestPositions(pts[:4096], scan_inf[:4096])
    d2 = ((pts[:4096].astype(np.float64) - q) ** 2).sum(axis=1)
    scale = np.abs(pts[:4096]).max(axis=1) + np.abs(rows[:, :3]).max()
    assert (np.abs(np.sqrt(d2) - np.sqrt(scan_inf["t"][:4096].astype(np.float64))) <= ce.K * ce.EPS * scale).all()
    g.SetQueryAcceleration(True)
    assert g.QueryAccelInfo()["valid"] == 0
    for k, p in batches.items():
        got = g.ClosestPoint(p)
        bad = ce.differing(got, scan[k])
        print("%s %s: %d of %d rows differ" % (scene, k, bad.size, n))
        assert bad.size == 0, (scene, k, bad[:5], got[bad[:3]], scan[k][bad[:3]])
    info = g.QueryAccelInfo()
    assert info["valid"] == 1 and info["device_bytes"] > 0 and info["always_tested"] == 0
    if scene == "lattice":
        ties = scan_inf[:ce.lattice_points().shape[0]]
        assert (ties["t"] == 0).any() and (ties["t"] == 0.25).any()
    g.close()


def test_non_finite_triangles_are_always_tested_and_never_win_with_a_nan():
    rows = ce.random_scene(37, seed=3).reshape(-1, 3, 4)
    good = rows.reshape(-1, 4).copy()
    rows[3, 1, 0] = np.nan
    rows[10, 2, 2] = np.inf
    rows[20, 0, :3] = 3.0e38
    rows[20, 1, :3] = -3.0e38
    rows = rows.reshape(-1, 4)
    pts = ce.points_for(good, 2000, seed=4)
    tab = ce.table(pts, rows)
    assert np.isnan(tab[0][:, [3, 10, 20]]).any()
    for d2max in (INF, np.float32(4.0)):
        p = ce.with_radius(pts, d2max)
        exp = ce.winners(tab, p[:, 3])
        assert not np.isnan(exp["t"]).any() and (exp["prim"] >= 0).any()
        for mm in (0, 1):
            g = _tracer(mm)
            assert g.UploadScene(rows)
            _assert_same(g.ClosestPoint(p), exp, "non-finite scan mm=%d" % mm)
            g.SetQueryAcceleration(True)
            _assert_same(g.ClosestPoint(p), exp, "non-finite bvh mm=%d" % mm)
            assert g.QueryAccelInfo()["always_tested"] == 3
            g.close()


def test_zero_area_triangles_give_the_helpers_bits_in_both_modes():
    rows = ce.degenerate_scene()
    rng = np.random.default_rng(8)
    pts = np.concatenate([ce.points_for(rows, 1500, seed=7), rng.uniform(-3, 3, (500, 3)).astype(np.float32)])
    p = ce.with_radius(pts, INF)
    tab = ce.table(pts, rows)
    exp = ce.winners(tab, p[:, 3])
    degenerate = np.arange(3, 8)
    print("zero-area triangles win %d of %d points; their t is a NaN for %d pairs" %
          (int(np.isin(exp["prim"], degenerate).sum()), pts.shape[0], int(np.isnan(tab[0][:, degenerate]).sum())))
    for edges in (False, True):
        for mm in (0, 1):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            _assert_same(g.ClosestPoint(p), exp, "zero-area scan edges=%d mm=%d" % (edges, mm))
            g.SetQueryAcceleration(True)
            _assert_same(g.ClosestPoint(p), exp, "zero-area bvh edges=%d mm=%d" % (edges, mm))
            g.close()


def test_no_scene_spheres_only_empty_batch_and_bad_arguments():
    import raytracertest_amd as R
    L = R.api.load_library()
    pts = ce.with_radius(np.random.default_rng(2).uniform(-2, 2, (70, 3)).astype(np.float32), INF)
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        got = g.ClosestPoint(pts)                                        # no scene: nothing to be near to
        assert got.shape == (70,) and (got["prim"] == -1).all() and not got["t"].any() and not got["u"].any() and not got["v"].any()
        assert g.ClosestPoint(np.zeros((0, 4), np.float32)).shape == (0,)
        assert g.ClosestPoint(np.zeros((0, 3), np.float32)).shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can win
        _assert_same(g.ClosestPoint(pts), ce.expected(pts, None, spheres=SPHERES), "spheres only accel=%d" % accel)
        assert (g.ClosestPoint(pts)["prim"] == 0).all()
        _assert_same(g.ClosestPoint(pts[:, :3]), g.ClosestPoint(pts), "(n, 3) points")
        near = g.ClosestPoint(pts[:, :3], max_distance=0.5)
        _assert_same(near, ce.expected(ce.with_radius(pts, np.float32(0.5) * np.float32(0.5)), None, spheres=SPHERES), "max_distance")
        assert (near["prim"] == -1).any() and (near["prim"] == 0).any()
        assert (g.ClosestPoint(pts[:, :3], max_distance=-1.0)["prim"] == -1).all()
        out = np.zeros(70, HIT_DTYPE)
        assert L.rt_tracer_closest_point(g._h, None, 70, out.ctypes.data) == 1 and "null" in g.LastError()
        assert L.rt_tracer_closest_point(g._h, pts.ctypes.data, 70, None) == 1
        assert L.rt_tracer_closest_point(g._h, None, 0, None) == 0       # n = 0 is a no-op
        for bad in (np.zeros((4, 6), np.float32), np.float32(1.0)):
            with pytest.raises(ValueError):
                g.ClosestPoint(bad)
        g.close()


def test_torch_path_gives_the_same_bytes_and_a_misaligned_pointer_is_rejected():
    import torch
    import raytracertest_amd as R
    rows, fams, exp = _reference(1100)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for fam in ("inf", "half"):
            p = fams[fam]
            hits = g.ClosestPoint(p)
            _assert_same(hits, exp[(fam, True)], "numpy accel=%d %s" % (accel, fam))
            t = torch.from_numpy(p).to("cuda:0")
            th = g.ClosestPoint(t)
            assert th.dtype == torch.float32 and th.shape == (p.shape[0], 4) and th.device == t.device
            assert th.cpu().numpy().tobytes() == hits.tobytes()
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):                                   # on the caller's current stream
                th2 = g.ClosestPoint(t)
            s.synchronize()
            assert torch.equal(th2.view(torch.int32), th.view(torch.int32))
            assert g.ClosestPoint(t[:0]).shape == (0, 4)
        t3 = torch.from_numpy(np.ascontiguousarray(fams["inf"][:, :3])).to("cuda:0")
        assert g.ClosestPoint(t3).cpu().numpy().tobytes() == g.ClosestPoint(fams["inf"]).tobytes()
    t = torch.from_numpy(fams["inf"]).to("cuda:0")
    for bad in (t.cpu(), t.double(), t[:, :2].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.ClosestPoint(bad)
    flat = t.reshape(-1)
    out = torch.empty(8 * 4 + 4, dtype=torch.float32, device="cuda:0")
    assert L.rt_tracer_closest_point_device(g._h, flat.data_ptr() + 4, 8, out.data_ptr(), None) == 1     # misaligned points
    assert "16-byte" in g.LastError()
    assert L.rt_tracer_closest_point_device(g._h, flat.data_ptr(), 8, out.data_ptr() + 4, None) == 1     # misaligned answers
    assert "16-byte" in g.LastError()
    assert L.rt_tracer_closest_point_device(g._h, flat.data_ptr(), 8, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out[:32].cpu().numpy().tobytes() == exp[("inf", True)][:8].tobytes()
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    pts = ce.with_radius(ce.points_for(moved, 8192, seed=9), INF)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.ClosestPoint(pts)
    u0, built = g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
    assert u0["refits"] == 0 and built["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = g.ClosestPoint(pts)
    u1, info = g.QueryAccelUpdateInfo(), g.QueryAccelInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and info["valid"] == 1 and info["build_us"] == built["build_us"]
    g.SetQueryAcceleration(False)
    scan = g.ClosestPoint(pts)
    _assert_same(got, scan, "after the refit")
    assert ce.differing(first, scan).size > 0                            # the scene did move
    _assert_same(scan[:512], ce.expected(pts[:512], moved), "the moved scene against the helper")
    g.close()


def test_closest_point_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    pts = ce.with_radius(ce.points_for(rows, 4096, seed=7, spread=4.0), INF)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.ClosestPoint(pts)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.ClosestPoint(pts))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(20)
    assert len(got) == 20 and all(ce.same_hits(x, idle) for x in got) and (idle["prim"] >= 0).all()
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    pts = ce.points_for(rows, 2000, seed=3, spread=3.0)
    half = ce.radius_families(pts, rows)["half"]
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    exp = one.ClosestPoint(half)
    one.close()
    _assert_same(exp, ce.expected(half, rows), "one band against the helper")
    assert (exp["prim"] >= 0).any() and (exp["prim"] == -1).any()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_same(m.ClosestPoint(half), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_same(m.ClosestPoint(half), exp, "two bands, bvh")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()
