"""The k-nearest point query on the device (RayTracer.ClosestAll / ClosestWithin): the scan and the BVH walk against the numpy
restatement of nearest_expect, bit for bit, rows and counts, for both upload layouts, both arithmetic modes (which must not
change a byte), with and without spheres, six search radii, max_hits on both sides of the list-capacity switch and batches that
end in partial waves and blocks; record 0 against ClosestPoint; the BVH walk against the scan kernel on 65 536 points of a scene
of stacked sheets, of 10 000 random triangles and of a lattice whose ties the cut falls into; the continuation cursor; non-finite
and zero-area triangles; the torch path, argument checks, a refitted tree, a running Trace left alone and multi-device
forwarding."""
import functools
import hashlib

import numpy as np
import pytest

import closest_expect as ce
import nearest_expect as ne
from query_expect import HIT_DTYPE, edge_rows

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
# two coincident spheres (a tie between spheres: both are listed, the lower prim first), one the points are inside or near, one far away
SPHERES = np.array([[0.5, 0.3, -1.0, 0.8], [0.5, 0.3, -1.0, 0.8], [40.0, -35.0, 20.0, 6.0]], np.float32)
COUNTS = (1, 63, 64, 65)                                                 # partial waves; 4097 is a partial last block as well
KS = (1, 3, 4, 5, 16)                                                    # 4 | 5: the list of 4 slots gives way to the one of 16


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _assert_rows(got, exp, label):
    hits, counts = got
    assert hits.dtype == HIT_DTYPE and hits.shape == exp[0].shape and counts.dtype == np.uint32 and counts.shape == exp[1].shape, label
    bad = ne.differing_rows(hits, exp[0], counts, exp[1])
    assert bad.size == 0, (label, bad.size, bad[:5], hits[bad[:2]], exp[0][bad[:2]], counts[bad[:3]], exp[1][bad[:3]])


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, 4097 points, the six radius families and the expected rows of 16 without and with SPHERES: one table and one
    sort for all (a shorter row is the longer one cut)."""
    rows = ce.random_scene(n_tris, seed=100 + n_tris)
    pts = ce.points_for(rows, 4097, seed=200 + n_tris)
    tab = ce.table(pts, rows, spheres=SPHERES)
    bare = tuple(x[:, :n_tris] for x in tab)
    fams = {"inf": ce.with_radius(pts, INF), "kth6": ce.with_radius(pts, ne.kth_radius(bare, 6)),
            "kth20": ce.with_radius(pts, ne.kth_radius(bare, 20)), "zero": ce.with_radius(pts, 0.0),
            "nan": ce.with_radius(pts, np.nan), "negative": ce.with_radius(pts, -1.0)}
    exp = {}
    for sph, tb in ((False, bare), (True, tab)):
        order = ne.presort(tb)
        for fam, p in fams.items():
            exp[(fam, sph)] = ne.expected_all(tb, p[:, 3], 16, order=order)
            for x in exp[(fam, sph)]:
                x.setflags(write=False)
    return rows, fams, exp, bare, tab


def test_the_families_saturate_and_leave_room_as_intended():
    _, fams, exp, _, _ = _reference(1100)
    assert (exp[("kth6", False)][1] == 6).all() and (exp[("kth20", False)][1] == 16).all() and (exp[("inf", False)][1] == 16).all()
    assert not exp[("nan", True)][1].any() and not exp[("negative", True)][1].any() and exp[("zero", False)][1].any()
    assert (exp[("inf", True)][0]["prim"] >= 1100).any()
    prim = exp[("inf", True)][0]["prim"]                                 # the coincident spheres: listed together, in prim order
    first = prim[:, :15] == 1100
    assert first.any() and (prim[:, 1:][first] == 1101).all()
    _, _, exp5, _, _ = _reference(5)
    assert (exp5[("inf", False)][1] == 5).all() and (exp5[("inf", True)][1] == 8).all()


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_radius_max_hits_and_count(n_tris, spheres):
    rows, fams, exp, _, _ = _reference(n_tris)
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
                for fam, p in fams.items():
                    for k in KS:
                        label = "n_tris=%d spheres=%d edges=%d mm=%d accel=%d %s k=%d" % (n_tris, spheres, edges, mm, accel, fam, k)
                        want = ne.cut(*exp[(fam, spheres)], k)
                        got = g.ClosestAll(p, k)
                        _assert_rows(got, want, label)
                        blob.update(got[0].tobytes())
                        blob.update(got[1].tobytes())
                        if fam in ("inf", "kth6"):
                            for n in COUNTS:
                                _assert_rows(g.ClosestAll(p[:n], k), (want[0][:n], want[1][:n]), label + " n=%d" % n)
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


@pytest.mark.parametrize("mm", [0, 1])
def test_record_0_of_every_row_is_closest_points_answer_for_every_max_hits(mm):
    rows, fams, _, _, _ = _reference(1100)
    g = _tracer(mm)
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for fam in ("inf", "kth6", "zero", "nan"):
            one = g.ClosestPoint(fams[fam])
            for k in range(1, 17):
                hits, counts = g.ClosestAll(fams[fam], k)
                assert ce.same_hits(hits[:, 0], one), (mm, accel, fam, k)
                assert np.array_equal(counts > 0, one["prim"] >= 0)
    g.close()


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
    nearest = g.ClosestPoint(pts)
    median = np.float32(np.median(nearest["t"]))
    batches = {"inf": ce.with_radius(pts, INF), "median": ce.with_radius(pts, median), "zero": ce.with_radius(pts, 0.0)}
    scan = {(r, k): g.ClosestAll(p, k) for r, p in batches.items() for k in (4, 16)}
    assert (scan[("inf", 16)][1] == 16).all() and 0.3 < (scan[("median", 4)][1] > 0).mean() < 0.7
    assert ce.same_hits(scan[("inf", 4)][0][:, 0], nearest)
    if scene == "lattice":                                               # the cut falls inside groups of equal t
        t = scan[("inf", 16)][0]["t"][:ce.lattice_points().shape[0]]
        assert (t[:, 3] == t[:, 4]).mean() > 0.8 and (t[:, 0] == t[:, 1]).all()
    g.SetQueryAcceleration(True)
    assert g.QueryAccelInfo()["valid"] == 0
    for (r, k), exp in scan.items():
        hits, counts = g.ClosestAll(batches[r], k)
        bad_rows = ne.differing_rows(hits, exp[0])
        bad_counts = np.nonzero(counts != exp[1])[0]
        print("%s %s max_hits=%d: %d of %d rows and %d counts differ" % (scene, r, k, bad_rows.size, n, bad_counts.size))
        assert bad_rows.size == 0 and bad_counts.size == 0, (scene, r, k, bad_rows[:5], hits[bad_rows[:2]], exp[0][bad_rows[:2]])
    info = g.QueryAccelInfo()
    assert info["valid"] == 1 and info["always_tested"] == 0
    g.close()


def test_closest_within_enumerates_everything_through_the_cursor():
    import lattice_cases as lc
    rows = ce.random_scene(37, seed=137)
    pts = ce.points_for(rows, 257, seed=237)
    full = ne.accepted_lists(ce.table(pts, rows), INF)
    lat_rows, lat = lc.rooms(), ce.lattice_points()
    lat_full = ne.accepted_lists(ce.table(lat, lat_rows), np.float32(0.25))
    assert max(h.shape[0] for h in lat_full) > 16
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        assert g.UploadScene(rows)
        for k in (4, 16):
            hits, offsets = g.ClosestWithin(pts, np.inf, k)
            assert hits.dtype == HIT_DTYPE and offsets.shape == (258,) and (np.diff(offsets) == 37).all()
            assert ne.same_rows(hits, np.concatenate(full)), (accel, k)
        # by hand, 10 rounds of 4: no repeat, no loss
        got, rounds = ne.chain(lambda live, after: g.ClosestAll(ce.with_radius(pts[live], INF), 4, after=after), 257, 4, rounds=10)
        assert rounds == 10 and all(ne.same_rows(a, b) for a, b in zip(got, full))
        assert g.UploadScene(lat_rows)                                   # a finite radius; cuts inside groups of equal t
        for k in (4, 5):
            hits, offsets = g.ClosestWithin(lat, 0.5, k)
            assert np.array_equal(np.diff(offsets), [h.shape[0] for h in lat_full])
            assert ne.same_rows(hits, np.concatenate(lat_full)), (accel, k)
        hits, offsets = g.ClosestWithin(ce.with_radius(lat, -1.0), 0.0)  # (n, 4): the column decides; nothing within
        assert hits.shape == (0,) and not offsets.any()
        g.close()


def test_cursor_argument_cases():
    rows, fams, exp, bare, _ = _reference(37)
    p = fams["inf"]
    n = p.shape[0]
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        assert g.UploadScene(rows)
        for k in (4, 16):
            base = ne.cut(*exp[("inf", False)], k)
            none = ne.no_cursor(n)
            none["t"], none["u"] = np.float32(np.nan), 7.0               # prim == NONE: no cursor, whatever else it holds
            _assert_rows(g.ClosestAll(p, k, after=none), base, "prim none")
            nan = ne.no_cursor(n)
            nan["t"], nan["prim"] = np.float32(np.nan), 5
            hits, counts = g.ClosestAll(p, k, after=nan)                 # a NaN cursor t accepts nothing
            assert not counts.any() and (hits["prim"] == -1).all() and not hits["t"].any()
            mixed = base[0][:, k - 1].copy()                             # every second point continues, the others start over
            mixed["prim"][1::2] = -1
            mixed["u"], mixed["v"] = np.float32(np.nan), -3.0            # u and v of the cursor are ignored
            _assert_rows(g.ClosestAll(p, k, after=mixed), ne.expected_all(bare, INF, k, after=mixed), "mixed k=%d" % k)
            low = ne.no_cursor(n)
            low["prim"] = -2                                             # int32 comparison: t = 0 ties go behind prim -2
            _assert_rows(g.ClosestAll(p, k, after=low), ne.expected_all(bare, INF, k, after=low), "prim -2")
        with pytest.raises(ValueError):
            g.ClosestAll(p, 4, after=ne.no_cursor(n - 1))
        with pytest.raises(ValueError):
            g.ClosestAll(p, 4, after=np.zeros((n, 4), np.float32))
        g.close()


def test_non_finite_and_zero_area_triangles():
    rows = ce.random_scene(37, seed=3).reshape(-1, 3, 4)
    good = rows.reshape(-1, 4).copy()
    rows[3, 1, 0] = np.nan
    rows[10, 2, 2] = np.inf
    rows[20, 0, :3] = 3.0e38
    rows[20, 1, :3] = -3.0e38
    rows = rows.reshape(-1, 4)
    cases = [("non-finite", rows, ce.points_for(good, 2000, seed=4), 3)]   # (the three are in the always-tested list)
    deg = ce.degenerate_scene()
    cases.append(("zero-area", deg, np.concatenate([ce.points_for(deg, 1500, seed=7),
                                                    np.random.default_rng(8).uniform(-3, 3, (500, 3)).astype(np.float32)]), None))
    for name, r, pts, always in cases:
        tab = ce.table(pts, r)
        order = ne.presort(tab)
        for d2max in (INF, np.float32(4.0)):
            p = ce.with_radius(pts, d2max)
            for k in (4, 16):
                exp = ne.expected_all(tab, p[:, 3], k, order=order)
                assert not np.isnan(exp[0]["t"]).any() and exp[1].any()
                for mm in (0, 1):
                    g = _tracer(mm)
                    assert g.UploadScene(r)
                    _assert_rows(g.ClosestAll(p, k), exp, "%s scan mm=%d k=%d" % (name, mm, k))
                    g.SetQueryAcceleration(True)
                    _assert_rows(g.ClosestAll(p, k), exp, "%s bvh mm=%d k=%d" % (name, mm, k))
                    assert always is None or g.QueryAccelInfo()["always_tested"] == always
                    g.close()


def test_non_finite_points_take_no_pruning_decision():
    rows, _, _, _, _ = _reference(1100)
    pts = ce.points_for(rows, 256, seed=5)
    pts[::4, 0] = np.inf
    pts[1::8, 1] = np.nan
    pts[2::16, 2] = -np.inf
    p = ce.with_radius(pts, INF)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    for k in (4, 16):
        scan = g.ClosestAll(p, k)
        assert (scan[1][3::16] == k).all()                               # (the finite ones among them)
        g.SetQueryAcceleration(True)
        _assert_rows(g.ClosestAll(p, k), scan, "bvh")
        g.SetQueryAcceleration(False)
    g.close()


def test_no_scene_spheres_only_empty_batch_and_bad_arguments():
    import raytracertest_amd as R
    L = R.api.load_library()
    pts = ce.with_radius(np.random.default_rng(2).uniform(-2, 2, (70, 3)).astype(np.float32), INF)
    sph_tab = ce.table(pts, None, spheres=SPHERES)
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        hits, counts = g.ClosestAll(pts, 5)                              # no scene: nothing to be near to
        assert hits.shape == (70, 5) and not counts.any() and (hits["prim"] == -1).all() and not hits["t"].any()
        for empty in (np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32)):
            hits, counts = g.ClosestAll(empty, 3)
            assert hits.shape == (0, 3) and counts.shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        for k in KS:
            _assert_rows(g.ClosestAll(pts, k), ne.expected_all(sph_tab, INF, k), "spheres only accel=%d k=%d" % (accel, k))
        assert (g.ClosestAll(pts, 16)[1] == 3).all()
        _assert_rows(g.ClosestAll(pts[:, :3]), g.ClosestAll(pts), "(n, 3) points")
        near = g.ClosestAll(pts[:, :3], 4, max_distance=0.5)
        _assert_rows(near, ne.expected_all(sph_tab, np.float32(0.5) * np.float32(0.5), 4), "max_distance")
        assert (near[1] == 0).any() and (near[1] == 2).any()
        assert not g.ClosestAll(pts[:, :3], 4, max_distance=-1.0)[1].any()
        out = np.zeros((70, 4), HIT_DTYPE)
        cnt = np.zeros(70, np.uint32)
        assert L.rt_tracer_closest_all(g._h, None, None, 70, 4, out.ctypes.data, cnt.ctypes.data) == 1 and "null" in g.LastError()
        assert L.rt_tracer_closest_all(g._h, pts.ctypes.data, None, 70, 4, None, cnt.ctypes.data) == 1
        assert L.rt_tracer_closest_all(g._h, pts.ctypes.data, None, 70, 4, out.ctypes.data, None) == 1
        for k in (0, 17):
            assert L.rt_tracer_closest_all(g._h, pts.ctypes.data, None, 70, k, out.ctypes.data, cnt.ctypes.data) == 1
            assert "max_hits" in g.LastError()
            with pytest.raises(ValueError):
                g.ClosestAll(pts, k)
        assert L.rt_tracer_closest_all(g._h, None, None, 0, 4, None, None) == 0         # n = 0 is a no-op
        for bad in (np.zeros((4, 6), np.float32), np.float32(1.0)):
            with pytest.raises(ValueError):
                g.ClosestAll(bad)
        g.close()


def test_torch_path_on_a_side_stream_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, fams, exp, _, _ = _reference(1100)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for fam, k in (("inf", 16), ("kth6", 4), ("kth6", 5)):
            p = fams[fam]
            hits, counts = g.ClosestAll(p, k)
            _assert_rows((hits, counts), ne.cut(*exp[(fam, True)], k), "numpy accel=%d %s" % (accel, fam))
            t = torch.from_numpy(p).to("cuda:0")
            th, tc = g.ClosestAll(t, k)
            assert th.dtype == torch.float32 and th.shape == (p.shape[0], k, 4) and tc.dtype == torch.int32 and tc.shape == (p.shape[0],)
            assert th.cpu().numpy().tobytes() == hits.tobytes() and tc.cpu().numpy().tobytes() == counts.tobytes()
            after = th[:, k - 1, :].contiguous()                         # the cursor as a tensor: the next page
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):                                   # on the caller's current stream
                th2, tc2 = g.ClosestAll(t, k)
                nh, nc = g.ClosestAll(t, k, after=after)
            s.synchronize()
            assert torch.equal(th2.view(torch.int32), th.view(torch.int32)) and torch.equal(tc2, tc)
            page2 = g.ClosestAll(p, k, after=np.ascontiguousarray(hits[:, k - 1]))
            assert nh.cpu().numpy().tobytes() == page2[0].tobytes() and nc.cpu().numpy().tobytes() == page2[1].tobytes()
            th0, tc0 = g.ClosestAll(t[:0], k)
            assert th0.shape == (0, k, 4) and tc0.shape == (0,)
        t3 = torch.from_numpy(np.ascontiguousarray(fams["inf"][:, :3])).to("cuda:0")
        assert g.ClosestAll(t3, 4)[0].cpu().numpy().tobytes() == g.ClosestAll(fams["inf"], 4)[0].tobytes()
    t = torch.from_numpy(fams["inf"]).to("cuda:0")
    for bad in (t.cpu(), t.double(), t[:, :2].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.ClosestAll(bad, 4)
    for bad_after in (t.cpu(), t[:-1].contiguous(), t.double(), ne.no_cursor(t.shape[0])):
        with pytest.raises(ValueError):
            g.ClosestAll(t, 4, after=bad_after)
    flat = t.reshape(-1)
    out = torch.empty(8 * 4 * 4 + 4, dtype=torch.float32, device="cuda:0")
    cnt = torch.empty(8, dtype=torch.int32, device="cuda:0")
    cur = torch.full((8 * 4 + 4,), -1, dtype=torch.int32, device="cuda:0").view(torch.float32)
    P, O, Cn, A = flat.data_ptr(), out.data_ptr(), cnt.data_ptr(), cur.data_ptr()
    for args in ((P + 4, None, 8, 4, O, Cn), (P, A + 4, 8, 4, O, Cn), (P, None, 8, 4, O + 4, Cn)):   # misaligned pts, after, hits
        assert L.rt_tracer_closest_all_device(g._h, *args, None) == 1
        assert "16-byte" in g.LastError()
    for args in ((None, None, 8, 4, O, Cn), (P, None, 8, 4, None, Cn), (P, None, 8, 4, O, None)):
        assert L.rt_tracer_closest_all_device(g._h, *args, None) == 1
    assert L.rt_tracer_closest_all_device(g._h, None, None, 0, 4, None, None, None) == 0
    assert L.rt_tracer_closest_all_device(g._h, P, A, 8, 4, O, Cn, None) == 0
    torch.cuda.synchronize()
    want = ne.cut(exp[("inf", True)][0][:8], exp[("inf", True)][1][:8], 4)
    assert out[:128].cpu().numpy().tobytes() == want[0].tobytes() and cnt.cpu().numpy().tobytes() == want[1].tobytes()
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
    first = g.ClosestAll(pts, 16)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = {k: g.ClosestAll(pts, k) for k in (16, 4)}                     # the first of them refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    for k in (16, 4):
        _assert_rows(got[k], g.ClosestAll(pts, k), "after the refit k=%d" % k)
    assert ne.differing_rows(first[0], got[16][0]).size > 0             # the scene did move
    _assert_rows(tuple(x[:512] for x in got[16]), ne.expected_all(ce.table(pts[:512], moved), INF, 16), "the moved scene against the helper")
    g.close()


def test_closest_all_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    pts = ce.with_radius(ce.points_for(rows, 4096, seed=7, spread=4.0), INF)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.ClosestAll(pts, 16)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.ClosestAll(pts, 16 if i % 4 < 2 else 4))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(8)
    assert len(got) == 8 and (idle[1] == 16).all()
    for h, c in got:
        k = h.shape[1]
        assert ne.same_rows(h, idle[0][:, :k]) and (c == k).all()
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    pts = ce.points_for(rows, 2000, seed=3, spread=3.0)
    tab = ce.table(pts, rows)
    p = ce.with_radius(pts, ne.kth_radius(tab, 6))
    exp = ne.expected_all(tab, p[:, 3], 4)
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_rows(one.ClosestAll(p, 4), exp, "one band against the helper")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_rows(m.ClosestAll(p, 4), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_rows(m.ClosestAll(p, 4), exp, "two bands, bvh")
    page2 = m.ClosestAll(p, 4, after=np.ascontiguousarray(exp[0][:, 3]))
    _assert_rows(page2, ne.expected_all(tab, p[:, 3], 4, after=np.ascontiguousarray(exp[0][:, 3])), "two bands, the cursor")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()
