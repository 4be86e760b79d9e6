"""The all-hits query on the device (RayTracer.IntersectAll): the scan against the oracle's ordered list, bit for bit with the
padding records, under both arithmetic modes, both layouts and both hit rules (which must not change a byte), for max_hits on
either side of both list capacities and batches that end in partial waves and blocks; the BVH mode under the contract of
allhits_expect.check_bvh_all_hits, against the oracle on adversarial inputs and against the scan kernel on a scene of stacked
sheets and on 10 000 random triangles; cross-checks against Occluded and Intersect on the same tracer; the torch path, argument
checks, uploads between calls, a running Trace left alone, multi-device forwarding and bare boxes."""
import numpy as np
import pytest

from allhits_expect import (check_bvh_all_hits, expected_all_hits, hit_table_uv, layered_scene, same_rows, sets_from_oracle,
                            sets_from_table, truncated)
from occluded_expect import interval_families, with_interval
from query_accel_expect import EXCLUSION_CAP, populations
from query_expect import FLT_MAX, HIT_DTYPE, adversarial_rays, adversarial_scene, edge_rows, same_hits

pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
INF = np.float32(np.inf)
NAN = np.float32(np.nan)
TINY = np.nextafter(np.float32(0), np.float32(1))


def _tracer(math_mode=0, nearest=False, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)


def adversarial_segments(rays, table, seed):
    """The four interval families of every ray, and around every distinct t* the oracle lists for a ray: [t*, t*], its two
    nextafter neighbours on either side, NaN bounds, tmin > tmax and the infinite intervals.  Shuffled, so that every prefix
    mixes them.  Returns (segments (m, 8), index of each segment's ray)."""
    n = rays.shape[0]
    segs = list(interval_families(rays, seed).values())
    idx = [np.arange(n)] * len(segs)
    hit, tt = table[0], table[1]
    w, p = np.nonzero(hit & ~np.isnan(tt))
    pairs = np.unique(np.c_[w, tt[w, p].view(np.uint32)], axis=0)
    w, t = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.uint32).view(np.float32)
    up, down = np.nextafter(t, INF), np.nextafter(t, -INF)
    for lo, hi in ((t, t), (up, INF), (-INF, down), (down, up), (t, INF), (-INF, t), (up, up), (down, down),
                   (NAN, INF), (-INF, NAN), (NAN, NAN), (up, down), (INF, -INF), (-INF, -INF), (INF, INF)):
        segs.append(with_interval(rays[w], lo, hi))
        idx.append(w)
    segs, idx = np.concatenate(segs), np.concatenate(idx)
    perm = np.random.default_rng(seed).permutation(segs.shape[0])
    return np.ascontiguousarray(segs[perm]), idx[perm]


def _assert_rows(got, exp, label):
    hits, counts = got
    assert hits.dtype == HIT_DTYPE and counts.dtype == np.uint32 and hits.shape == exp[0].shape and counts.shape == exp[1].shape, label
    bad = np.nonzero((hits.view(np.uint32).reshape(counts.shape[0], -1) != exp[0].view(np.uint32).reshape(counts.shape[0], -1)).any(axis=1)
                     | (counts != exp[1]))[0]
    assert bad.size == 0, (label, bad[:5], hits[bad[:2]], exp[0][bad[:2]], counts[bad[:5]], exp[1][bad[:5]])


@pytest.mark.parametrize("n_tris", [1, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_all_hits_against_the_oracle_every_mode_layout_rule_and_max_hits(orc, n_tris, spheres):
    rows = adversarial_scene(n_tris, seed=n_tris)
    rays = adversarial_rays(rows, 100 if n_tris == 1100 else 400, seed=n_tris + 1)
    sph = SPHERES if spheres else None
    excluded = 0
    for mm in (0, 1):
        contract = orc.FMA if mm == 0 else orc.STRICT
        table = hit_table_uv(orc, rays, rows, sph, contract)
        segs, idx = adversarial_segments(rays, table, seed=n_tris + 2)
        assert segs.shape[0] > 513
        exp16 = expected_all_hits(table, segs, 16, idx)
        assert (exp16[1] == 0).any() and (exp16[1] > 0).any()
        if n_tris >= 37:                                                 # truncation at 4 (37: up to 13 hits) and at 16, equal t inside a row
            assert (exp16[1] > 4).any() and ((exp16[1] == 16).any() or n_tris == 37)
            a, b = exp16[0][:, :-1], exp16[0][:, 1:]
            assert ((a["t"] == b["t"]) & (b["prim"] >= 0)).sum() > 50
        E, W = sets_from_table(table, segs, rows, idx)
        for edges in (False, True):
            answers = []
            for nearest in (False, True):
                g = _tracer(mm, nearest)
                assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
                if spheres:
                    g.UploadSpheres(SPHERES)
                label = "n_tris=%d spheres=%d mm=%d edges=%d nearest=%d" % (n_tris, spheres, mm, edges, nearest)
                blob = []
                for max_hits in (1, 3, 4, 5, 16):                        # both list capacities, each partly and fully used
                    exp = truncated(exp16, max_hits)
                    got_all = g.IntersectAll(segs, max_hits)
                    for n in (segs.shape[0], 1, 63, 65, 257, 513):       # partial waves, and a partial last block
                        got = got_all if n == segs.shape[0] else g.IntersectAll(segs[:n], max_hits)
                        _assert_rows(got, (exp[0][:n], exp[1][:n]), label + " max_hits=%d n=%d" % (max_hits, n))
                    blob.append(got_all[0].tobytes() + got_all[1].tobytes())
                    g.SetQueryAcceleration(True)
                    for n in (segs.shape[0], 1, 63, 65):
                        got = g.IntersectAll(segs[:n], max_hits)
                        excluded += check_bvh_all_hits(got, (exp[0][:n], exp[1][:n]), E, W, max_hits,
                                                       label="bvh " + label + " n=%d" % n)
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
                    g.SetQueryAcceleration(False)
                    back = g.IntersectAll(segs, max_hits)
                    assert back[0].tobytes() + back[1].tobytes() == blob[-1]
                answers.append(b"".join(blob))
                g.close()
            assert len(answers) == 2 and answers[0] == answers[1]        # the hit rule does not change a byte
    print("n_tris=%d spheres=%d: %d BVH answers used the exclusion" % (n_tris, spheres, excluded))


def test_cross_checks_against_occluded_and_intersect_on_the_same_tracer():
    rows = adversarial_scene(300, seed=9)
    rays = adversarial_rays(rows, 3000, seed=10)
    for mm in (0, 1):
        g = _tracer(mm, nearest=True)
        assert g.UploadScene(rows)
        g.UploadSpheres(SPHERES)
        for accel in (False, True):
            g.SetQueryAcceleration(False)
            near = g.Intersect(rays)
            assert (near["prim"] >= 0).sum() > 1000
            for fam, segs in interval_families(rays, seed=11).items():
                g.SetQueryAcceleration(False)
                occ = g.Occluded(segs)
                g.SetQueryAcceleration(accel)
                for max_hits in (1, 16):
                    _, counts = g.IntersectAll(segs, max_hits)
                    if not accel:
                        assert np.array_equal(counts > 0, occ), (mm, fam, max_hits)
                    else:                                                # (the traversal may lose ill-conditioned hits, never invent one)
                        assert (counts > 0).any() and not ((counts > 0) & ~occ).any(), (mm, fam, max_hits)
            g.SetQueryAcceleration(accel)
            if not accel:
                # the nearest hit in front of the origin, whatever the tracer's rule
                hits, counts = g.IntersectAll(with_interval(rays, TINY, np.nextafter(FLT_MAX, np.float32(0))), 1)
                assert same_hits(hits[:, 0], near) and np.array_equal(counts > 0, near["prim"] >= 0)
        g.close()


def test_no_scene_spheres_only_empty_batch_and_the_range_of_max_hits():
    import raytracertest_amd as R
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        segs = np.array([[0, 0, 0, 0, 0, -1, -INF, INF]] * 70, np.float32)
        hits, counts = g.IntersectAll(segs)
        assert hits.shape == (70, 16) and not counts.any() and (hits["prim"] == -1).all() and not hits["t"].any()
        hits, counts = g.IntersectAll(np.zeros((0, 8), np.float32), 3)
        assert hits.shape == (0, 3) and counts.shape == (0,)
        g.UploadSpheres(SPHERES)
        hits, counts = g.IntersectAll(segs, 5)                           # spheres alone can be hit: the ray meets 0, 1 and 3
        assert (counts == 3).all() and (hits["prim"][:, :3] == [3, 0, 1]).all() and (hits["prim"][:, 3:] == -1).all()
        assert (hits["t"][:, 0] < 0).all() and (hits["t"][:, 1] == hits["t"][:, 2]).all() and not hits["u"].any() and not hits["v"].any()
        segs[:, 6:] = [100.0, 200.0]
        assert not g.IntersectAll(segs, 5)[1].any()
        for bad in (0, 17, -1, 2.5):
            with pytest.raises(ValueError, match="max_hits"):
                g.IntersectAll(segs, bad)
        L = R.api.load_library()
        out = np.zeros((70, 17), HIT_DTYPE)
        cnt = np.zeros(70, np.uint32)
        for bad in (0, 17):
            assert L.rt_tracer_intersect_all(g._h, segs.ctypes.data, 70, bad, out.ctypes.data, cnt.ctypes.data) == 1
            assert "max_hits" in g.LastError()
        assert L.rt_tracer_intersect_all(g._h, segs.ctypes.data, 70, 4, None, cnt.ctypes.data) == 1
        assert L.rt_tracer_intersect_all(g._h, segs.ctypes.data, 70, 4, out.ctypes.data, None) == 1
        g.close()


def test_torch_path_gives_the_same_bytes_and_bad_arguments_raise():
    import torch
    import raytracertest_amd as R
    rows = adversarial_scene(300, seed=9)
    rays = adversarial_rays(rows, 3000, seed=10)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    segs = np.concatenate(list(interval_families(rays, seed=11).values()))
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for max_hits in (3, 16):
            hits, counts = g.IntersectAll(segs, max_hits)
            assert (counts == 0).any() and (counts > 1).any()
            t = torch.from_numpy(segs).to("cuda:0")
            th, tc = g.IntersectAll(t, max_hits)
            assert th.dtype == torch.float32 and th.shape == (segs.shape[0], max_hits, 4) and th.device == t.device
            assert tc.dtype == torch.int32 and tc.shape == (segs.shape[0],) and tc.device == t.device
            assert th.cpu().numpy().tobytes() == hits.tobytes() and np.array_equal(tc.cpu().numpy(), counts.view(np.int32))
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):                                   # on the caller's current stream
                th2, tc2 = g.IntersectAll(t, max_hits)
            s.synchronize()
            assert torch.equal(th2.view(torch.int32), th.view(torch.int32)) and torch.equal(tc2, tc)
            eh, ec = g.IntersectAll(t[:0], max_hits)
            assert eh.shape == (0, max_hits, 4) and ec.shape == (0,)
    t = torch.from_numpy(segs).to("cuda:0")
    for bad in (t.cpu(), t.double(), t[:, :6].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.IntersectAll(bad)
    with pytest.raises(ValueError, match="max_hits"):
        g.IntersectAll(t, 17)
    for bad in (rays[:8], segs.T, np.float32(1.0)):                      # numpy: (n, 6) rays are not taken for segments
        with pytest.raises(ValueError):
            g.IntersectAll(bad)
    one = g.IntersectAll(segs[0], 2)                                     # one segment, flat
    assert one[0].shape == (1, 2) and one[1].shape == (1,)
    L = R.api.load_library()
    flat = t.reshape(-1)
    out = torch.empty(8 * 4 * 4 + 4, dtype=torch.float32, device="cuda:0")
    cnt = torch.empty(8, dtype=torch.int32, device="cuda:0")
    assert L.rt_tracer_intersect_all_device(g._h, flat.data_ptr() + 4, 8, 4, out.data_ptr(), cnt.data_ptr(), None) == 1   # misaligned segments
    assert "16-byte" in g.LastError()
    assert L.rt_tracer_intersect_all_device(g._h, flat.data_ptr(), 8, 4, out.data_ptr() + 4, cnt.data_ptr(), None) == 1   # misaligned hits
    assert "16-byte" in g.LastError()
    g.close()


def test_non_finite_triangles_are_always_tested(orc):
    rows = adversarial_scene(37, seed=3).reshape(-1, 3, 4)
    rows[3, 1, 0] = np.nan
    rows[10, 2, 2] = np.inf
    rows[20, 0, :3] = 3.0e38
    rows[20, 1, :3] = -3.0e38
    rows = rows.reshape(-1, 4)
    rays = adversarial_rays(adversarial_scene(37, seed=3), 600, seed=4)
    g = _tracer()
    assert g.UploadScene(rows)
    for fam, segs in interval_families(rays, seed=5).items():
        with np.errstate(all="ignore"):
            E, W = sets_from_oracle(orc, segs, rows)
            for max_hits in (4, 16):
                g.SetQueryAcceleration(False)
                scan = g.IntersectAll(segs, max_hits)
                g.SetQueryAcceleration(True)
                got = g.IntersectAll(segs, max_hits)
                assert g.QueryAccelInfo()["always_tested"] == 3
                check_bvh_all_hits(got, scan, E, W, max_hits, label="non-finite triangles %s" % fam)
    g.close()


@pytest.mark.parametrize("scene", ["layered", "c4_10k"])
def test_bvh_against_the_scan_on_the_device(orc, scene):
    """layered_scene(48, 16, 5) on the CPU oracle, 7000 rays of each population (21 000 in all) over "any" and "forward": 0 rays
    have an ill-conditioned in-interval hit, so the populations stay far inside EXCLUSION_CAP / 4 on the reference alone.
    Rows that fill all 16 entries, by the same oracle on 500 "any" rays of each population: near 0.648, origin 0.658, far 0.124
    (a far origin looks at the stack from the side and leaves it through an edge) -- more than half of the rays that cross the
    stack, which is what the test asserts; pooled over the three populations the reference itself gives 0.477."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = layered_scene(48, 16, 5) if scene == "layered" else scenes.random_triangles(10000, 12345)
    g = R.RayTracer((512, 288), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert g.UploadScene(rows)
    pops = populations(rows, 1 << 16, seed=21)
    batches = {(k, f): s for k, r in pops.items() for f, s in interval_families(r, seed=22).items()}
    scan = {(key, m): g.IntersectAll(s, m) for key, s in batches.items() for m in (1, 4, 16)}
    for (key, m), (hits, counts) in scan.items():                        # the scan's own rows are ordered and padded
        a, b = hits[:, :-1], hits[:, 1:]
        filled = np.arange(1, m)[None, :] < counts[:, None]
        assert ((a["t"] < b["t"]) | ((a["t"] == b["t"]) & (a["prim"] < b["prim"])) | ~filled).all() and (counts <= m).all()
        inside = np.arange(m)[None, :] < counts[:, None]
        assert ((hits["prim"] >= 0) == inside).all() and not hits["t"][~inside].any() and (hits["prim"][~inside] == -1).all()
    if scene == "layered":
        share = {k: float((scan[((k, "any"), 16)][1] == 16).mean()) for k in pops}
        print("layered: share of the 'any' rays that fill 16 entries:", share, "all: %.3f" % np.mean(list(share.values())))
        assert share["near"] > 0.5 and share["origin"] > 0.5, share
    g.SetQueryAcceleration(True)
    assert g.QueryAccelInfo()["valid"] == 0
    used = 0
    for key, s in batches.items():
        E, W = sets_from_oracle(orc, s, rows)
        for m in (1, 4, 16):
            got = g.IntersectAll(s, m)
            used += check_bvh_all_hits(got, scan[(key, m)], E, W, m, cap=EXCLUSION_CAP, label="%s %s %s" % ((scene,) + key))
    info = g.QueryAccelInfo()
    print(scene, info, "rays that used the exclusion:", used)
    assert info["valid"] == 1 and info["device_bytes"] > 0
    # an upload between two BVH calls is seen by the second one
    small = scenes.cornell32()
    assert g.UploadScene(small)
    assert g.QueryAccelInfo()["valid"] == 0
    s = batches[("origin", "forward")][:4096]
    got = g.IntersectAll(s, 4)
    after = g.QueryAccelInfo()
    assert after["valid"] == 1 and after["nodes"] < info["nodes"]
    g.SetQueryAcceleration(False)
    small_scan = g.IntersectAll(s, 4)
    assert small_scan[1].any()
    E, W = sets_from_oracle(orc, s, small)
    check_bvh_all_hits(got, small_scan, E, W, 4, cap=EXCLUSION_CAP, label="%s after the upload" % scene)
    g.close()


def test_bare_boxes_are_answers_not_faults_and_one_sided():
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    g = _tracer()
    assert g.UploadScene(rows)
    segs = interval_families(populations(rows, 1 << 14, seed=5)["near"], seed=6)["any"]
    scan = g.IntersectAll(segs, 16)
    whole = scan[1] < 16                                                 # rows that hold the ray's whole exact set
    assert whole.mean() > 0.5
    g.SetQueryAcceleration(True)
    a = g.IntersectAll(segs, 16)
    g.DebugQueryAccelSlack(1000)
    assert same_rows(a, g.IntersectAll(segs, 16))
    g.DebugQueryAccelSlack(0)
    bare = g.IntersectAll(segs, 16)
    print("bare boxes: %d of %d rays lose a hit" % (int((bare[1] < scan[1])[whole].sum()), int(whole.sum())))
    assert (bare[1] <= scan[1])[whole].all()
    rays_whole = np.nonzero(whole)[0]
    listed = {(i, r.tobytes()) for i in rays_whole for r in scan[0][i, :scan[1][i]]}
    assert all((i, r.tobytes()) in listed for i in rays_whole for r in bare[0][i, :bare[1][i]])   # one-sided
    g.DebugQueryAccelSlack(1000)
    assert same_rows(a, g.IntersectAll(segs, 16))
    g.close()


def test_intersect_all_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    segs = interval_families(populations(rows, 4096, seed=7)["near"], seed=8)["forward"]

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.IntersectAll(segs, 4)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.IntersectAll(segs, 4))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(20)
    assert len(got) == 20 and all(same_rows(x, idle) for x in got[0::2])
    differ = [float(((x[0].view(np.uint32).reshape(4096, -1) != idle[0].view(np.uint32).reshape(4096, -1)).any(axis=1)).mean()) for x in got[1::2]]
    assert all(d <= EXCLUSION_CAP for d in differ), differ
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_forwards_to_its_first_band(orc):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    rng = np.random.default_rng(3)
    org = rng.uniform(-0.9, 0.9, (2000, 3)).astype(np.float32)
    org[:, 2] -= 2.0
    rays = np.ascontiguousarray(np.c_[org, rng.normal(0, 1, (2000, 3))], np.float32)
    fam = interval_families(rays, seed=4)
    segs = np.concatenate([fam["any"], fam["window"]])
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    exp = one.IntersectAll(segs, 6)
    one.close()
    assert (exp[1] > 1).any() and (exp[1] == 0).any()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    assert same_rows(m.IntersectAll(segs, 6), exp)
    m.SetQueryAcceleration(True)
    got = m.IntersectAll(segs, 6)
    assert m.QueryAccelInfo()["valid"] == 1
    E, W = sets_from_oracle(orc, segs, rows)
    check_bvh_all_hits(got, exp, E, W, 6, label="two bands")
    m.close()
