"""The visibility query on the device (RayTracer.Occluded / Visible): the scan against the oracle's OR over every primitive,
equal for every ray, under both arithmetic modes, both layouts, both hit rules (which must not change a byte) and every K
(rays per lane of the scan, forced by samples_in_flight, with batches that end in a partial block of each); the BVH mode
under the any-hit contract of occluded_expect.check_bvh_occluded, against the oracle on adversarial inputs and against the
scan kernel on 10 000 and 200 000 triangles; the torch path, argument checks, uploads between calls, a running Trace left
alone, multi-device forwarding and bare boxes."""
import numpy as np
import pytest

from occluded_expect import (check_bvh_occluded, expected_occluded, hit_table, interval_families, with_interval)
from query_accel_expect import EXCLUSION_CAP, populations
from query_expect import adversarial_rays, adversarial_scene, edge_rows

pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def _tracer(math_mode=0, nearest=False, K=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, nearest_hit=nearest,
                       samples_in_flight=K, **kw)


def adversarial_segments(rays, hits, seed):
    """The four interval families of every ray, and around the t* of every hit the tracer's own Intersect reports: [t*, t*],
    its two nextafter neighbours on either side, NaN bounds, tmin > tmax and the infinite intervals.  Shuffled, so that every
    prefix mixes them.  Returns (segments (m, 8), index of each segment's ray)."""
    n = rays.shape[0]
    segs = list(interval_families(rays, seed).values())
    idx = [np.arange(n)] * len(segs)
    w = np.nonzero(hits["prim"] >= 0)[0]
    t = hits["t"][w]
    up, down = np.nextafter(t, INF), np.nextafter(t, -INF)
    for lo, hi in ((t, t), (up, INF), (-INF, down), (down, up), (t, INF), (-INF, t), (up, up), (down, down),
                   (NAN, INF), (-INF, NAN), (NAN, NAN), (up, down), (INF, -INF), (-INF, -INF), (INF, INF)):
        segs.append(with_interval(rays[w], lo, hi))
        idx.append(w)
    segs, idx = np.concatenate(segs), np.concatenate(idx)
    perm = np.random.default_rng(seed).permutation(segs.shape[0])
    return np.ascontiguousarray(segs[perm]), idx[perm]


@pytest.mark.parametrize("n_tris", [1, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_occluded_against_the_oracle_every_mode_layout_rule_and_K(orc, n_tris, spheres):
    rows = adversarial_scene(n_tris, seed=n_tris)
    rays = adversarial_rays(rows, 100 if n_tris == 1100 else 400, seed=n_tris + 1)
    sph = SPHERES if spheres else None
    for mm in (0, 1):
        contract = orc.FMA if mm == 0 else orc.STRICT
        table = hit_table(orc, rays, rows, sph, contract)
        for edges in (False, True):
            def upload(g):
                assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
                if spheres:
                    g.UploadSpheres(SPHERES)

            # the cases are built around the reference rule's hits, once, so that every tracer below answers the same segments
            ref = _tracer(mm, nearest=False)
            upload(ref)
            segs, idx = adversarial_segments(rays, ref.Intersect(rays), seed=n_tris + 2)
            ref.close()
            assert segs.shape[0] > 1025
            sub = (table[0][idx], table[1][idx])
            exp = expected_occluded(orc, segs, rows, sph, contract, sub)
            assert exp.any() and (~exp).any()
            answers = []
            for nearest in (False, True):
                for K in (0, 1, 2, 4):                                   # 0: query_k's own choice; a block is 256 * K rays
                    g = _tracer(mm, nearest, K)
                    upload(g)
                    label = "n_tris=%d spheres=%d mm=%d edges=%d nearest=%d K=%d" % (n_tris, spheres, mm, edges, nearest, K)
                    got_all = g.Occluded(segs)
                    assert got_all.dtype == np.bool_ and got_all.shape == (segs.shape[0],)
                    for n in (segs.shape[0], 1, 63, 65, 257, 513, 1025):  # partial waves, and a partial last block of every K
                        got = got_all if n == segs.shape[0] else g.Occluded(segs[:n])
                        bad = np.nonzero(got != exp[:n])[0]
                        assert bad.size == 0, (label, n, bad[:5], segs[bad[:5]], exp[bad[:5]])
                        if n >= 63:
                            assert got.any() and (~got).any(), (label, n)  # every batch holds both answers
                    answers.append(got_all.tobytes())
                    if K == 0:                                           # (the traversal has no K)
                        g.SetQueryAcceleration(True)
                        for n in (segs.shape[0], 1, 63, 65):
                            got = g.Occluded(segs[:n])
                            check_bvh_occluded(got, exp[:n], segs[:n], rows, orc, sph, contract, table=(sub[0][:n], sub[1][:n]),
                                               label="bvh " + label + " n=%d" % n)
                        info = g.QueryAccelInfo()
                        assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
                        g.SetQueryAcceleration(False)
                        assert g.Occluded(segs).tobytes() == answers[-1]
                    g.close()
            assert len(answers) == 8 and all(a == answers[0] for a in answers)   # neither the hit rule nor K changes a byte


def test_no_scene_spheres_only_and_empty_batch():
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        segs = np.array([[0, 0, 0, 0, 0, -1, -INF, INF]] * 70, np.float32)
        assert not g.Occluded(segs).any()                                # no scene: nothing occludes
        assert g.Occluded(np.zeros((0, 8), np.float32)).shape == (0,)
        g.UploadSpheres(SPHERES)
        got = g.Occluded(segs)
        assert got.all()                                                  # spheres alone are enough
        segs[:, 6:] = [100.0, 200.0]
        assert not g.Occluded(segs).any()
        a = np.array([[0, 0, 0], [0, 0, 0], [5, 5, 0]], np.float32)
        b = np.array([[0.5, 0.3, -12.0], [0.0, 0.0, -1.0], [5, 5, -12.0]], np.float32)
        assert g.Visible(a, b).tolist() == [False, True, True]
        assert g.Visible(a, b, 0.0, 0.1).tolist() == [True, True, True]
        with pytest.raises(ValueError):
            g.Visible(a, b[:2])
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
        host = g.Occluded(segs)
        assert host.any() and (~host).any()
        t = torch.from_numpy(segs).to("cuda:0")
        out = g.Occluded(t)
        assert out.dtype == torch.uint8 and out.shape == (segs.shape[0],) and out.device == t.device
        assert np.array_equal(out.cpu().numpy(), host.view(np.uint8))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):                                       # on the caller's current stream
            out2 = g.Occluded(t)
        s.synchronize()
        assert torch.equal(out2, out)
        assert g.Occluded(t[:0]).shape == (0,)
    t = torch.from_numpy(segs).to("cuda:0")
    for bad in (t.cpu(), t.double(), t[:, :6].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.Occluded(bad)
    for bad in (rays[:8], segs.T, np.float32(1.0)):                      # numpy: (n, 6) rays are not taken for segments
        with pytest.raises(ValueError):
            g.Occluded(bad)
    assert g.Occluded(segs[0]).shape == (1,)                             # one segment, flat
    L = R.api.load_library()
    flat = t.reshape(-1)
    out = torch.empty(8, dtype=torch.uint8, device="cuda:0")
    assert L.rt_tracer_occluded_device(g._h, flat.data_ptr() + 4, 8, out.data_ptr(), None) == 1     # misaligned segments
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
        g.SetQueryAcceleration(False)
        scan = g.Occluded(segs)
        g.SetQueryAcceleration(True)
        got = g.Occluded(segs)
        assert g.QueryAccelInfo()["always_tested"] == 3
        with np.errstate(all="ignore"):
            check_bvh_occluded(got, scan, segs, rows, orc, label="non-finite triangles " + fam)
    g.close()


@pytest.mark.parametrize("scene", ["c4_10k", "random_200k"])
def test_bvh_against_the_scan_on_the_device(orc, scene):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "c4_10k" else scenes.random_triangles(200000, 77)
    g = R.RayTracer((512, 288), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert g.UploadScene(rows)
    pops = populations(rows, 1 << 18, seed=21)
    batches = {(k, f): s for k, r in pops.items() for f, s in interval_families(r, seed=22).items()}
    scan = {key: g.Occluded(s) for key, s in batches.items()}
    g.SetQueryAcceleration(True)
    assert g.QueryAccelInfo()["valid"] == 0
    for key, s in batches.items():
        got = g.Occluded(s)
        share = float(scan[key].mean())
        label = "%s %s %s" % ((scene,) + key)
        check_bvh_occluded(got, scan[key], s, rows, orc, cap=EXCLUSION_CAP, label=label)
        if scene == "c4_10k":
            assert 0.02 <= share <= 0.98, (label, share)
    info = g.QueryAccelInfo()
    print(scene, info)
    assert info["valid"] == 1 and info["device_bytes"] > 0
    # an upload between two BVH calls is seen by the second one
    small = scenes.cornell32()
    assert g.UploadScene(small)
    assert g.QueryAccelInfo()["valid"] == 0
    s = batches[("origin", "forward")][:4096]
    got = g.Occluded(s)
    after = g.QueryAccelInfo()
    assert after["valid"] == 1 and after["nodes"] < info["nodes"]
    g.SetQueryAcceleration(False)
    small_scan = g.Occluded(s)
    assert small_scan.any()
    check_bvh_occluded(got, small_scan, s, small, orc, cap=EXCLUSION_CAP, label="%s after the upload" % scene)
    g.close()


def test_bare_boxes_are_answers_not_faults_and_one_sided():
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    g = _tracer()
    assert g.UploadScene(rows)
    segs = interval_families(populations(rows, 1 << 16, seed=5)["near"], seed=6)["any"]
    scan = g.Occluded(segs)
    g.SetQueryAcceleration(True)
    a = g.Occluded(segs)
    g.DebugQueryAccelSlack(1000)
    assert np.array_equal(a, g.Occluded(segs))
    g.DebugQueryAccelSlack(0)
    bare = g.Occluded(segs)
    print("bare boxes: %d of %d rays lose their occluder" % (int((scan & ~bare).sum()), segs.shape[0]))
    assert not (bare & ~scan).any()                                      # BVH = 1 implies scan = 1
    g.DebugQueryAccelSlack(1000)
    assert np.array_equal(a, g.Occluded(segs))
    g.close()


def test_occluded_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    segs = interval_families(populations(rows, 4096, seed=7)["near"], seed=8)["forward"]

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Occluded(segs)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.Occluded(segs))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(20)
    assert len(got) == 20 and all(np.array_equal(x, idle) for x in got[0::2])
    assert all(not (x & ~idle).any() and (x != idle).mean() <= EXCLUSION_CAP for x in got[1::2])
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
    segs = interval_families(rays, seed=4)["window"]
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    exp = one.Occluded(segs)
    one.close()
    assert exp.any() and (~exp).any()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    assert np.array_equal(m.Occluded(segs), exp)
    m.SetQueryAcceleration(True)
    got = m.Occluded(segs)
    assert m.QueryAccelInfo()["valid"] == 1
    check_bvh_occluded(got, exp, segs, rows, orc, label="two bands")
    m.close()
