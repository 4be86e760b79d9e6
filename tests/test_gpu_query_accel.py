"""Ray queries through the BVH on the device (RT_QUERY_BVH): against the oracle's scan under every mode, layout and hit rule;
against the scan kernel on the same tracer for three ray populations and a frame of pinhole rays, on 10 000 and 200 000
triangles; FocusAt, rebuilds after uploads, a running Trace left alone, multi-device forwarding, and that it prunes.
A ray may differ from the scan only under the exclusion rule of query_accel_expect.check_against_scan."""
import time

import numpy as np
import pytest

from query_accel_expect import check_against_scan, populations
from query_expect import HIT_DTYPE, adversarial_rays, adversarial_scene, edge_rows, expected_hits, same_hits

pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)


def _tracer(math_mode=0, nearest=False, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, nearest_hit=nearest, **kw)


@pytest.mark.parametrize("n_tris", [1, 37, 300])
@pytest.mark.parametrize("spheres", [False, True])
def test_bvh_intersect_against_the_oracle_every_mode_and_layout(orc, n_tris, spheres):
    rows = adversarial_scene(n_tris, seed=n_tris)
    rays = adversarial_rays(rows, 160 if n_tris == 300 else 400, seed=n_tris + 1)
    sph = SPHERES if spheres else None
    for mm in (0, 1):
        contract = orc.FMA if mm == 0 else orc.STRICT
        for nearest in (False, True):
            exp = expected_hits(orc, rays, rows, sph, contract, nearest)
            assert (exp["prim"] >= 0).any() and (exp["prim"] < 0).any()
            for edges in (False, True):
                g = _tracer(mm, nearest)
                g.SetQueryAcceleration(True)
                assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
                if spheres:
                    g.UploadSpheres(SPHERES)
                got_all = g.Intersect(rays)
                info = g.QueryAccelInfo()
                assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0 and info["leaves"] >= 1
                for n in (rays.shape[0], 1, 63, 65):                    # partial waves
                    got = got_all if n == rays.shape[0] else g.Intersect(rays[:n])
                    assert got.dtype == HIT_DTYPE
                    check_against_scan(got, exp[:n], rays[:n], edge_rows(rows) if edges else rows, edges,
                                              "oracle n_tris=%d spheres=%d mm=%d nearest=%d edges=%d n=%d" % (n_tris, spheres, mm, nearest, edges, n))
                g.SetQueryAcceleration(False)                            # and back: the scan, bit for bit
                assert same_hits(g.Intersect(rays), exp) and g.QueryAccelInfo()["mode"] == 0
                g.close()


def test_non_finite_triangles_are_always_tested():
    rows = adversarial_scene(37, seed=3).reshape(-1, 3, 4)
    rows[3, 1, 0] = np.nan
    rows[10, 2, 2] = np.inf
    rows[20, 0, :3] = 3.0e38
    rows[20, 1, :3] = -3.0e38
    rows = rows.reshape(-1, 4)
    rays = adversarial_rays(adversarial_scene(37, seed=3), 600, seed=4)
    for nearest in (False, True):
        g = _tracer(0, nearest)
        assert g.UploadScene(rows)
        scan = g.Intersect(rays)
        g.SetQueryAcceleration(True)
        got = g.Intersect(rays)
        assert g.QueryAccelInfo()["always_tested"] == 3
        with np.errstate(all="ignore"):
            check_against_scan(got, scan, rays, rows, label="non-finite triangles nearest=%d" % nearest)
        g.close()


def test_no_scene_and_empty_batch():
    g = _tracer()
    g.SetQueryAcceleration(True)
    rays = np.array([[0, 0, 0, 0, 0, -1]] * 5, np.float32)
    h = g.Intersect(rays)
    assert (h["prim"] == -1).all() and (h["t"] == 0).all()
    assert g.Intersect(np.zeros((0, 6), np.float32)).shape == (0,)
    g.UploadSpheres(SPHERES)
    assert (g.Intersect(rays)["prim"] == 0).all()                     # spheres alone: prim = n_tris + sphere = 0
    import raytracertest_amd as R
    with pytest.raises(R.RtError, match="unknown mode"):
        g.SetQueryAcceleration(2)


def _frame_pixels(W, H):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
    return np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], 1))


@pytest.mark.parametrize("scene", ["c4_10k", "random_200k"])
def test_bvh_against_the_scan_on_the_device(scene):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "c4_10k" else scenes.random_triangles(200000, 77)
    W, H = 512, 288
    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert g.UploadScene(rows)
    pops = populations(rows, 1 << 18, seed=21)
    scan = {k: g.Intersect(r) for k, r in pops.items()}
    pix = _frame_pixels(W, H)
    scan_pick, pick_rays = g.Pick(pix, return_rays=True)
    fx, fy = (int(c) for c in pix[np.nonzero((scan_pick["prim"] >= 0) & (scan_pick["t"] > 0))[0][0]])
    f_scan = g.FocusAt(fx, fy)
    g.SetCameraParameters(70.0, 3.0, 0.05)
    g.SetQueryAcceleration(True)
    assert g.QueryAccelInfo()["valid"] == 0
    for k, r in pops.items():
        got = g.Intersect(r)
        assert (scan[k]["prim"] >= 0).mean() > 0.2, k
        check_against_scan(got, scan[k], r, rows, label="%s %s" % (scene, k))
    info = g.QueryAccelInfo()
    print(scene, info)
    assert info["valid"] == 1 and info["depth"] <= 16 and info["leaves"] * 4 >= rows.shape[0] // 3 and info["device_bytes"] > 0
    got_pick, rays2 = g.Pick(pix, return_rays=True)
    assert np.array_equal(rays2.view(np.uint32), pick_rays.view(np.uint32))
    check_against_scan(got_pick, scan_pick, pick_rays, rows, label="%s pinhole frame" % scene)
    g.SetCameraParameters(70.0, 3.0, 0.05)
    assert g.FocusAt(fx, fy) == f_scan
    # an upload between two BVH queries is seen by the second one
    built = g.QueryAccelInfo()
    small = scenes.cornell32()
    assert g.UploadScene(small)
    assert g.QueryAccelInfo()["valid"] == 0
    g.UploadSpheres(SPHERES)
    r = pops["origin"][:4096]
    got = g.Intersect(r)
    after = g.QueryAccelInfo()
    assert after["valid"] == 1 and after["leaves"] >= 8 and after["nodes"] < built["nodes"]
    g.UploadSpheres(np.zeros((0, 4), np.float32))
    assert g.QueryAccelInfo()["valid"] == 1                               # spheres do not touch the tree
    g.SetQueryAcceleration(False)
    g.UploadSpheres(SPHERES)
    check_against_scan(got, g.Intersect(r), r, small, label="%s after the upload" % scene)
    g.close()


def test_slack_1000_is_the_product_and_bare_boxes_are_answers_not_faults():
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    g = _tracer()
    assert g.UploadScene(rows)
    r = populations(rows, 1 << 16, seed=5)["near"]
    scan = g.Intersect(r)
    g.SetQueryAcceleration(True)
    a = g.Intersect(r)
    g.DebugQueryAccelSlack(1000)
    assert same_hits(a, g.Intersect(r))
    g.DebugQueryAccelSlack(0)
    bare = g.Intersect(r)                                                # may differ; every hit is still a real triangle hit
    print("bare boxes: %d of %d rays differ from the scan" % (int((bare["prim"] != scan["prim"]).sum()), r.shape[0]))
    assert ((bare["prim"] >= -1) & (bare["prim"] < 10000)).all()
    g.DebugQueryAccelSlack(1000)
    check_against_scan(g.Intersect(r), scan, r, rows, label="slack back at 1000")
    g.close()


def test_bvh_picks_do_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    pix = np.array([[1000, 500], [17, 3], [1919, 1079]], np.uint32)

    def run(picks, bvh):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Pick(pix)
        got = []
        g.Trace(24, 4, 2)
        if bvh:
            g.SetQueryAcceleration(True)                                 # the tree is built while the Trace runs
        for _ in range(picks):
            got.append(g.Pick(pix))
        assert g.Wait() == 1
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
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    pix = _frame_pixels(96, 64)
    scan = m.Pick(pix)
    m.SetQueryAcceleration(True)
    got, rays = m.Pick(pix, return_rays=True)
    info = m.QueryAccelInfo()
    assert info["mode"] == 1 and info["valid"] == 1 and info["leaves"] >= 8
    check_against_scan(got, scan, rays, rows, label="two bands")
    m.close()


def test_a_one_pixel_pick_prunes():
    """Relative to the scan in the same run: the median of 20 one-pixel picks on C4's scene through the tree (built beforehand)
    is below half the scan's.  A lane's dependent work falls from 10 000 triangle tests to tens of node visits."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    g = R.RayTracer((3840, 2160), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert g.UploadScene(scenes.random_triangles(10000, 12345))
    px = np.array([[1920, 1080]], np.uint32)

    def median_us(n=20):
        for _ in range(5):
            g.Pick(px)
        out = []
        for _ in range(n):
            t0 = time.perf_counter()
            g.Pick(px)
            out.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(out))

    scan_hit = g.Pick(px)
    scan = median_us()
    g.SetQueryAcceleration(True)
    assert same_hits(g.Pick(px), scan_hit) and g.QueryAccelInfo()["valid"] == 1
    bvh = median_us()
    print("one-pixel pick, C4 scene: scan %.1f us, BVH %.1f us (tree built in %d us)" % (scan, bvh, g.QueryAccelInfo()["build_us"]))
    assert bvh < 0.5 * scan
    g.close()
