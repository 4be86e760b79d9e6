"""The exposure query on the device (RayTracer.Exposure / AmbientOcclusion).  The yardstick is Occluded, not the code under test:
in every case masks == pack_masks(~Occluded(exposure_segments(...))) byte for byte, Occluded called in the same query mode and, on
the small scenes, itself checked against the oracle's OR over every primitive.  Scenes of 1, 37 and 1 100 triangles (the last
crosses an LDS chunk) with and without spheres, the open box against its analytic rule, the rooms lattice with points on its
walls; both layouts, both arithmetic modes, scan and BVH; 1, 2, 63 and 64 directions; 1, 3, 4, 5 and 257 points (partial blocks
of one and three live waves); the device's rays against the numpy restatement; flags, intervals, argument rules; torch tensors on
a side stream, a running Trace left alone, a two-band handle, re-uploaded scenes; the Python helpers."""

import numpy as np
import pytest

import exposure_expect as ee
from lattice_cases import SHIFT, rooms
from occluded_expect import check_bvh_occluded, expected_occluded, hit_table, in_interval
from query_expect import adversarial_rays, adversarial_scene, edge_rows

pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
INF = np.float32(np.inf)
NAN = np.float32(np.nan)
ALL64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _dirs():
    from raytracertest_amd import api
    return ee.as_dirs4(api.hemisphere_directions(64))


def _low(k):
    return ALL64 if k == 64 else np.uint64((1 << k) - 1)


def _same_as_occluded(g, pts, dirs, world=False, label=""):
    """The yardstick: Exposure's masks against Occluded of the restated segments, in the tracer's current query mode."""
    masks = g.Exposure(pts, dirs, world=world)
    n, k = np.asarray(pts).reshape(-1, 8).shape[0], dirs.shape[0]
    assert masks.dtype == np.uint64 and masks.shape == (n,)
    segs = ee.exposure_segments(pts, dirs, world=world)
    occ = g.Occluded(segs)
    want = ee.pack_masks(~occ.reshape(n, k))
    bad = np.nonzero(masks != want)[0]
    assert bad.size == 0, (label, n, k, bad[:5], [hex(int(x)) for x in masks[bad[:3]]], [hex(int(x)) for x in want[bad[:3]]])
    assert not (masks & ~_low(k)).any(), (label, n, k)                    # bits >= n_dirs are zero
    return masks, segs, occ


def _scene_points(rows, n, seed):
    """n points around an adversarial scene: the origins of its adversarial rays (NaN, infinite and huge ones among them), random
    unit normals with the special ones in front, windows of t."""
    rng = np.random.default_rng(seed)
    rays = adversarial_rays(rows, n, seed=seed)
    pick = rng.permutation(rays.shape[0])[:n]
    p = np.zeros((n, 8), np.float32)
    p[:, :3] = rays[pick, :3]
    p[:, 3:6] = ee.unit_normals(n, seed + 1)
    sp = ee.special_normals()
    p[1:1 + min(n - 1, sp.shape[0]), 3:6] = sp[:max(min(n - 1, sp.shape[0]), 0)]
    p[:, 6] = rng.uniform(-0.5, 0.5, n)
    p[:, 7] = np.where(rng.uniform(size=n) < 0.5, INF, p[:, 6] + rng.uniform(0.0, 12.0, n)).astype(np.float32)
    p[0, :3], p[0, 3:6], p[0, 6:] = [0.1, -0.2, 0.3], [0.0, 0.0, -1.0], [1e-3, INF]   # one plain point that looks into the scene
    return p


@pytest.mark.parametrize("n_tris", [1, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_masks_equal_occluded_every_scene_layout_mode_and_count(orc, n_tris, spheres):
    rows = adversarial_scene(n_tris, seed=n_tris)
    sph = SPHERES if spheres else None
    pts = _scene_points(rows, 257, seed=n_tris + 5)
    dirs = _dirs()
    seen = set()
    for mm in (0, 1):
        contract = orc.FMA if mm == 0 else orc.STRICT
        few = ee.exposure_segments(pts[:3], dirs)                         # the yardstick itself against the oracle
        table = hit_table(orc, few, rows, sph, contract)
        exp_few = in_interval(few, table).any(axis=1)
        for edges in (False, True):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            if spheres:
                g.UploadSpheres(SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                label = "n_tris=%d spheres=%d mm=%d edges=%d accel=%d" % (n_tris, spheres, mm, edges, accel)
                occ_few = g.Occluded(few)
                if accel:
                    with np.errstate(all="ignore"):
                        check_bvh_occluded(occ_few, exp_few, few, rows, orc, sph, contract, table=table, label=label)
                else:
                    assert np.array_equal(occ_few, exp_few), label
                for n in (257, 1, 3, 4, 5):                               # partial blocks of one and of three live waves
                    for k in (64, 1, 2, 63):
                        masks, _, occ = _same_as_occluded(g, pts[:n], dirs[:k], label=label)
                        if n == 257 and k == 64:
                            seen.add((bool(occ.any()), bool((~occ).any())))
                for k in (64, 63):
                    _same_as_occluded(g, pts, dirs[:k], world=True, label=label + " world")
            g.close()
    assert (True, True) in seen                                           # the batches hold both answers


def _rooms_points():
    """Points on the walls of rooms(): face interiors of outer and inner walls with the wall's normal either way, origins on the
    surface with tmin = 0 and tmin = 1e-3."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in (0, 2, 4):
            for sgn in (1.0, -1.0):
                for tmin in (0.0, 1e-3):
                    p = np.zeros(8, np.float32)
                    p[a], p[b], p[c] = k - SHIFT, 1.25 - SHIFT, 2.5 - SHIFT
                    p[3 + a] = sgn
                    p[6], p[7] = tmin, (INF if k != 2 else 1.5)
                    out.append(p)
    return np.ascontiguousarray(out, np.float32)


def test_open_box_against_its_analytic_rule_and_rooms_with_points_on_the_walls(orc):
    dirs = _dirs()
    box, pts = ee.open_box(), ee.open_box_points()
    segs = ee.exposure_segments(pts, dirs)
    want, excluded = ee.open_box_rule(segs)
    assert excluded.sum() <= 0.01 * segs.shape[0]
    lattice, wall_pts = rooms(), _rooms_points()
    for mm in (0, 1):
        for edges in (False, True):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(box)) if edges else g.UploadScene(box))
            answers = []
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                masks, _, _ = _same_as_occluded(g, pts, dirs, label="open box mm=%d edges=%d accel=%d" % (mm, edges, accel))
                got = ee.unpack_masks(masks).reshape(-1)
                wrong = (got != want) & ~excluded
                assert not wrong.any(), (mm, edges, accel, segs[wrong][:5])
                answers.append(masks)
            # the slack sweep's x0: bare boxes keep the masks of this scene
            g.DebugQueryAccelSlack(0)
            assert np.array_equal(g.Exposure(pts, dirs), answers[1])
            g.DebugQueryAccelSlack(1000)
            assert np.array_equal(g.Exposure(pts, dirs), answers[1]) and np.array_equal(answers[0], answers[1])
            assert (g.UploadSceneEdges(edge_rows(lattice)) if edges else g.UploadScene(lattice))
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                masks, _, occ = _same_as_occluded(g, wall_pts, dirs, label="rooms mm=%d edges=%d accel=%d" % (mm, edges, accel))
                assert occ.any() and (~occ).any()
            g.close()


def test_device_rays_equal_the_numpy_restatement_byte_for_byte():
    normals = np.concatenate([ee.unit_normals(2000, seed=1), ee.special_normals()])
    rng = np.random.default_rng(2)
    pts = np.zeros((normals.shape[0], 8), np.float32)
    pts[:, :3] = rng.normal(0.0, 3.0, (normals.shape[0], 3))
    pts[:, 3:6] = normals
    pts[:, 6:] = rng.uniform(-1.0, 5.0, (normals.shape[0], 2))
    table = rng.normal(0.0, 1.0, (64, 4)).astype(np.float32)
    g = _tracer()
    for k in (1, 63, 64):
        for world in (False, True):
            got = g.DebugExposureRays(pts, table[:k], world=world).reshape(-1, 8)
            want = ee.exposure_segments(pts, table[:k], world=world)
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), (k, world, np.argwhere(~same)[:5], got[~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])
    g.close()


def test_world_mode_with_nan_normals_equals_local_mode_with_rotated_directions():
    rows = adversarial_scene(300, seed=9)
    normal = ee.unit_normals(1, seed=4)[0]
    pts = _scene_points(rows, 130, seed=12)
    pts[:, 3:6] = normal
    dirs = _dirs()
    rotated = ee.as_dirs4(ee.exposure_segments(pts[:1], dirs)[:, 3:6])    # the fp32 directions the local mode traces
    poisoned = pts.copy()
    poisoned[:, 3:6] = NAN
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        local, _, occ = _same_as_occluded(g, pts, dirs)
        assert occ.any() and (~occ).any()
        assert np.array_equal(g.Exposure(poisoned, rotated, world=True), local)
        assert np.array_equal(g.Exposure(pts, rotated, world=True), local)
    g.close()


def test_per_point_intervals(orc):
    box = ee.open_box()
    dirs = _dirs()
    base = ee.open_box_points()[20:28]                                    # inside the box
    segs = ee.exposure_segments(base, dirs).reshape(8, 64, 8)
    table = hit_table(orc, segs.reshape(-1, 8), box, None, orc.FMA)
    hit, t = table[0].reshape(8, 64, -1), table[1].reshape(8, 64, -1)
    pts, closed_bit = [], []
    for i in range(8):                                                    # a t the oracle lists for one direction of the point
        j = int(np.nonzero(hit[i].any(axis=1))[0][i])
        ts = t[i, j][hit[i, j]].max()
        up, down = np.nextafter(ts, INF), np.nextafter(ts, -INF)
        for lo, hi, closes in ((ts, ts, True), (up, up, None), (down, down, None), (down, up, True), (ts, INF, True), (-INF, ts, True),
                               (NAN, INF, False), (-INF, NAN, False), (NAN, NAN, False), (up, down, False), (INF, -INF, False),
                               (-INF, INF, True), (INF, INF, False), (-INF, -INF, False), (1.0, 0.5, False)):
            p = base[i].copy()
            p[6], p[7] = lo, hi
            pts.append(p)
            closed_bit.append((j, closes))
    pts = np.ascontiguousarray(pts, np.float32)
    exp = ~expected_occluded(orc, ee.exposure_segments(pts, dirs), box, None, orc.FMA).reshape(-1, 64)
    g = _tracer()
    assert g.UploadScene(box)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        masks, _, _ = _same_as_occluded(g, pts, dirs, label="intervals accel=%d" % accel)
        if not accel:
            assert np.array_equal(masks, ee.pack_masks(exp))              # the scan is exact
        for m, p, (j, closes) in zip(masks, pts, closed_bit):
            if closes is not None:
                assert bool((m >> np.uint64(j)) & np.uint64(1)) == (not closes), (p, j, closes, hex(int(m)))
            if np.isnan(p[6:]).any() or p[6] > p[7]:
                assert m == ALL64                                        # a NaN bound or tmin > tmax: every bit set
        for k in (1, 63):
            sub = g.Exposure(pts, dirs[:k])
            assert np.array_equal(sub, masks & _low(k))
    g.close()


def test_argument_rules_no_scene_spheres_only_and_non_finite_normals():
    import torch
    import raytracertest_amd as R
    L = R.api.load_library()
    dirs = _dirs()
    down = np.array([[0, 0, 0, 0, 0, -1, 0, INF]] * 70, np.float32)       # normal -z: the hemisphere looks at the spheres
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        assert (g.Exposure(down, dirs) == ALL64).all()                    # no scene: every direction is open
        assert (g.Exposure(down, dirs[:5]) == np.uint64(31)).all()
        assert g.Exposure(np.zeros((0, 8), np.float32), dirs).shape == (0,)
        g.UploadSpheres(np.array([[0.0, 0.0, -3.0, 2.9]], np.float32))    # spheres alone are enough
        masks, _, occ = _same_as_occluded(g, down, dirs)
        assert occ.any() and (masks != ALL64).all()
        masks6 = g.Exposure(down[:, :6], dirs, tmin=0.0, tmax=np.inf)     # (n, 6) points with scalar bounds
        assert np.array_equal(masks6, masks)
        assert (g.Exposure(down[:, :6], dirs, tmin=100.0, tmax=200.0) == ALL64).all()
        bad = down.copy()                                                 # a non-finite normal: NaN directions never occlude
        bad[::2, 3] = NAN
        bad[1::4, 5] = INF
        got, _, _ = _same_as_occluded(g, bad, dirs)
        assert (got[::2] == ALL64).all() and np.array_equal(got[3::4], masks[3::4])
        p, d = down.ctypes.data, dirs.ctypes.data
        out = np.full(70, 5, np.uint64)
        for n_dirs in (0, 65):
            assert L.rt_tracer_exposure(g._h, p, 70, d, n_dirs, 0, out.ctypes.data) == 1 and "n_dirs" in g.LastError()
            assert L.rt_tracer_exposure(g._h, p, 0, d, n_dirs, 0, out.ctypes.data) == 1          # checked whatever n is
        assert L.rt_tracer_exposure(g._h, p, 70, d, 64, 2, out.ctypes.data) == 1 and "flags" in g.LastError()
        assert L.rt_tracer_exposure(g._h, None, 70, d, 64, 0, out.ctypes.data) == 1
        assert L.rt_tracer_exposure(g._h, p, 70, None, 64, 0, out.ctypes.data) == 1
        assert L.rt_tracer_exposure(g._h, p, 70, d, 64, 0, None) == 1
        assert L.rt_tracer_exposure(g._h, None, 0, None, 64, 0, None) == 0                       # n = 0 is a no-op
        assert (out == 5).all()
        for who in (g.Exposure,):
            for bad_dirs in (dirs[:0], np.zeros((65, 4), np.float32), dirs[:, :2]):
                with pytest.raises(ValueError):
                    who(down, bad_dirs)
            with pytest.raises(ValueError):
                who(down[:, :7], dirs)
            with pytest.raises(ValueError):
                who(down, dirs, tmin=0.0)                                 # (n, 8) points carry their own bounds
        # misaligned device pointers
        tp = torch.from_numpy(np.concatenate([down.reshape(-1), np.zeros(8, np.float32)])).to("cuda:0")
        td = torch.from_numpy(np.concatenate([dirs.reshape(-1), np.zeros(8, np.float32)])).to("cuda:0")
        tm = torch.zeros(72, dtype=torch.int64, device="cuda:0")
        ok = (tp.data_ptr(), td.data_ptr(), tm.data_ptr())
        assert L.rt_tracer_exposure_device(g._h, ok[0], 70, ok[1], 64, 0, ok[2], None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(tm[:70].cpu().numpy().view(np.uint64), masks)
        for off in ((4, 0, 0), (0, 8, 0), (0, 0, 4)):
            assert L.rt_tracer_exposure_device(g._h, ok[0] + off[0], 70, ok[1] + off[1], 64, 0, ok[2] + off[2], None) == 1
            assert "aligned" in g.LastError()
        g.close()


def test_torch_tensors_on_a_side_stream_give_the_same_bits():
    import torch
    rows = adversarial_scene(300, seed=9)
    pts = _scene_points(rows, 1000, seed=10)
    dirs = _dirs()
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    tp, td = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(dirs).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        host = g.Exposure(pts, dirs)
        assert (host != ALL64).any() and (host != 0).any()
        out = g.Exposure(tp, td)
        assert out.dtype == torch.int64 and out.shape == (1000,) and out.device == tp.device
        assert np.array_equal(out.cpu().numpy().view(np.uint64), host)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):                                        # on the caller's current stream
            out2 = g.Exposure(tp, td[:, :3].contiguous(), world=False)
            out3 = g.Exposure(tp[:, :6].contiguous(), td, tmin=1e-3, tmax=4.0)
        s.synchronize()
        assert torch.equal(out2, out)
        six = pts.copy()
        six[:, 6:] = [1e-3, 4.0]
        assert np.array_equal(out3.cpu().numpy().view(np.uint64), g.Exposure(six, dirs))
        assert np.array_equal(g.Exposure(tp, dirs[:7]).cpu().numpy().view(np.uint64), host & _low(7))   # numpy directions are uploaded
        assert g.Exposure(tp[:0], td).shape == (0,)
    for bad in (tp.cpu(), tp.double(), tp[:, :7].contiguous(), tp.t(), tp.reshape(-1)):
        with pytest.raises(ValueError):
            g.Exposure(bad, td)
    for bad in (td.cpu(), td.double(), td[:0], td.t()):
        with pytest.raises(ValueError):
            g.Exposure(tp, bad)
    g.close()


def test_exposure_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    pts = _scene_points(rows, 512, seed=7)
    pts[:, 6:] = [1e-3, INF]
    dirs = _dirs()

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Exposure(pts, dirs)
        got = []
        g.Trace(12, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                            # both modes; the tree is built while the Trace runs
            got.append(g.Exposure(pts, dirs))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        if calls:
            _same_as_occluded(g, pts, dirs, label="after the trace, BVH")
        g.close()
        return idle, got, out

    idle, got, out = run(20)
    assert (idle != ALL64).any() and (idle != 0).any()
    assert len(got) == 20 and all(np.array_equal(x, idle) for x in got[0::2])
    # BVH: never an occluder the scan does not see (an open bit of the scan stays open), and few differences
    assert all(not (idle & ~x).any() and (ee.popcount(x ^ idle).sum() <= 0.01 * 64 * pts.shape[0]) for x in got[1::2])
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_band_handle_and_reuploaded_scenes():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    rng = np.random.default_rng(3)
    pts = np.zeros((300, 8), np.float32)
    pts[:, :3] = rng.uniform(-0.9, 0.9, (300, 3))
    pts[:, 2] -= 2.0
    pts[:, 3:6] = ee.unit_normals(300, seed=5)
    pts[:, 6:] = [1e-3, INF]
    dirs = _dirs()
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    exp = one.Exposure(pts, dirs)
    assert (exp != ALL64).any() and (exp != 0).any()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    assert np.array_equal(m.Exposure(pts, dirs), exp)
    m.SetQueryAcceleration(True)
    _same_as_occluded(m, pts, dirs, label="two bands, BVH")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()
    # a re-uploaded scene: rebuilt, and refitted under ACCEL_REFIT
    moved = rows.copy()
    moved[:, :3] = moved[:, :3] * np.float32(1.125) + np.float32([0.05, -0.03, 0.02])
    one.SetQueryAcceleration(True)
    for policy in (R.api.ACCEL_REBUILD, R.api.ACCEL_REFIT):
        one.SetQueryAccelUpdate(policy)
        for scene in (rows, moved, rows):
            assert one.UploadScene(scene)
            assert one.QueryAccelInfo()["valid"] == 0
            _same_as_occluded(one, pts, dirs, label="re-upload policy=%d" % policy)
            assert one.QueryAccelInfo()["valid"] == 1
        info = one.QueryAccelUpdateInfo()
        assert (info["refits"] >= 1) == (policy == R.api.ACCEL_REFIT), info
    one.SetQueryAcceleration(False)
    assert one.UploadScene(rows)
    assert np.array_equal(one.Exposure(pts, dirs), exp)
    one.close()


def test_ambient_occlusion_is_the_popcount_of_two_exposure_calls():
    from raytracertest_amd import api
    box = ee.open_box()
    p = ee.open_box_points()
    g = _tracer()
    assert g.UploadScene(box)
    rng = np.random.default_rng(8)
    normals = p[:, 3:6].astype(np.float64) * rng.uniform(0.5, 3.0, (40, 1))           # not unit: the helper normalises in float64
    unit = (normals / np.sqrt((normals * normals).sum(axis=1))[:, None]).astype(np.float32)
    dirs = api.hemisphere_directions(100)
    pts = p.copy()
    pts[:, 3:6] = unit
    pts[:, 6:] = [np.float32(1e-3), INF]
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        ao = g.AmbientOcclusion(p[:, :3], normals, samples=100)
        assert ao.dtype == np.float32 and ao.shape == (40,)
        a, b = g.Exposure(pts, dirs[:64]), g.Exposure(pts, dirs[64:])
        assert not (b >> np.uint64(36)).any()
        assert np.array_equal(ao, ((ee.popcount(a) + ee.popcount(b)) / np.float64(100)).astype(np.float32))
        assert 0.0 <= ao.min() < ao.max() < 1.0
        near = g.AmbientOcclusion(p[:, :3], normals, samples=64, max_distance=1e-2, bias=1e-3)
        assert (near[20:] == 1.0).all()                                   # nothing within 1e-2 of the points inside
    g.close()
