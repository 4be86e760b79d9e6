"""The exposure query without a device: the library's frame (rt_dbg_exposure_rays with no tracer: the kernels' function on the
host) against its numpy restatement byte for byte; the frame's orthonormality; the restated pipeline -- exposure_segments, then the
oracle's OR over every primitive -- on the open box against its analytic rule, with teeth; and hemisphere_directions."""
import numpy as np

import exposure_expect as ee
from occluded_expect import expected_occluded


def _bytes_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _points(normals, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((normals.shape[0], 8), np.float32)
    p[:, :3] = rng.normal(0.0, 3.0, (normals.shape[0], 3))
    p[:, 3:6] = normals
    p[:, 6] = rng.uniform(-1.0, 1.0, normals.shape[0])
    p[:, 7] = p[:, 6] + rng.uniform(0.0, 5.0, normals.shape[0]).astype(np.float32)
    return p


def test_library_frame_equals_the_numpy_restatement_byte_for_byte():
    from raytracertest_amd import api
    normals = np.concatenate([ee.unit_normals(2000, seed=1), ee.special_normals()])
    pts = _points(normals, seed=2)
    table = np.random.default_rng(3).normal(0.0, 1.0, (64, 4)).astype(np.float32)   # w is garbage: it must be ignored
    table[:8, :3] = api.hemisphere_directions(8)
    for k in (1, 63, 64):
        for world in (False, True):
            got = api.exposure_rays(pts, table[:k], world=world)
            assert got.shape == (pts.shape[0], k, 8)
            want = ee.exposure_segments(pts, table[:k], world=world)
            assert _bytes_equal(got.reshape(-1, 8), want), (k, world)
            other = table[:k].copy()
            other[:, 3] = 7.0
            assert _bytes_equal(api.exposure_rays(pts, other, world=world), got)        # w changes no byte
    # the special rows are what the header says: z = -0 takes s = -1, the zero vector a finite frame, a NaN normal NaN directions
    local = api.exposure_rays(pts[2000:], table[:8])
    assert np.isfinite(local[:8]).all() and np.isnan(local[8, :, 3:6]).all() and np.isfinite(local[8, :, [0, 1, 2, 6, 7]]).all()
    neg0 = ee.frame(np.float32([[0.6, 0.8, -0.0]]))
    pos0 = ee.frame(np.float32([[0.6, 0.8, 0.0]]))
    assert not np.array_equal(neg0[0], pos0[0])                                     # s = -1 and s = +1 are different frames
    # world mode: NaNs in the normal slots change no byte
    poisoned = pts.copy()
    poisoned[:, 3:6] = np.nan
    assert _bytes_equal(api.exposure_rays(poisoned, table, world=True), api.exposure_rays(pts, table, world=True))
    assert _bytes_equal(api.exposure_rays(poisoned, table, world=True)[:, :, 3:6],
                        np.broadcast_to(table[None, :, :3], (pts.shape[0], 64, 3)))


def test_frame_is_orthonormal_and_right_handed():
    from raytracertest_amd import api
    n32 = ee.unit_normals(200007, seed=11)
    pts = np.zeros((n32.shape[0], 8), np.float32)
    pts[:, 3:6] = n32
    rays = api.exposure_rays(pts, np.float32([[1, 0, 0], [0, 1, 0]]))             # the library's own T and B: 1 * T + 0 * B + 0 * n
    T32, B32 = ee.frame(n32)
    assert np.array_equal(rays[:, 0, 3:6], T32) and np.array_equal(rays[:, 1, 3:6], B32)
    T, B = rays[:, 0, 3:6].astype(np.float64), rays[:, 1, 3:6].astype(np.float64)
    n = n32.astype(np.float64)
    dot = lambda a, b: (a * b).sum(axis=1)                                          # noqa: E731
    worst = max(np.abs(dot(T, T) - 1).max(), np.abs(dot(B, B) - 1).max(), np.abs(dot(T, B)).max(), np.abs(dot(T, n)).max(),
                np.abs(dot(B, n)).max())
    print("frame orthonormality: worst deviation %.3e over %d normals (bound 2^-21 = %.3e)" % (worst, n.shape[0], 2.0 ** -21))
    assert worst <= 2.0 ** -21
    assert (dot(np.cross(T, B), n) > 0.99).all()
    for special in ee.special_normals()[:7]:                                         # the axes and z = -0 as well
        Ts, Bs = (x.astype(np.float64)[0] for x in ee.frame(special[None, :]))
        ns = special.astype(np.float64)
        assert abs(Ts @ Ts - 1) <= 2.0 ** -21 and abs(Bs @ Bs - 1) <= 2.0 ** -21 and abs(Ts @ Bs) <= 2.0 ** -21
        assert abs(Ts @ ns) <= 2.0 ** -21 and abs(Bs @ ns) <= 2.0 ** -21 and np.cross(Ts, Bs) @ ns > 0.99


def test_restated_pipeline_on_the_open_box_agrees_with_the_analytic_rule(orc):
    from raytracertest_amd import api
    rows = ee.open_box()
    assert rows.shape == (60, 4)
    pts = ee.open_box_points()
    dirs = api.hemisphere_directions(64)
    segs = ee.exposure_segments(pts, dirs)
    want, excluded = ee.open_box_rule(segs)
    assert excluded.sum() <= 0.01 * segs.shape[0]
    for contract in (orc.FMA, orc.STRICT):
        got = ~expected_occluded(orc, segs, rows, None, contract)
        wrong = (got != want) & ~excluded
        print("open box, contract %d: %d excluded of %d, %d wrong, %.1f %% open" % (contract, excluded.sum(), segs.shape[0], wrong.sum(),
                                                                                 100.0 * got.mean()))
        assert not wrong.any(), segs[wrong][:5]
        assert 0.1 < got.mean() < 0.6
    masks = ee.pack_masks(want.reshape(40, 64))
    assert masks.dtype == np.uint64 and np.array_equal(ee.unpack_masks(masks), want.reshape(40, 64))
    assert np.array_equal(ee.popcount(masks), want.reshape(40, 64).sum(axis=1))
    # single-sided walls do not close the box: that is why it is double-sided
    single = ~expected_occluded(orc, segs, ee.open_box(double_sided=False), None, orc.FMA)
    print("single-sided walls: the rule fails on %d of %d rays" % (((single != want) & ~excluded).sum(), segs.shape[0]))
    assert ((single != want) & ~excluded).sum() > 100
    # teeth: a negated normal, or T and B exchanged, gives other masks than the analytic ones
    flipped = pts.copy()
    flipped[:, 3:6] = -flipped[:, 3:6]
    for bad in (ee.exposure_segments(flipped, dirs), ee.exposure_segments(pts, dirs, swap=True)):
        got = ~expected_occluded(orc, bad, rows, None, orc.FMA)
        assert not np.array_equal(ee.pack_masks(got.reshape(40, 64)), masks)


def test_hemisphere_directions():
    from raytracertest_amd import api
    for m in (64, 100):
        d = api.hemisphere_directions(m)
        assert d.shape == (m, 3) and d.dtype == np.float32
        d64 = d.astype(np.float64)
        assert np.abs(np.sqrt((d64 * d64).sum(axis=1)) - 1).max() <= 2.0 ** -23
        assert (d[:, 2] > 0).all()
        k = np.arange(m) + 0.5
        assert np.allclose(d64[:, 2], np.sqrt(1 - k / m), atol=1e-7)                 # cosine-weighted: z^2 uniform
        assert np.allclose(np.arctan2(d64[:, 1], d64[:, 0]), np.angle(np.exp(1j * k * np.pi * (3 - np.sqrt(5)))), atol=1e-5)
    whole = api.hemisphere_directions(128)
    k = np.arange(64) + 0.5                                                          # samples k < 64 of the 128 set, evaluated here
    r, phi = np.sqrt(k / 128), k * np.pi * (3 - np.sqrt(5))
    first = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - k / 128)], axis=1)
    assert whole[:64].shape == (64, 3) and np.abs(whole[:64].astype(np.float64) - first).max() <= 2.0 ** -24
    assert not np.array_equal(whole[:64], api.hemisphere_directions(64))             # a slice of a set is not the smaller set
    assert len({tuple(x) for x in whole}) == 128
    for bad in (0, -1, 2.5):
        try:
            api.hemisphere_directions(bad)
        except ValueError:
            continue
        raise AssertionError(bad)
