"""The test side of the visibility query, checked without a device: the expected-answer helper against the closest-hit helper
it must agree with, and the numpy restatement of the any-hit traversal walking trees dumped by rt_dbg_bvh_build against the
brute force, under the BVH contract."""
import numpy as np
import pytest

from occluded_expect import (check_bvh_occluded, expected_occluded, hit_table, in_interval_conditioning, interval_families,
                             walk_tree_occluded, with_interval)
from query_accel_expect import populations
from query_expect import FLT_MAX, adversarial_rays, adversarial_scene, expected_hits

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
INF = np.float32(np.inf)
TINY = np.nextafter(np.float32(0), np.float32(1))                    # the smallest positive float


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("spheres", [False, True])
def test_helper_is_consistent_with_the_closest_hit_helper(orc, contract, spheres):
    rows = adversarial_scene(37, seed=37)
    rays = adversarial_rays(rows, 300, seed=38)
    sph = SPHERES if spheres else None
    table = hit_table(orc, rays, rows, sph, contract)

    def occ(tmin, tmax, sel):
        return expected_occluded(orc, with_interval(rays[sel], tmin, tmax), rows, sph, contract, (table[0][sel], table[1][sel]))

    far = expected_hits(orc, rays, rows, sph, contract, nearest=False)
    win = far["prim"] >= 0
    assert win.any() and (~win).any()
    t = far["t"][win]
    assert not np.isnan(t).any() and (t < 0).any()                   # the reference rule keeps hits behind the origin
    assert occ(t, t, win).all()                                      # [t*, t*] occludes (t* = +inf of a sphere included)
    beyond = occ(np.nextafter(t, INF), INF, win)                     # nothing lies beyond the farthest hit
    assert not beyond[t < INF].any() and (t < INF).sum() > 100
    # no winner under the reference rule <=> no hit above the initial -FLT_MAX
    assert np.array_equal(occ(np.nextafter(-FLT_MAX, np.float32(0)), INF, slice(None)), win)

    near = expected_hits(orc, rays, rows, sph, contract, nearest=True)
    nwin = near["prim"] >= 0
    t = near["t"][nwin]
    assert nwin.any() and (t > 0).all()
    assert occ(t, t, nwin).all()
    assert not occ(TINY, np.nextafter(t, -INF), nwin).any()          # nothing in front of the nearest hit
    assert np.array_equal(occ(TINY, np.nextafter(FLT_MAX, np.float32(0)), slice(None)), nwin)

    # the interval's own rules
    every = slice(None)
    assert np.array_equal(occ(-INF, INF, every), (table[0] & ~np.isnan(table[1])).any(axis=1))   # any hit at all, but a NaN t
    assert not occ(np.nan, INF, every).any() and not occ(-INF, np.nan, every).any()
    assert not occ(np.float32(1.0), np.float32(0.5), every).any()    # tmin > tmax


def test_interval_families_and_conditioning(orc):
    rows = adversarial_scene(37, seed=37)
    rays = adversarial_rays(rows, 50, seed=2)
    fam = interval_families(rays, seed=3)
    assert list(fam) == ["unit", "forward", "any", "window"]
    for k, s in fam.items():
        assert s.dtype == np.float32 and s.shape == (rays.shape[0], 8) and np.array_equal(s[:, :6].view(np.uint32), rays.view(np.uint32))
    assert (fam["unit"][:, 6] == 0).all() and (fam["unit"][:, 7] == 1).all()
    assert (fam["forward"][:, 6] == np.float32(1e-3)).all() and (fam["forward"][:, 7] == INF).all()
    assert (fam["any"][:, 6] == -INF).all() and (fam["any"][:, 7] == INF).all()
    w = fam["window"]
    assert (w[:, 6] >= -1).all() and (w[:, 6] <= 1).all() and (w[:, 7] >= w[:, 6]).all() and (w[:, 7] - w[:, 6] <= 1.5001).all()
    # a ray straight at a triangle is a well-conditioned occluder; the same ray with an interval behind it has none
    tri = np.array([[0, 0, -10, 0], [1, 0, -10, 0], [0, 1, -10, 0]], np.float32)
    seg = np.array([[0.2, 0.2, 0, 0, 0, -1, 0, 20], [0.2, 0.2, 0, 0, 0, -1, 11, 20]], np.float32)
    assert expected_occluded(orc, seg, tri).tolist() == [True, False]
    assert in_interval_conditioning(orc, seg, tri).tolist() == [True, False]
    # a grazing ray (direction nearly in the plane) may be accepted, but it is not well conditioned
    graze = np.array([[-5, 0.2, -10 + 5e-4, 1, 0, -1e-4, -INF, INF]], np.float32)
    assert in_interval_conditioning(orc, graze, tri).tolist() == [False]
    assert in_interval_conditioning(orc, graze, tri[:0], np.array([[0, 0.2, -10, 1]], np.float32)).tolist() == [True]   # a sphere counts


def _scene(name):
    from raytracertest_amd import scenes
    return scenes.cornell32() if name == "cornell32" else scenes.random_triangles(2000, 5)


@pytest.mark.parametrize("name", ["cornell32", "random2000"])
def test_restated_any_hit_walk_obeys_the_contract(orc, name):
    from raytracertest_amd import api
    rows = _scene(name)
    n_tris = rows.shape[0] // 3
    nodes, recs, info = api.bvh_build(rows)
    pops = populations(rows, 64, seed=21)
    for pop, rays in pops.items():
        rays = rays.copy()
        rays[::9, 3] = 0.0                                           # axis-parallel components, a zero direction, a NaN
        rays[5, 3:] = 0.0
        rays[6, 1] = np.nan
        table = hit_table(orc, rays, rows, SPHERES[:1])
        for fam, segs in interval_families(rays, seed=4).items():
            exp = expected_occluded(orc, segs, rows, SPHERES[:1], table=table)
            got, tests = walk_tree_occluded(orc, nodes, recs, info, segs, rows, SPHERES[:1])
            used = check_bvh_occluded(got, exp, segs, rows, orc, SPHERES[:1], table=table, label="%s %s %s" % (name, pop, fam))
            assert used == 0
            if n_tris >= 1000 and pop == "near":                     # it prunes (far origins inflate every box: pad ~ rho |o|)
                assert tests < 0.25 * n_tris * segs.shape[0]
    rays = np.concatenate(list(pops.values()))
    both = expected_occluded(orc, interval_families(rays, seed=4)["forward"], rows)
    assert both.any() and (~both).any()


def test_the_contract_check_has_teeth(orc):
    """With rho = 0 and every box shrunk to its middle 40 %, the restated walk loses well-conditioned occluders, and an
    answer that invents an occluder is refused as well."""
    from raytracertest_amd import api
    rows = _scene("random2000")
    nodes, recs, info = api.bvh_build(rows)
    shrunk = nodes.copy()
    with np.errstate(invalid="ignore"):
        w = shrunk["hi"] - shrunk["lo"]
        shrunk["lo"] += np.float32(0.3) * w
        shrunk["hi"] -= np.float32(0.3) * w
    rays = populations(rows, 96, seed=21)["near"]
    segs = interval_families(rays, seed=4)["any"]
    table = hit_table(orc, rays, rows)
    exp = expected_occluded(orc, segs, rows, table=table)
    got, _ = walk_tree_occluded(orc, shrunk, recs, info, segs, rows, rho=np.float32(0))
    assert (exp & ~got).sum() > 3
    with pytest.raises(AssertionError, match="well-conditioned occluder was lost"):
        check_bvh_occluded(got, exp, segs, rows, orc, table=table)
    with pytest.raises(AssertionError, match="the scan does not"):
        check_bvh_occluded(np.ones_like(exp), exp, segs, rows, orc, table=table)
