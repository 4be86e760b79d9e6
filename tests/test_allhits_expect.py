"""The test side of the all-hits query, checked without a device: the expected-answer helper against the closest-hit and the
any-hit helpers it must agree with, and the numpy restatement of the traversal walking trees dumped by rt_dbg_bvh_build against
the brute force, under the BVH contract; and the contract check's own teeth."""
import numpy as np
import pytest

from allhits_expect import (check_bvh_all_hits, exact_set, expected_all_hits, hit_table_uv, layered_scene, same_rows,
                            sets_from_table, walk_tree_all_hits)
from occluded_expect import expected_occluded, interval_families, with_interval
from query_accel_expect import populations
from query_expect import FLT_MAX, adversarial_rays, adversarial_scene, expected_hits, same_hits

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)
INF = np.float32(np.inf)
TINY = np.nextafter(np.float32(0), np.float32(1))                    # the smallest positive float


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("spheres", [False, True])
def test_helper_is_consistent_with_the_closest_hit_and_any_hit_helpers(orc, contract, spheres):
    rows = adversarial_scene(37, seed=37)
    rays = adversarial_rays(rows, 300, seed=38)
    sph = SPHERES if spheres else None
    table = hit_table_uv(orc, rays, rows, sph, contract)
    n_prims = table[0].shape[1]

    # the nearest hit in front of the origin is the first element over [TINY, FLT_MAX)
    near = expected_hits(orc, rays, rows, sph, contract, nearest=True)
    hits, counts = expected_all_hits(table, with_interval(rays, TINY, np.nextafter(FLT_MAX, np.float32(0))), 1)
    assert same_hits(hits[:, 0], near) and np.array_equal(counts > 0, near["prim"] >= 0) and (counts > 0).sum() > 100

    # the farthest hit above -FLT_MAX is the last t of the whole list, and its prim the lowest among the entries with that t
    far = expected_hits(orc, rays, rows, sph, contract, nearest=False)
    hits, counts = expected_all_hits(table, with_interval(rays, np.nextafter(-FLT_MAX, np.float32(0)), INF), n_prims)
    assert np.array_equal(counts > 0, far["prim"] >= 0)
    ties = 0
    for i in np.nonzero(counts)[0]:
        row = hits[i, :counts[i]]
        last = row[row["t"] == row["t"][-1]]
        ties += last.shape[0] > 1
        assert last["t"][0].tobytes() == far["t"][i].tobytes() or (last["t"][0] == 0 and far["t"][i] == 0)
        assert last["prim"].min() == last["prim"][0] == far["prim"][i]
        best = row[row["prim"] == far["prim"][i]]
        assert same_hits(best, far[i:i + 1])
    assert ties > 10 and counts.max() > 8                            # equal t, and rows longer than a short list

    # a ray is occluded exactly when its list is not empty; the order rule holds in every row
    pairs = 0
    for fam, segs in interval_families(rays, seed=3).items():
        hits, counts = expected_all_hits(table, segs, 16)
        assert np.array_equal(counts > 0, expected_occluded(orc, segs, rows, sph, contract, (table[0], table[1])))
        for i in np.nonzero(counts > 1)[0]:
            row = hits[i, :counts[i]]
            a, b = row[:-1], row[1:]
            assert ((a["t"] < b["t"]) | ((a["t"] == b["t"]) & (a["prim"] < b["prim"]))).all()
            pairs += int((a["t"] == b["t"]).sum())
        assert (hits["prim"][np.arange(16)[None, :] >= counts[:, None]] == -1).all()
    assert pairs > 50


def test_layered_scene_has_many_hits_per_ray(orc):
    rows = layered_scene(24, 8, 5)
    assert rows.shape == (3 * 3072, 4) and rows.dtype == np.float32
    assert np.array_equal(rows, layered_scene(24, 8, 5)) and not np.array_equal(rows, layered_scene(24, 8, 6))
    z = rows.reshape(-1, 3, 4)[:, :, 2]
    assert -8.0 < z.min() < -7.6 and -2.2 < z.max() < -1.8
    rays = populations(rows, 40, seed=21)["near"]
    table = hit_table_uv(orc, rays, rows)
    _, counts = expected_all_hits(table, interval_families(rays, seed=4)["any"], 3072)
    print("layered_scene(24, 8, 5): %.1f hits per ray, at most %d" % (counts.mean(), counts.max()))
    assert counts.mean() > 4 and counts.max() > 8


def _scene(name):
    from raytracertest_amd import scenes
    return scenes.cornell32() if name == "cornell32" else layered_scene(24, 8, 5)


@pytest.mark.parametrize("name", ["cornell32", "layered"])
def test_restated_walk_obeys_the_contract(orc, name):
    from raytracertest_amd import api
    rows = _scene(name)
    n_tris = rows.shape[0] // 3
    nodes, recs, info = api.bvh_build(rows)
    pops = populations(rows, 48, seed=21)
    for pop, rays in pops.items():
        rays = rays.copy()
        rays[::9, 3] = 0.0                                           # axis-parallel components, a zero direction, a NaN
        rays[5, 3:] = 0.0
        rays[6, 1] = np.nan
        table = hit_table_uv(orc, rays, rows, SPHERES[:1])
        for fam, segs in interval_families(rays, seed=4).items():
            E, W = sets_from_table(table, segs, rows)
            for max_hits in (1, 4, 16):
                exp = expected_all_hits(table, segs, max_hits)
                hits, counts, tests = walk_tree_all_hits(orc, nodes, recs, info, segs, rows, max_hits, SPHERES[:1])
                used = check_bvh_all_hits((hits, counts), exp, E, W, max_hits, every=True,
                                          label="%s %s %s" % (name, pop, fam))
                assert used == 0
                if n_tris >= 1000 and pop == "near" and max_hits == 1:   # it prunes (far origins inflate every box: pad ~ rho |o|)
                    assert tests < 0.25 * n_tris * segs.shape[0], (fam, tests)


def test_the_contract_check_has_teeth(orc):
    """With rho = 0 and every box shrunk to its middle 40 %, the restated walk loses well-conditioned hits and the check
    refuses; it also refuses two entries swapped, an invented hit, and a dropped well-conditioned hit with the next pulled in."""
    from raytracertest_amd import api
    rows = _scene("layered")
    nodes, recs, info = api.bvh_build(rows)
    shrunk = nodes.copy()
    with np.errstate(invalid="ignore"):
        w = shrunk["hi"] - shrunk["lo"]
        shrunk["lo"] += np.float32(0.3) * w
        shrunk["hi"] -= np.float32(0.3) * w
    rays = populations(rows, 48, seed=21)["near"]
    segs = interval_families(rays, seed=4)["any"]
    table = hit_table_uv(orc, rays, rows)
    E, W = sets_from_table(table, segs, rows)
    exp = expected_all_hits(table, segs, 4)
    hits, counts, _ = walk_tree_all_hits(orc, shrunk, recs, info, segs, rows, 4, rho=np.float32(0))
    assert not same_rows((hits, counts), exp)
    with pytest.raises(AssertionError, match="well-conditioned hit was lost"):
        check_bvh_all_hits((hits, counts), exp, E, W, 4)
    assert check_bvh_all_hits(exp, exp, E, W, 4, every=True) == 0

    i = int(np.nonzero(exp[1] == 4)[0][0])                           # a ray with a full row of well-conditioned hits
    assert W(i)[:5].all() and exact_set(table, segs, i).shape[0] > 5

    def broken(edit):
        h, c = exp[0].copy(), exp[1].copy()
        edit(h, c)
        return h, c

    def swap(h, c):
        h[i, [1, 2]] = h[i, [2, 1]]

    def invent(h, c):
        h[i, 3]["prim"] = int(np.nonzero(~table[0][i])[0][0])

    def wrong_bits(h, c):
        h[i, 0]["u"] = np.nextafter(h[i, 0]["u"], INF)

    def drop(h, c):
        h[i, 1:] = exact_set(table, segs, i)[2:5]

    def shorten(h, c):
        h[i, 3] = (0, 0, 0, -1)
        c[i] = 3

    for edit, msg in ((swap, "not strictly ascending"), (invent, "not in the exact set"), (wrong_bits, "bits differ"),
                      (drop, "well-conditioned hit was lost"), (shorten, "well-conditioned hit was lost")):
        with pytest.raises(AssertionError, match=msg):
            check_bvh_all_hits(broken(edit), exp, E, W, 4)
    with pytest.raises(AssertionError):                              # the cap counts the rays that differ
        check_bvh_all_hits(broken(drop), exp, E, W, 4, cap=1e-3)
