"""The host builder of the ray queries' BVH (rt_dbg_bvh_build; needs no device): structure of the dumped tree on ordinary,
degenerate and non-finite scenes, the depth bound the traversal stack is sized from, determinism, and a numpy restatement of
the traversal's box test walking the dumped tree against the oracle's scan."""
import numpy as np
import pytest

from query_accel_expect import check_against_scan, check_tree, walk_tree
from query_expect import adversarial_rays, adversarial_scene, edge_rows, expected_hits, tri_rows as _rows


def _slivers(n, seed):
    """n needle triangles in the plane z = -5: long in x, 1e-4 high."""
    rng = np.random.default_rng(seed)
    a = np.c_[rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.full(n, -5.0)]
    return _rows(np.stack([a, a + [2.0, 0.0, 0.0], a + [1.0, 1e-4, 0.0]], 1))


def _with_bad_vertices(rows):
    r = rows.copy().reshape(-1, 3, 4)
    r[3, 1, 0] = np.nan
    r[10, 2, 2] = np.inf
    r[11, 0, 1] = -np.inf
    r[20, 0, :3] = 3.0e38                       # finite vertices whose edges overflow
    r[20, 1, :3] = -3.0e38
    return r.reshape(-1, 4)


def _scenes():
    from raytracertest_amd import scenes
    one = _rows([[[0, 0, -5], [1, 0, -5], [0, 1, -5]]])
    return {
        "cornell32": scenes.cornell32(),
        "random10k": scenes.random_triangles(10000, 12345),
        "random200k": scenes.random_triangles(200000, 77),
        "adversarial300": adversarial_scene(300, 11),
        "bad_vertices": _with_bad_vertices(adversarial_scene(37, 3)),
        "one": one,
        "copies10k": np.tile(one, (10000, 1)),
        "slivers": _slivers(2000, 5),
    }


@pytest.mark.parametrize("name", ["cornell32", "random10k", "random200k", "adversarial300", "bad_vertices", "one", "copies10k", "slivers"])
def test_tree_structure_depth_and_determinism(name):
    from raytracertest_amd import api
    rows = _scenes()[name]
    for edges in (False, True):
        up = edge_rows(rows) if edges else rows
        nodes, recs, info = api.bvh_build(up, edges)
        depth = check_tree(nodes, recs, info, up, edges)
        n = up.shape[0] // 3
        assert info["depth_bound"] == 16 and 3 * info["depth_bound"] * 64 * 8 <= 65536     # the stack of one wave fits in LDS
        if name == "bad_vertices":
            assert info["always_tested"] == 4 if not edges else info["always_tested"] >= 3
        elif name != "bad_vertices":
            assert info["always_tested"] == 0
        if name == "copies10k":                        # coincident centres: median splits, a balanced tree
            assert depth == 6                          # 2500 leaves under 4-wide nodes: ceil(log4(2500))
        if n >= 10000 and name != "copies10k":
            assert depth <= 2 + int(np.ceil(np.log(n / 4) / np.log(4))) + 3
        n2, r2, i2 = api.bvh_build(up, edges)
        assert n2.tobytes() == nodes.tobytes() and r2.tobytes() == recs.tobytes()
        assert {k: v for k, v in i2.items() if k != "build_us"} == {k: v for k, v in info.items() if k != "build_us"}


def test_builder_rejects_bad_arguments():
    from raytracertest_amd import api
    L = api.load_library()
    import ctypes as C
    info = (C.c_uint64 * 8)()
    rows = _scenes()["one"]
    assert L.rt_dbg_bvh_build(None, 3, 0, None, 0, None, 0, info) == 1
    assert L.rt_dbg_bvh_build(rows.ctypes.data, 4, 0, None, 0, None, 0, info) == 1
    assert L.rt_dbg_bvh_build(rows.ctypes.data, 3, 0, None, 0, None, 0, None) == 1
    assert L.rt_dbg_bvh_build(rows.ctypes.data, 3, 0, None, 0, None, 0, info) == 0 and info[2] == 1 and info[3] == 1
    buf = np.zeros(64, np.uint8)
    assert L.rt_dbg_bvh_build(rows.ctypes.data, 3, 0, buf.ctypes.data, 64, buf.ctypes.data, 48, info) != 0   # too small


@pytest.mark.parametrize("nearest", [False, True])
def test_restated_box_test_agrees_with_the_oracle_scan(orc, nearest):
    from raytracertest_amd import api, scenes
    rows = adversarial_scene(300, 11)
    rays = adversarial_rays(rows, 1500, 5)
    nodes, recs, info = api.bvh_build(rows)
    got, tests = walk_tree(orc, nodes, recs, info, rays, rows, nearest=nearest)
    exp = expected_hits(orc, rays, rows, nearest=nearest)
    assert check_against_scan(got, exp, rays, rows, label="adversarial300 nearest=%d" % nearest) == 0
    finite = np.isfinite(rays).all(axis=1) & (rays[:, 3:] != 0).any(axis=1)
    print("triangle tests per finite ray: %.1f of 300" % ((tests - 300.0 * (~finite).sum()) / finite.sum()))
    assert tests < 0.5 * 300 * rays.shape[0]                       # it prunes
    rows = scenes.cornell32()
    rng = np.random.default_rng(2)
    org = rng.uniform(-0.9, 0.9, (1500, 3)).astype(np.float32)
    org[:, 2] -= 2.0
    rays = np.ascontiguousarray(np.c_[org, rng.normal(0, 1, (1500, 3))], np.float32)
    rays[::7, 3] = 0.0                                             # axis-parallel components
    rays[::11, 4:] = 0.0
    nodes, recs, info = api.bvh_build(rows)
    got, _ = walk_tree(orc, nodes, recs, info, rays, rows, nearest=nearest)
    assert check_against_scan(got, expected_hits(orc, rays, rows, nearest=nearest), rays, rows, label="cornell32 nearest=%d" % nearest) == 0


def test_bare_boxes_lose_hits(orc):
    """The comparison has teeth: with rho = 0 and every box shrunk to its middle 40 %, the restated walk misses hits."""
    from raytracertest_amd import api
    rows = adversarial_scene(300, 11)
    rays = adversarial_rays(rows, 1500, 5)
    nodes, recs, info = api.bvh_build(rows)
    shrunk = nodes.copy()
    with np.errstate(invalid="ignore"):                           # (the boxes of absent children are +inf, -inf)
        w = shrunk["hi"] - shrunk["lo"]
        shrunk["lo"] += np.float32(0.3) * w
        shrunk["hi"] -= np.float32(0.3) * w
    got, _ = walk_tree(orc, shrunk, recs, info, rays, rows, rho=np.float32(0))
    exp = expected_hits(orc, rays, rows)
    assert (got["prim"] != exp["prim"]).sum() > 10
