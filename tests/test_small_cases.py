"""The small-scene option matrix (tests/small_cases.py) stays what tests/test_gpu_small_options.py claims it is, without a
device: a valid all-pairs cover with nothing infeasible beyond what the code refuses or makes vacuous, a hot sub-table that
covers its own pairs, every anchor; frames that give tile_corner_bound's verdict the case's builder is named after, with a
margin; frames and scenes with certain-winner tiles, empty tiles and contested tiles; and teeth -- the oracle with one option of
a case changed renders another frame."""
import numpy as np
import pytest

import small_cases as sc

IDS = [c["name"] for c in sc.CASES]


def test_cases_cover_every_pair_of_axis_values():
    covered = set()
    for c in sc.CASES:
        for axis, values in sc.AXES.items():
            assert c[axis] in values or (axis == "builder" and c[axis] is None and c["kernel"] == "scan"), (c["name"], axis, c[axis])
        assert (c["builder"] is None) == (c["kernel"] == "scan"), c["name"]
        assert not any(p in sc.pairs_of(c) for p in sc.INFEASIBLE), c["name"]
        covered |= sc.pairs_of(c)
    missing = sc.required_pairs() - covered
    assert not missing, sorted(tuple(sorted(p, key=str)) for p in missing)
    assert len(set(IDS)) == len(sc.CASES) <= 64


def test_infeasible_holds_what_the_code_rules_out_and_nothing_else():
    want = {frozenset({("kernel", "unfiltered"), ("iters", "fused")}), frozenset({("kernel", "scan"), ("iters", "fused")}),
            frozenset({("kernel", "scan"), ("shape", "interleaved")})}
    want |= {frozenset({("kernel", "scan"), ("builder", b)}) for b in ("pair", "region", "tile32", "tile64")}
    for w in ("per_pixel", "no_owe", "traced"):
        want.add(frozenset({("winners", w), ("hit", "near")}))
        want |= {frozenset({("winners", w), ("extras", e)}) for e in ("spheres", "smooth", "spheres+smooth")}
    assert sc.INFEASIBLE == want and len(want) == 19
    assert sc.INFEASIBLE <= sc.all_pairs(sc.AXES)


def test_the_hot_sub_table_covers_its_pairs():
    hot = [c for c in sc.CASES if sc.hot(c)]
    for c in hot:
        assert (c["hit"], c["extras"], c["kernel"]) == ("far", "none", "filtered") and c["winners"] in ("table", "per_pixel", "no_owe")
    covered = set().union(*(sc.pairs_of(c, sc.HOT_AXES + ("math",)) for c in hot))
    missing = sc.hot_required_pairs() - covered
    assert not missing, sorted(tuple(sorted(p, key=str)) for p in missing)
    assert len(sc.hot_required_pairs()) == 4 * 5 + 4 * 3 + 4 * 4 + 4 * 2 + 5 * 3 + 5 * 4 + 5 * 2 + 3 * 4 + 3 * 2 + 4 * 2 + 2 * 4
    assert {c["winners"] for c in hot} == {"table", "per_pixel", "no_owe"}


def test_every_anchor_is_in_the_table():
    for what, holds in sc.ANCHORS.items():
        assert any(holds(c) for c in sc.CASES), "anchor missing: " + what
    by_name = {c["name"]: c for c in sc.CASES}
    assert all(sc.hot(by_name[n]) and by_name[n]["winners"] == "table" for n in sc.HOT_ANCHORS)


def test_triangle_counts_sit_on_both_sides_of_the_builders_and_of_pick_k():
    for c in sc.CASES:
        if c["builder"] is not None:
            assert c["n_tris"] in sc.N_TRIS[c["builder"]], c["name"]
        assert c["iters"] in ("one", "steps") or sc.iterations(c) > 1, c["name"]
        assert c["iters"] != "steps" or sc.n_steps(c) >= 3, c["name"]
        assert c["iters"] != "fused" or sc.iterations(c) * c["spp"] <= 64, c["name"]      # rt_tracer.hpp: fused_iterations
    for b, counts in sc.N_TRIS.items():
        assert {c["n_tris"] for c in sc.CASES if c["builder"] == b} == set(counts), b
    assert {sc.n_steps(c) for c in sc.CASES if c["iters"] == "steps"} >= {3, 5}


def test_launch_figures_of_the_anchors_against_literals():
    """samples_in_flight() restates pick_k, lds_bytes() trace_lds_bytes: 4 x bin_list x 40 with bin_list = ceil32(n) >= 32, or
    min(n, 1024) x 36 for the scan"""
    by_name = {c["name"]: c for c in sc.CASES}
    want = {"a1_bench_pair": (2, 5120), "a2_bench_region_n129": (4, 25600), "a3_strict_tile64_interleaved_fused_spp7": (2, 20480),
            "a4_smooth_region_band_cadence": (2, 40960), "a5_spheres_smooth_near_tile32_ragged": (1, 5120),
            "forced_k1_region_spp3_steps": (1, 40960), "forced_k4_tile32_spp7": (4, 5120), "region_n128_spp7_steps5": (2, 20480),
            "h_pair_ragged_no_owe_fused_spp7": (2, 5120), "h_tile64_unsplit_no_owe_spp7_n129": (4, 25600),
            "h_region_ragged_no_owe_steps": (1, 10240), "scan_spheres_smooth_near_cadence": (4, 129 * 36),
            "scan_near_ragged_steps": (2, 5 * 36), "scan_per_pixel_ragged": (1, 256 * 36)}
    for name, (k, lds) in want.items():
        assert (sc.samples_in_flight(by_name[name]), sc.lds_bytes(by_name[name])) == (k, lds), name
    assert sc.owed_draws(by_name["a1_bench_pair"]) == 3 * 3 * 2 and sc.owed_draws(by_name["region_n128_spp7_steps5"]) == 3 * 7 * 4
    assert sc.owed_draws(by_name["h_pair_unsplit_no_owe_steps"]) == 0 and sc.owed_draws(by_name["traced_region_interleaved_steps"]) == 0
    assert sc.list_builds(by_name["a1_bench_pair"]) == 3 and sc.list_builds(by_name["region_n128_spp7_steps5"]) == 1


def test_frames_launch_as_named_and_give_the_builders_verdict_with_a_margin(orc):
    for (shape, side), f in sc.FRAMES.items():
        W, rows, full_h, r0 = f["W"], f["rows"], f["full_h"], f["row_begin"]
        assert W <= 256 and rows <= 160 and r0 + rows <= (full_h or rows), (shape, side)
        if shape == "unsplit":
            assert rows < 128 and sc.split_row(rows) == 0
        else:
            assert rows >= 128 and 0 < sc.split_row(rows) < rows and sc.split_row(rows) % 8 == 0
        if shape == "band":
            assert full_h > rows and r0 % 8 != 0
        else:
            assert full_h == 0 and r0 == 0
        if shape == "ragged":
            assert W % 32 != 0 and W % 8 != 0 and rows % 8 != 0
        cam = orc.camera(f["angles"], f["fov"], sc.FOCAL, sc.APERTURE)
        granted, a, ratio = sc.corner_bound(f, list(cam.M))
        assert abs(a - 14.0 * np.tan(np.radians(f["fov"] / 2.0)) / (full_h or rows)) < 1e-12 and abs(ratio - 1.0) < 1e-5, (shape, side)
        assert granted == (side == "region") and (a <= sc.A_REGION_MAX if granted else a >= sc.A_TILE_MIN), (shape, side, a)
        assert f["angles"][0] == 0.0                                     # no pitch: the middle row of the frame sees y = 0
    assert sc.FRAMES["interleaved", "region"] is sc.FRAMES["rows", "region"] and sc.FRAMES["interleaved", "tile"] is sc.FRAMES["rows", "tile"]
    for c in sc.CASES:
        f = sc.frame(c)
        granted, _, _ = sc.corner_bound(f, list(orc.camera(f["angles"], f["fov"], sc.FOCAL, sc.APERTURE).M))
        kind = (0 if c["n_tris"] <= 32 else 1) if granted else (2 if c["n_tris"] <= 32 else 3)      # rt_kernels.hip: launch_tile_lists
        assert sc.builder_kind(c) in (None, kind), c["name"]
        r, n = sc.teeth_rows(c)
        assert 0 <= r and r + n <= f["rows"], c["name"]
        assert sc.interleave(c) in ((None, 0, 1) if c["shape"] in ("band", "ragged") else (None,) if c["shape"] == "unsplit" else (0, 1)), c["name"]
    split = [c for c in sc.CASES if c["shape"] in ("band", "ragged")]
    assert {sc.interleave(c) for c in split} == {None, 0, 1}


@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.hot(c)], ids=[c["name"] for c in sc.CASES if sc.hot(c)])
def test_hot_frames_have_every_kind_of_tile(orc, case):
    """the oracle's probe of every tile (its pixels x 9 lens points): certain candidates, tiles whose rays hit nothing, tiles with
    rays of different winners"""
    kind, winner, met = sc.tile_kinds(orc, case)
    counts = [int((kind == k).sum()) for k in (sc.NOTHING, sc.CERTAIN, sc.MIXED)]
    print(case["name"], "nothing / certain / mixed:", counts)
    assert counts[1] >= 8 and counts[0] >= 4, (case["name"], counts)
    contested = sum(1 for ty, tx in zip(*np.nonzero(kind == sc.MIXED)) if met[ty, tx] >= 2)
    assert contested >= 8, (case["name"], contested)
    assert (met[kind == sc.NOTHING] == 0).all() and (winner[kind == sc.CERTAIN] >= 0).all() and (winner[kind != sc.CERTAIN] == -1).all()


@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_teeth_every_option_of_a_case_changes_the_oracles_frame(orc, case):
    r, n = sc.teeth_rows(case)
    one = dict(case, iters="one")                                       # (one launch shows it)
    ref = sc.oracle(orc, one, row0=r, rows=n).render.view(np.uint32)
    flips = {"math": dict(math="strict" if case["math"] == "fma" else "fma"),
             "hit": dict(hit="far" if case["hit"] == "near" else "near")}
    if "spheres" in case["extras"]:
        flips["spheres"] = dict(spheres=False)
    if "smooth" in case["extras"]:
        flips["smooth"] = dict(smooth=False)
    if case["n_tris"] > 32:
        flips["extras"] = dict(with_extras=False)
    for what, kw in flips.items():
        t = sc.oracle(orc, one, row0=r, rows=n, **kw)
        assert not np.array_equal(t.render.view(np.uint32), ref), "%s: the oracle renders the same frame with %s changed" % (case["name"], what)


def _frame_of(orc, case, hit, drop=None, spheres=None):
    """the whole band at 1 spp under a hit rule, without the extras of one kind / with these spheres"""
    f = sc.frame(case)
    rows, _ = sc.scene(case)
    if drop is not None:
        keep = np.ones(case["n_tris"], bool)
        keep[32:] = [sc.extra_kind(k) != drop for k in range(case["n_tris"] - 32)]
        rows = rows.reshape(-1, 3, 4)[keep].reshape(-1, 4)
    o = orc.OracleTracer(f["W"], f["full_h"] or f["rows"], f["angles"], f["fov"], sc.FOCAL, sc.APERTURE, seed=3, row0=f["row_begin"],
                         rows=f["rows"], nthreads=8, hit_mode=int(hit == "near"))
    assert o.upload_scene(rows)
    if spheres is not None:
        o.upload_spheres(spheres)
    o.trace(1, 1)
    return o.render.view(np.uint32).copy()


@pytest.mark.parametrize("key", sorted(sc.FRAMES), ids=["%s-%s" % k for k in sorted(sc.FRAMES)])
def test_extras_and_spheres_lie_where_the_scenes_promise(orc, key):
    """in every frame: the side extras show under both hit rules, those inside the room under nearest hit only, those behind
    the back wall under farthest hit only; the sphere behind the room wins under farthest hit, the one in front under nearest
    hit, and the one at the side lies in tiles that no triangle reaches"""
    shape, side = key
    case = dict(name="probe", math="fma", hit="far", extras="none", builder="region" if side == "region" else "tile64", shape=shape,
                n_tris=256, spp=1, iters="one", extra={})
    seen = {(hit, drop): not np.array_equal(_frame_of(orc, case, hit), _frame_of(orc, case, hit, drop))
            for hit in ("far", "near") for drop in ("side", "inside", "behind")}
    assert seen == {("far", "side"): True, ("near", "side"): True, ("far", "inside"): False, ("near", "inside"): True,
                    ("far", "behind"): True, ("near", "behind"): False}, seen
    # (the first extra alone -- all a scene of 33 triangles has -- is a side extra on the teeth rows)
    assert sc.extra_kind(0) == "side" and abs(sc.extras(1)[0, :, 1]).max() < 0.15
    none = np.zeros((0, 4), np.float32)
    for hit, i in (("far", 0), ("near", 1)):
        assert not np.array_equal(_frame_of(orc, case, hit, spheres=sc.SPHERES), _frame_of(orc, case, hit, spheres=np.delete(sc.SPHERES, i, 0))), (hit, i)
    kind, _, met = sc.tile_kinds(orc, case)
    lit = (_frame_of(orc, case, "far", spheres=sc.SPHERES[2:]) != _frame_of(orc, case, "far", spheres=none)).any(axis=2)
    ty, tx = np.nonzero(lit)
    assert ty.size >= 16, "the side sphere is not in the frame"
    assert (met[ty // 8, tx // 8] == 0).all(), "a triangle reaches a tile of the side sphere"
    assert sc.SPHERES[0, 2] + sc.SPHERES[0, 3] < -3.5 and sc.SPHERES[1, 2] - sc.SPHERES[1, 3] > -1.0


def test_the_smooth_cases_use_edge_scenes_with_normals_that_are_not_the_faces():
    from raytracertest_amd import meshes
    c = next(c for c in sc.CASES if c["extras"] == "smooth" and c["n_tris"] > 32)
    rows, edges = sc.scene(c, 11)
    assert edges and rows.shape == (3 * c["n_tris"], 4) and rows[:, 3].all()          # (.w: the packed vertex normals)
    e = rows.reshape(-1, 3, 4)
    face = np.cross(e[:, 1, :3], e[:, 2, :3])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    vn = meshes.vertex_normals(rows).reshape(-1, 3, 3)
    assert (np.abs(np.einsum("tvk,tk->tv", vn, face)) < 0.999).all(axis=1).sum() >= 0.9 * c["n_tris"]
    plain, edges = sc.scene(dict(c, extras="none"), 11)
    assert not edges and plain.shape == (3 * c["n_tris"], 4)
    five = sc.scene(dict(c, extras="none", n_tris=5))[0]                              # back wall, left wall, the tall box's front
    assert np.array_equal(five, plain.reshape(-1, 3, 4)[list(sc.FIVE)].reshape(-1, 4)) and np.array_equal(plain[:96], sc.scene(dict(c, extras="none", n_tris=32))[0])
