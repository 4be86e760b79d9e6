"""The region query's test side, checked without a device: the restated fp32 rule agrees with an independent float64
separating-axis test, the restated traversal of a tree from rt_dbg_bvh_build equals brute force and tests a small share of the
scan's triangles, the walk with one thing broken (open comparisons; a rule without step 1) gives another answer, the cursor
enumerates every accepted set, the bad boxes accept nothing, and the populations reach the counts they are for."""
import numpy as np
import pytest

import lattice_cases as lc
import overlap_expect as oe

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def library_has_the_query():
    """The rule restated here is the one of the library under test: without rt_tracer_overlap there is nothing to restate."""
    from raytracertest_amd import api
    assert hasattr(api.load_library(), "rt_tracer_overlap") and hasattr(api.RayTracer, "Overlap")


@pytest.fixture(scope="module")
def random1100():
    from raytracertest_amd import api
    rows = oe.random_scene(1100, 21, span=3.0, edge=0.6)
    return rows, oe.random_boxes(rows, 300, 22, width=0.6), api.bvh_build(rows)


@pytest.fixture(scope="module")
def rooms():
    from raytracertest_amd import api
    rows = lc.rooms()
    boxes, tags = oe.touching_boxes(rows, range(0, rows.shape[0] // 3, 7))
    return rows, boxes, tags, api.bvh_build(rows)


@pytest.mark.parametrize("snap", [None, 0.25])
def test_the_fp32_rule_equals_the_float64_test(snap):
    """Measured here: 0 disagreements in 2 000 000 pairs (1000 triangles of edge ~0.2 in [-1, 1]^3, 2000 boxes up to 0.5 wide;
    6 003 pairs accepted), and 0 in the 2 000 000 pairs of the same inputs snapped to multiples of 1/4 (85 020 accepted, touching
    exact).  Nothing is left out; the largest disagreement margin is "none in 2 000 000 pairs" in both."""
    rows = oe.random_scene(1000, 11, snap=snap)
    boxes = oe.random_boxes(rows, 2000, 12, snap=snap)
    acc = oe.table(boxes, rows)
    overlap, margin, scale = oe.sat64(boxes, rows)
    differ = acc != overlap
    worst = (margin[differ] / (oe.EPS * scale[differ])).max() if differ.any() else None
    print("snap %r: %d pairs, %d accepted, %d disagree, largest disagreement margin: %s" %
          (snap, acc.size, acc.sum(), differ.sum(), "none in %d pairs" % acc.size if worst is None else "%.3f eps scale" % worst))
    assert acc.size == 2_000_000 and acc.sum() > 1000
    excused = differ & (margin < oe.K * oe.EPS * scale)
    assert (differ == excused).all()                                     # a disagreement needs a margin within rounding
    assert excused.sum() < 0.01 * acc.size
    assert not differ.any()                                              # the recorded measurement: nothing had to be left out


def test_the_walk_equals_brute_force_and_prunes_on_the_random_scene(random1100):
    """Measured: the walk tests 0.44 % of the scan's 300 x 1100 box-triangle pairs; the bound is four times that."""
    rows, boxes, (nodes, recs, info) = random1100
    for k in (0, 4, 16):
        prims, counts, tests = oe.walk_tree_overlap(nodes, recs, info, boxes, rows, k)
        assert oe.same((prims, counts), oe.expected(boxes, rows, k))
    share = tests / (boxes.shape[0] * 1100.0)
    print("triangle tests: %.4f of the scan's" % share)
    assert share < 0.02


def test_the_walk_equals_brute_force_on_the_lattice_where_touching_is_exact(rooms):
    rows, boxes, tags, (nodes, recs, info) = rooms
    acc = oe.table(boxes, rows)
    for i, (j, axis, touches) in enumerate(tags):                       # hi == tmin touches; one ulp below does not
        assert acc[i, j] == touches
    prims, counts, _ = oe.walk_tree_overlap(nodes, recs, info, boxes, rows, 16)
    assert oe.same((prims, counts), oe.expected(boxes, rows, 16))
    cells = oe.boxes_of(np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3) - lc.SHIFT,
                        np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3) - lc.SHIFT + 1.0)
    prims, counts, _ = oe.walk_tree_overlap(nodes, recs, info, cells, rows, 16)
    assert oe.same((prims, counts), oe.expected(cells, rows, 16))
    assert counts.min() >= 12                                            # a cell touches its own six quads at the least


def test_open_comparisons_in_the_walk_change_an_answer_on_the_touching_boxes(rooms):
    rows, boxes, tags, (nodes, recs, info) = rooms
    prims, counts, _ = oe.walk_tree_overlap(nodes, recs, info, boxes, rows, 16, closed=False)
    assert not oe.same((prims, counts), oe.expected(boxes, rows, 16))


def test_without_step_1_the_walk_differs_from_its_own_brute_force(random1100):
    """Step 1 is what makes the prune exact: a rule of steps 2-3 alone accepts triangles that only a box face separates, the
    tree skips them, and the walk loses them (measured: 234 accepted by brute force, 218 by the walk)."""
    rows, boxes, (nodes, recs, info) = random1100
    brute = oe.rows_of_table(oe.table(boxes, rows, box_step=False), 16)
    prims, counts, _ = oe.walk_tree_overlap(nodes, recs, info, boxes, rows, 16, box_step=False)
    print("accepted without step 1: %d by brute force, %d by the walk" % (brute[1].sum(), counts.sum()))
    assert not oe.same((prims, counts), brute)
    assert counts.sum() < brute[1].sum()


@pytest.mark.parametrize("max_hits", [1, 4, 16])
def test_chaining_the_cursor_reproduces_the_whole_accepted_set(max_hits):
    rows = oe.random_scene(37, 37)
    spheres = f32([[0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.5], [0.5, 0.5, 0.5, 0.25]])
    boxes = np.concatenate([oe.whole_box(rows, spheres), oe.random_boxes(rows, 20, 38, width=1.0)])
    acc = oe.table(boxes, rows, spheres=spheres)
    assert acc[0].all() and acc.shape[1] == 40
    got, rounds = oe.chain(lambda live, after: oe.rows_of_table(acc[live], max_hits, after), boxes.shape[0], max_hits)
    for g, want in zip(got, oe.accepted_sets(acc)):
        assert np.array_equal(g, want)
    assert rounds == -(-40 // max_hits)


def test_cursor_edges_on_a_table():
    acc = np.ones((3, 5), bool)
    prims, counts = oe.rows_of_table(acc, 4, after=[4, oe.NONE, 7])
    assert counts.tolist() == [0, 5, 0] and prims[1].tolist() == [0, 1, 2, 3] and (prims[[0, 2]] == oe.NONE).all()


def test_bad_boxes_accept_nothing_and_nan_pads_change_nothing():
    rows = oe.random_scene(37, 37)
    spheres = f32([[0.0, 0.0, 0.0, 0.5]])
    good = oe.whole_box(rows, spheres)[0]
    assert oe.table(good, rows, spheres=spheres).all()
    bad = oe.bad_boxes(good)
    assert bad.shape[0] == len(oe.BAD_NAMES) and not oe.table(bad, rows, spheres=spheres).any()
    point = oe.point_boxes(rows, [3])[0]
    assert not oe.table(oe.bad_boxes(point), rows).any()
    boxes = np.concatenate([good[None], oe.random_boxes(rows, 50, 39)])
    assert np.array_equal(oe.table(oe.nan_pads(boxes), rows, spheres=spheres), oe.table(boxes, rows, spheres=spheres))
    # infinite bounds on the right side are no bad boxes: steps 2-3 never separate, what step 1 accepts is accepted
    acc, step1 = oe.triangle_rule(oe.unbounded_boxes(good), *oe.records_of_rows(rows))
    assert np.array_equal(acc, step1) and acc[0].all() and 0 < acc[1].sum() <= 37 and 0 < acc[2].sum() <= 37


def test_nan_and_zero_area_records():
    rows = oe.random_scene(6, 41).reshape(-1, 3, 4)
    rows[1, 1, 0] = np.nan                                               # a NaN in one corner only: fmin / fmax would drop it
    rows[2, 0, 2] = np.inf
    rows[3, 2] = rows[3, 1] = rows[3, 0]                                 # a point
    rows[4, 2] = rows[4, 0] + 2 * (rows[4, 1] - rows[4, 0])              # a needle
    rows = rows.reshape(-1, 4)
    acc = oe.table(np.concatenate([oe.boxes_of([-9.0] * 3, [9.0] * 3), oe.point_boxes(rows, [3])[:1]]), rows)
    assert acc[0].tolist() == [True, False, False, True, True, True]      # what the arithmetic gives: no special case
    assert acc[1].tolist() == [False, False, False, True, False, False]


def test_sphere_boxes_and_point_boxes_reach_what_they_are_for():
    for s in ([0.0, 0.0, 0.0, 0.5], [8.0, 0.0, -4.0, 0.5], [-5.0, 0.0, 0.0, 1.5]):
        boxes, want = oe.sphere_boxes(s)
        assert oe.sphere_rule(boxes, f32([s]))[:, 0].tolist() == want.tolist()
    rows = lc.rooms()
    tris = np.arange(0, 480, 11)
    acc = oe.table(oe.point_boxes(rows, tris), rows)
    for i, j in enumerate(tris):
        assert acc[i, j] and acc[len(tris) + i, j]                       # on the vertex; inside the face
        assert acc[i].sum() >= 4 and acc[len(tris) + i].sum() == 1       # a lattice vertex is shared; a face point is not


def test_the_populations_reach_every_kind_of_count(random1100):
    rows, boxes, _ = random1100
    boxes = np.concatenate([boxes, oe.whole_box(rows)])
    for k in (1, 4, 16):
        _, counts = oe.expected(boxes, rows, k)
        print("max_hits %d: counts of 0: %d, of 1: %d, exactly max_hits: %d, more: %d" %
              (k, (counts == 0).sum(), (counts == 1).sum(), (counts == k).sum(), (counts > k).sum()))
        assert (counts == 0).any() and (counts == 1).any() and (counts > k).any()
        assert (counts == k).any() or k == 16
    boxes16 = oe.random_boxes(rows, 300, 23, width=2.0)
    _, counts = oe.expected(boxes16, rows, 16)
    assert (counts == 16).any()
