"""The hexahedron-shaped region query's test side, checked without a device: the restated fp32 rule agrees with an independent
float64 separating-axis test and with a float64 clipping of the record by the six face planes; segments agree with a float64
segment-through-triangle test; on the 1/8 lattice aligned boxes give exactly overlap_expect's accepted sets; non-finite regions
accept nothing; the sphere rule is the surface against a solid; and the restated traversal of a tree from rt_dbg_bvh_build
equals brute force, with open comparisons does not, and with a shortened stack still does."""
import numpy as np
import pytest

import hexoverlap_expect as he
import lattice_cases as lc
import overlap_expect as oe

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def library_has_the_query():
    """The rule restated here is the one of the library under test: without rt_tracer_overlap_hexahedra there is nothing to
    restate."""
    from raytracertest_amd import api
    assert hasattr(api.load_library(), "rt_tracer_overlap_hexahedra") and hasattr(api.RayTracer, "OverlapHexahedra")


@pytest.mark.parametrize("kind", ["frusta", "boxes", "pyramids"])
def test_the_fp32_rule_equals_the_float64_axes_and_the_clipping(kind):
    """20 000 pairs of each kind, the region's centre within 0.6 of the record's centroid.  A disagreement is excused only when
    the float64 test's deciding axis has a gap below 16 * 2^-24 * scale; at most 1 % may be excused.  Measured here:
        frusta:   7 833 past the box step, 2 423 accepted, 0 differ from the float64 axes, 0 from the clipping
        boxes:    4 892 past the box step, 1 117 accepted, 0 and 0
        pyramids: 8 717 past the box step, 2 686 accepted, 0 and 0"""
    n = 20000
    H, v0, e1, e2 = he.pair_population(kind, n, {"frusta": 1, "boxes": 2, "pyramids": 3}[kind])
    acc, s1 = he.pair_rule(H, v0, e1, e2)
    B, C = v0 + e1, v0 + e2
    overlap, margin, scale = he.sat64(H, v0, B, C)
    clipped = he.clip64(H, v0, B, C)
    assert not overlap[~s1].any() and not clipped[~s1].any()            # outside the boxes every side says no, exactly
    share = acc.mean()
    print("%s: %d pairs, %d past the box step, %d accepted (%.1f %%), %d differ from the float64 axes, %d from the clipping" %
          (kind, n, s1.sum(), acc.sum(), 100 * share, (acc != overlap).sum(), (acc != clipped).sum()))
    assert 0.05 <= share <= 0.15
    for other in (overlap, clipped):
        differ = acc != other
        excused = differ & (margin < he.K * he.EPS * scale)
        assert (differ == excused).all()                                 # a disagreement needs a gap within rounding
        assert excused.sum() <= 0.01 * n
    assert np.array_equal(overlap, clipped) or ((overlap != clipped) <= (margin < he.K * he.EPS * scale)).all()


def test_segments_agree_with_a_float64_segment_through_triangle_test():
    """Measured: 20 000 segments of length 0.18 to 0.6 within 0.6 of a record, 164 accepted, none differs."""
    H, v0, e1, e2 = he.pair_population("segments", 20000, 4)
    acc, _ = he.pair_rule(H, v0, e1, e2)
    through = he.segment64(H, v0, v0 + e1, v0 + e2)
    print("segments: %d accepted, %d differ" % (acc.sum(), (acc != through).sum()))
    assert acc.sum() > 100
    assert np.array_equal(acc, through)


def test_on_the_eighth_lattice_aligned_boxes_give_exactly_the_box_query_s_sets():
    """Corners and records on multiples of 1/8 in [-2, 2]^3: every product and sum of the rule is exact, so the forty-three axes
    and Overlap's thirteen decide the same pairs, touching pairs included."""
    rows = oe.random_scene(400, 5, edge=1.0, span=1.5, snap=0.125)
    rows = np.clip(rows, -2, 2)
    rng = np.random.default_rng(6)
    lo = np.round(rng.uniform(-2, 1.5, (600, 3)) * 8) / 8
    hi = np.minimum(lo + np.round(rng.uniform(0, 1.0, (600, 3)) * 8) / 8, 2.0)          # flat and point boxes among them
    touching, tags = oe.touching_boxes(rows, range(0, 400, 9))
    touching = touching[[t[2] for t in tags]]                            # hi EQUAL to the record's minimum: on the lattice too
    boxes = np.concatenate([oe.boxes_of(lo, hi), touching])
    want = oe.table(boxes, rows)
    from raytracertest_amd.api import RayTracer as R
    corners = R.box_corners(boxes[:, 0:3], boxes[:, 4:7])
    assert np.array_equal(corners, he.box_corners(boxes[:, 0:3], boxes[:, 4:7]))
    got = he.table(he.queries_of(corners), rows)
    print("lattice: %d boxes, %d accepted pairs, %d differ" % (boxes.shape[0], want.sum(), (got != want).sum()))
    assert want.sum() > 2000 and want[600:].any(axis=1).all()
    assert np.array_equal(got, want)


def test_non_finite_regions_accept_nothing_and_nan_pads_change_nothing():
    rows = he.random_scene(37, 37)
    spheres = f32([[0.0, 0.0, 0.0, 0.5]])
    good = he.queries_of(he.box_corners([-2, -2, -0.25], [2, 2, 0.25]))[0]  # through the scene and the sphere
    acc = he.table(good, rows, spheres=spheres)
    assert acc[0, :37].any() and acc[0, 37]
    bad = he.bad_queries(good)
    assert bad.shape == (72, 32) and not np.isfinite(he.corners_of(bad)).all(axis=(1, 2)).any()
    assert not he.table(bad, rows, spheres=spheres).any()
    queries = np.concatenate([good[None], he.regions_near(rows, 50, 39)])
    assert np.array_equal(he.table(he.nan_pads(queries), rows, spheres=spheres), he.table(queries, rows, spheres=spheres))


def test_nan_and_infinite_records():
    rows = he.random_scene(6, 41).reshape(-1, 3, 4)
    rows[1, 1, 0] = np.nan                                               # a NaN in one corner only: fmin / fmax would drop it
    rows[2, 0, 2] = np.inf
    rows = rows.reshape(-1, 4)
    big = he.queries_of(he.box_corners([-9, -9, -9], [9, 9, 40]))
    acc = he.table(big, rows)
    assert acc[0, [0, 3, 4, 5]].all() and not acc[:, 1].any() and not acc[:, 2].any()


def test_the_sphere_rule_is_the_surface_against_a_solid():
    """The last case is the header's caveat: a region without volume has six zero face normals, which separate nothing, so every
    centre counts as inside it and only the farthest corner decides."""
    s = f32([[0.0, 0.0, 0.0, 1.0]])
    box = lambda c, r: he.box_corners([c[0] - r, c[1] - r, c[2] - r], [c[0] + r, c[1] + r, c[2] + r])[0]
    queries = he.queries_of([box((0, 0, 0), 0.25),                       # wholly inside the ball: touches nothing
                             box((0, 0, 0), 3.0),                        # the ball wholly inside the region: accepted
                             box((1.5, 0, 0), 1.0),                      # one face cuts the ball
                             box((2, 0, 0), 1.0),                        # tangent at (1, 0, 0)
                             box((3, 3, 3), 0.5),                        # beyond
                             he.segments([[0, 0, -3]], [[0, 0, 3]])[0],  # a segment through the ball
                             he.segments([[0, 0, -0.5]], [[0, 0, 0.5]])[0],   # a segment inside it
                             he.segments([[2, 0, -3]], [[2, 0, 3]])[0]])      # a segment beside it: no face normal, "inside"
    assert he.sphere_rule(queries, s)[:, 0].tolist() == [False, True, True, True, False, True, False, True]


@pytest.fixture(scope="module")
def random1100():
    from raytracertest_amd import api
    rows = he.random_scene(1100, 21, span=3.0, edge=0.6)
    return rows, he.regions_near(rows, 300, 22, size=0.6), api.bvh_build(rows)


@pytest.fixture(scope="module")
def rooms():
    """The lattice scene and regions whose bounding boxes end ON its planes: aligned boxes and frusta between lattice points."""
    from raytracertest_amd import api
    rows = lc.rooms()
    rng = np.random.default_rng(8)
    lo = np.round(rng.uniform(-2, 2, (200, 3))) - lc.SHIFT
    hi = lo + np.round(rng.uniform(0, 2, (200, 3)))
    boxes = he.box_corners(lo, hi)
    skew = boxes.copy()
    skew[:, 4:, :2] += f32(0.5) * (skew[:, 4:, :2] - skew[:, :4, :2].mean(axis=1, keepdims=True))   # the far cap wider: frusta
    return rows, he.queries_of(np.concatenate([boxes, skew[:100]])), api.bvh_build(rows)


def test_the_walk_equals_brute_force_and_prunes_on_the_random_scene(random1100):
    rows, queries, (nodes, recs, info) = random1100
    acc = he.table(queries, rows)
    for k in (0, 4, 16):
        prims, counts, tests = he.walk_tree_hexahedra(nodes, recs, info, queries, rows, k, acc=acc)
        assert he.same((prims, counts), he.rows_of_table(acc, k))
    share = tests / (queries.shape[0] * 1100.0)
    print("triangle tests: %.4f of the scan's" % share)
    assert share < 0.05 and counts.any()


def test_the_walk_equals_brute_force_on_the_lattice_and_open_comparisons_do_not(rooms):
    """A region whose bounding box ends on a wall's plane only touches the boxes of that wall's leaves: with closed=False the
    walk loses those records, which shows that the closed comparison carries the exactness."""
    rows, queries, (nodes, recs, info) = rooms
    acc = he.table(queries, rows)
    want = he.rows_of_table(acc, 16)
    prims, counts, _ = he.walk_tree_hexahedra(nodes, recs, info, queries, rows, 16, acc=acc)
    assert he.same((prims, counts), want) and (counts > 16).any()
    prims, counts, _ = he.walk_tree_hexahedra(nodes, recs, info, queries, rows, 16, closed=False, acc=acc)
    print("open comparisons: %d of %d regions change" % ((counts != want[1]).sum(), counts.shape[0]))
    assert not he.same((prims, counts), want) and counts.sum() < want[1].sum()


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_a_shortened_stack_restarts_and_still_equals_brute_force(random1100, cap):
    rows, queries, (nodes, recs, info) = random1100
    acc = he.table(queries[:60], rows)
    prims, counts, tests = he.walk_tree_hexahedra(nodes, recs, info, queries[:60], rows, 16, stack_cap=cap, acc=acc)
    assert he.same((prims, counts), he.rows_of_table(acc, 16))
    assert cap > 1 or tests >= 60 * 1100 * 0.5                           # most walks had to start again


def test_the_populations_reach_every_kind_of_count(random1100):
    rows, _, _ = random1100
    queries = he.mixed_queries(rows, 600, 7)
    acc = he.table(queries, rows)
    for k in (1, 4, 16):
        _, counts = he.rows_of_table(acc, k)
        assert (counts == 0).any() and (counts == 1).any() and (counts > k).any()
    assert not np.isfinite(he.corners_of(queries)).all(axis=(1, 2)).all() and np.isnan(queries[:, 3::4]).any()
