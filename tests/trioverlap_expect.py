"""Test side of the triangle-shaped region query (rt_tracer_overlap_triangles, csrc/rt_trioverlap.hpp): the
triangle and sphere rules of include/rt_mi355x.h in numpy float32, operation by operation, as a table queries x prims; the
expected rows and counts by brute force; the traversal restated over a dumped tree, with two switches that break it; two
independently written float64 tests (a separating-axis test with per-axis margins, and six segments through two triangles); and
the query populations of the tests.  A helper, not a test.  Everything is deterministic and needs no device."""
import numpy as np

import closest_expect as ce
from overlap_expect import EPS, K, MAX_HITS, NONE, accepted_sets, chain, corners, random_scene, rows_of_table, same, walk_tree  # noqa: F401  (re-exported)
from query_accel_expect import records_of_rows
from query_expect import cross3 as _cross, dot3 as _dot

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def queries_of(tris):
    """(n, 12) float32 {P0 xyz, 0, P1 xyz, 0, P2 xyz, 0} from (n, 3, 3) corners."""
    t = np.asarray(tris, f32).reshape(-1, 3, 3)
    q = np.zeros((t.shape[0], 3, 4), f32)
    q[:, :, :3] = t
    return q.reshape(-1, 12)


def corners_of(queries):
    """(n, 3, 3): the three corners of (n, 12) queries, the pads dropped."""
    return np.asarray(queries, f32).reshape(-1, 3, 4)[:, :, :3]


def _axis_separates(x, rec, qry):
    """The rule of one axis, written as the header states it: every record projection > every query projection, or every one <.
    Nine plain comparisons each way; a NaN makes its comparisons false."""
    r = [_dot(x, v) for v in rec]
    q = [np.zeros_like(r[0])] + [_dot(x, v) for v in qry]
    assert all(v.dtype == f32 for v in r + q)
    above = np.ones(r[0].shape, bool)
    below = np.ones(r[0].shape, bool)
    for rv in r:
        for qv in q:
            above &= rv > qv
            below &= rv < qv
    return above | below


def separated_pairs(P, A, B, C, e1, e2):
    """Steps 2 and 3 on m pairs: P (m, 3, 3) the query corners, A, B, C, e1, e2 (m, 3) the record -> (m,) bool, true when one of
    the seventeen axes separates."""
    with np.errstate(all="ignore"):
        P0 = [P[:, 0, k] for k in range(3)]
        a, b, c = (_sub([V[:, k] for k in range(3)], P0) for V in (A, B, C))
        p1, p2 = (_sub([P[:, i, k] for k in range(3)], P0) for i in (1, 2))
        E1, E2 = [e1[:, k] for k in range(3)], [e2[:, k] for k in range(3)]
        f = [E1, _sub(c, b), _sub(a, c)]
        g = [p1, _sub(p2, p1), p2]
        n, m = _cross(E1, E2), _cross(p1, p2)
        axes = [n, m] + [_cross(fi, gj) for fi in f for gj in g] + [_cross(n, fi) for fi in f] + [_cross(m, gj) for gj in g]
        assert len(axes) == 17
        sep = np.zeros(P.shape[0], bool)
        for x in axes:
            sep |= _axis_separates(x, (a, b, c), (p1, p2))
    return sep


def step1(queries, v0, e1, e2):
    """(N, T) bool: the box step, dense."""
    P = corners_of(queries)
    with np.errstate(all="ignore"):
        A, B, C = v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)
        finite = np.isfinite(P).all(axis=(1, 2))
        ok = np.broadcast_to(finite[:, None], (P.shape[0], v0.shape[0])).copy()
        for k in range(3):
            qmin = np.fmin(np.fmin(P[:, 0, k], P[:, 1, k]), P[:, 2, k])[:, None]
            qmax = np.fmax(np.fmax(P[:, 0, k], P[:, 1, k]), P[:, 2, k])[:, None]
            tmin = np.fmin(np.fmin(A[:, k], B[:, k]), C[:, k])[None, :]
            tmax = np.fmax(np.fmax(A[:, k], B[:, k]), C[:, k])[None, :]
            ok &= ~(np.isnan(B[:, k]) | np.isnan(C[:, k]))[None, :] & (tmin <= qmax) & (tmax >= qmin)
    return ok


def triangle_rule(queries, v0, e1, e2, box_step=True):
    """Every query against every record: queries (N, 12), v0, e1, e2 (T, 3) float32 -> (accepted, step 1) bool (N, T).  The text
    of include/rt_mi355x.h, one float32 operation per operation; steps 2-3 run on the pairs step 1 passes.  box_step=False: a
    rule WITHOUT step 1's three box axes (it keeps "the query is finite" and "no NaN corner"), on every pair, for the test
    that shows what step 1 is for."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (v0, e1, e2))
    s1 = step1(queries, v0, e1, e2)
    P = corners_of(queries)
    with np.errstate(all="ignore"):
        B, C = (v0 + e1).astype(f32), (v0 + e2).astype(f32)
        if box_step:
            cand = s1
        else:
            cand = np.isfinite(P).all(axis=(1, 2))[:, None] & ~(np.isnan(B) | np.isnan(C)).any(axis=1)[None, :]
    i, j = np.nonzero(cand)
    acc = np.zeros(s1.shape, bool)
    if i.size:
        acc[i, j] = ~separated_pairs(P[i], v0[j], B[j], C[j], e1[j], e2[j])
    return acc, s1


def sphere_rule(queries, spheres):
    """(N, S) bool: the sphere rule, one float32 operation per operation (closest_expect.closest_triangle on the query's own
    record for d2min)."""
    P = corners_of(queries)
    s = np.asarray(spheres, f32).reshape(-1, 4)
    out = np.zeros((P.shape[0], s.shape[0]), bool)
    with np.errstate(all="ignore"):
        finite = np.isfinite(P).all(axis=(1, 2))
        p1, p2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        for j in range(s.shape[0]):
            d2min = ce.closest_triangle(s[j:j + 1, :3], P[:, 0], p1, p2)[0][0]     # t of (1 point, N records)
            w = [[P[:, i, k] - s[j, k] for k in range(3)] for i in range(3)]
            d2 = [_dot(wi, wi) for wi in w]
            d2max = np.fmax(np.fmax(d2[0], d2[1]), d2[2])
            rr = s[j, 3] * s[j, 3]
            assert d2min.dtype == f32 and d2max.dtype == f32 and rr.dtype == f32
            out[:, j] = finite & (d2min <= rr) & (rr <= d2max)
    return out


def table(queries, rows, edges=False, spheres=None, box_step=True):
    """(N, P) bool, column = prim: the triangles' verdicts, then the spheres'."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    n = queries.shape[0]
    if rows is None or len(rows) == 0:
        acc = np.zeros((n, 0), bool)
    else:
        acc = triangle_rule(queries, *records_of_rows(rows, edges), box_step=box_step)[0]
    if spheres is not None and len(spheres):
        acc = np.c_[acc, sphere_rule(queries, spheres)]
    return acc


def expected(queries, rows, max_hits, after=None, edges=False, spheres=None):
    """Brute force -> (prims (n, max_hits) int32, counts (n,) uint32)."""
    return rows_of_table(table(queries, rows, edges, spheres), max_hits, after)


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_triangles(nodes, recs, info, queries, rows, max_hits, after=None, edges=False, spheres=None, closed=True,
                        box_step=True, stats=None):
    """overlap_expect.walk_tree (region_bvh_kernel in numpy) for query triangles: the bounding box of the corners, all of them
    finite.  Switches that break one thing each: closed=False; box_step=False walks with the rule that lacks step 1."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    P = corners_of(queries)

    def bounds(i):
        return (P[i].min(axis=0), P[i].max(axis=0)) if np.isfinite(P[i]).all() else None
    return walk_tree(nodes, recs, info, table(queries, rows, edges, spheres, box_step=box_step), bounds, max_hits, after, closed,
                     stats=stats)


# ---- float64, written independently ---------------------------------------------------------------------------------------

def box_pairs(queries, rows, edges=False):
    """The pairs (i, j) whose fp32 bounding boxes touch (comparisons of fp32 numbers are exact in any precision, so this is step
    1 and at the same time three valid separating axes of the float64 tests: a pair outside it does not intersect)."""
    s1 = step1(np.asarray(queries, f32).reshape(-1, 12), *records_of_rows(rows, edges))
    return np.nonzero(s1)


def sat64(queries, rows, i, j, edges=False):
    """Separating axes in float64 on the fp32 corners of the pairs (i, j): the two normals, the nine edge-edge crosses and the six
    in-plane edge normals -> (overlap (m,) bool, margin (m,): the least |signed separation| over the axes, each axis normalised,
    a degenerate axis left out; scale (m,): the largest |coordinate| of the pair).  separation > 0: the axis separates by that
    distance.  Written on absolute coordinates with numpy's own cross and matrix products: nothing is shared with the fp32 rule."""
    Q = corners_of(queries).astype(np.float64)[i]                        # (m, 3, 3)
    A, B, C = (x.astype(np.float64)[j] for x in corners(rows, edges))
    R = np.stack([A, B, C], axis=1)
    fe = [R[:, 1] - R[:, 0], R[:, 2] - R[:, 1], R[:, 0] - R[:, 2]]
    ge = [Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 1], Q[:, 0] - Q[:, 2]]
    n, m = np.cross(fe[0], -fe[2]), np.cross(ge[0], -ge[2])
    axes = [n, m] + [np.cross(a, b) for a in fe for b in ge] + [np.cross(n, a) for a in fe] + [np.cross(m, b) for b in ge]
    worst = np.full(Q.shape[0], -np.inf)
    margin = np.full(Q.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for ax in axes:
            ln = np.sqrt((ax * ax).sum(-1))
            pr = np.einsum("mck,mk->mc", R, ax)
            pq = np.einsum("mck,mk->mc", Q, ax)
            sep = np.maximum(pr.min(axis=1) - pq.max(axis=1), pq.min(axis=1) - pr.max(axis=1)) / ln
            ok = ln > 0
            worst = np.where(ok, np.maximum(worst, sep), worst)
            margin = np.where(ok, np.minimum(margin, np.abs(sep)), margin)
    scale = np.maximum(np.abs(R).max(axis=(1, 2)), np.abs(Q).max(axis=(1, 2)))
    return worst <= 0, margin, scale


def _segment_hits64(S0, S1, T):
    """(m,) bool: the closed segment S0 S1 meets the closed triangle T (m, 3, 3), in float64, general position (a segment in the
    triangle's plane counts as a miss)."""
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    d = S1 - S0
    h = np.cross(d, e2)
    det = (e1 * h).sum(-1)
    with np.errstate(all="ignore"):
        s = S0 - T[:, 0]
        u = (s * h).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def edges64(queries, rows, i, j, edges=False):
    """Two triangles in general position intersect exactly when an edge of one passes through the other: six segments per
    pair, in float64 -> (m,) bool."""
    Q = corners_of(queries).astype(np.float64)[i]
    R = np.stack([x.astype(np.float64)[j] for x in corners(rows, edges)], axis=1)
    hit = np.zeros(Q.shape[0], bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        hit |= _segment_hits64(Q[:, a], Q[:, b], R) | _segment_hits64(R[:, a], R[:, b], Q)
    return hit


# ---- queries -----------------------------------------------------------------------------------------------------------------

def random_queries(n, seed, edge=0.25, span=1.0, snap=None):
    """n query triangles of edge about `edge` with centres uniform in [-span, span]^3 (overlap_expect.random_scene's recipe)."""
    return random_scene(n, seed, edge=edge, span=span, snap=snap).reshape(-1, 12)


def queries_near(rows, n, seed, edge=0.5, edges=False):
    """n query triangles of edge about `edge` around random finite corners of the scene: most touch something."""
    rng = np.random.default_rng(seed)
    A, B, C = corners(rows, edges)
    fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1)
    pick = np.nonzero(fin)[0][rng.integers(0, fin.sum(), n)]
    t = A[pick].astype(np.float64)[:, None, :] + rng.uniform(-edge / 2, edge / 2, (n, 1, 3)) + rng.uniform(-edge / 2, edge / 2, (n, 3, 3))
    return queries_of(t)


PAIRINGS = [(s, c) for s in range(3) for c in range(3)]                 # query corner s is record corner c (A, B, C)


def shared_corner_queries(rows, tris, seed, far=50.0, edges=False, both=False):
    """For each triangle j of `tris` and each of the nine pairings: a query whose corner s is bit-equal to corner c of record j,
    the other two corners far-flung (uniform in [-far, far]^3) -- or, with both=True, a second corner on the record's next
    corner as well (a shared edge).  -> (queries, tags [(j, s, c)])."""
    rng = np.random.default_rng(seed)
    ABC = np.stack(corners(rows, edges), axis=1)                         # (T, 3, 3)
    out, tags = [], []
    for j in tris:
        for s, c in PAIRINGS:
            t = rng.uniform(-far, far, (3, 3)).astype(f32)
            t[s] = ABC[j, c]
            if both:
                t[(s + 1) % 3] = ABC[j, (c + 1) % 3]
            out.append(t), tags.append((int(j), s, c))
    return queries_of(out), tags


def coplanar_queries(rows, tris, edges=False):
    """Neighbours in a record's own plane, as far as fp32 places them there: the reflection over the edge BC (B, C, B + C - A:
    shares an edge), the record shifted by half of e1 (coplanar and crossing), by three e1 (coplanar and apart), and the record
    itself."""
    A, B, C = corners(rows, edges)
    out = []
    for j in tris:
        a, b, c = A[j], B[j], C[j]
        e1 = b - a
        out += [[b, c, (b + c) - a], [a + f32(0.5) * e1, b + f32(0.5) * e1, c + f32(0.5) * e1],
                [a + f32(3) * e1, b + f32(3) * e1, c + f32(3) * e1], [a, b, c]]
    return queries_of(out)


BAD_VALUES = (NAN, INF, -INF)


def bad_queries(query):
    """The queries that accept nothing, made from one good query (12,): each of the nine coordinates a NaN, +inf and -inf.
    -> (27, 12)."""
    out = np.repeat(np.asarray(query, f32).reshape(1, 12), 27, axis=0)
    for c in range(9):
        for v, bad in enumerate(BAD_VALUES):
            out[3 * c + v, 4 * (c // 3) + c % 3] = bad
    return out


def nan_pads(queries):
    """The same queries with NaNs in the three pad floats."""
    out = np.array(queries, f32).reshape(-1, 12).copy()
    out[:, [3, 7, 11]] = NAN
    return out


def mixed_queries(rows, n, seed, edges=False):
    """The device tests' batch of n queries: random triangles around the scene, triangles sharing a record's corner or edge bit
    for bit, coplanar neighbours, and the non-finite and NaN-pad queries, shuffled together deterministically."""
    rng = np.random.default_rng(seed)
    n_tris = np.asarray(rows).shape[0] // 3
    A, B, C = corners(rows, edges)
    fin = np.nonzero(np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1))[0]
    some = fin[rng.integers(0, fin.size, max(1, min(n // 72, 12)))] if fin.size else np.zeros(0, np.int64)
    parts = []
    if some.size:
        parts += [shared_corner_queries(rows, some, seed + 1, far=2.0, edges=edges)[0],
                  shared_corner_queries(rows, some, seed + 2, far=2.0, edges=edges, both=True)[0], coplanar_queries(rows, some, edges)]
    good = queries_near(rows, 1, seed + 3, edges=edges)[0] if fin.size else queries_of([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])[0]
    parts += [bad_queries(good), nan_pads(good[None])]
    special = np.concatenate(parts)[:max(n // 2, 0)]
    m = n - special.shape[0]
    wide = queries_near(rows, m // 4, seed + 4, edge=4.0, edges=edges) if fin.size and m >= 4 else np.zeros((0, 12), f32)
    rest = m - wide.shape[0]
    rand = queries_near(rows, rest, seed + 5, edges=edges) if fin.size else random_queries(rest, seed + 5)
    out = np.concatenate([special, wide, rand])
    assert out.shape == (n, 12) and n_tris >= 0
    return np.ascontiguousarray(out[rng.permutation(n)])


# ---- pinned degenerate cases -------------------------------------------------------------------------------------------------

def degenerate_cases():
    """Zero-area triangles on either side, dyadic so that every operation is exact: (rows of one record, query (12,), accepted).
    The record is the triangle (0,0,0) (4,0,0) (0,4,0) unless it is a needle."""
    tri = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    rec_needle = [[0, 0, 0], [4, 4, 0], [4, 4, 0]]                       # the segment (0,0,0)-(4,4,0)
    pt = lambda p: [p, p, p]
    cases = [
        ("a point inside", tri, pt([1, 1, 0]), True),
        ("a point on a corner", tri, pt([4, 0, 0]), True),
        ("a point in the plane, outside", tri, pt([3, 3, 0]), False),
        ("a point above", tri, pt([1, 1, 0.5]), False),
        ("a needle through", tri, [[1, 1, -1], [1, 1, 1], [1, 1, 1]], True),
        ("a needle through, its end on the face", tri, [[1, 1, 0], [1, 1, 2], [1, 1, 0]], True),
        ("a needle beside", tri, [[3, 3, -1], [3, 3, 1], [3, 3, 1]], False),
        ("a needle short of the face", tri, [[1, 1, 0.25], [1, 1, 1], [1, 1, 1]], False),
        ("two crossing needles", rec_needle, [[4, 0, 0], [0, 4, 0], [0, 4, 0]], True),
        ("two skew needles", rec_needle, [[4, 0, 1], [0, 4, 1], [0, 4, 1]], False),
    ]
    out = []
    for name, rec, q, want in cases:
        r = np.zeros((3, 4), f32)
        r[:, :3] = rec
        out.append((name, r, queries_of([q])[0], want))
    return out


# ---- SelfIntersections ------------------------------------------------------------------------------------------------------

def cube_rows(lo=-1.0, hi=1.0):
    """A closed cube of 12 triangles, (36, 4) vertex rows."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], f32)      # index = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, c, d in quads:
        tris += [[v[a], v[b], v[c]], [v[a], v[c], v[d]]]
    r = np.zeros((12, 3, 4), f32)
    r[:, :, :3] = tris
    return r.reshape(-1, 4)


def poked_cube_rows():
    """The cube and a thirteenth triangle poked through its face x = +1: the triangle crosses that face's two triangles (prims 2
    and 3) and nothing else.  -> (rows, the pierced pairs)."""
    poke = np.zeros((3, 4), f32)
    poke[:, :3] = [[0.5, 0.25, -0.125], [1.5, 0.5, 0.375], [1.5, -0.25, 0.25]]
    return np.concatenate([cube_rows(), poke]), [(2, 12), (3, 12)]


def to_edges(rows):
    """The same triangles in the edge layout (v0, e1, e2)."""
    r = np.asarray(rows, f32).reshape(-1, 3, 4).copy()
    r[:, 1, :3], r[:, 2, :3] = r[:, 1, :3] - r[:, 0, :3], r[:, 2, :3] - r[:, 0, :3]
    return r.reshape(-1, 4)
