"""Test side of the hexahedron-shaped region query (rt_tracer_overlap_hexahedra, csrc/rt_hexoverlap.hpp): the
triangle and sphere rules of include/rt_mi355x.h in numpy float32, operation by operation, as a table regions x prims; the
expected rows and counts by brute force; the traversal restated over a dumped tree, with a switch that breaks it and a stack
cap; two independently written float64 tests (separating axes with per-axis margins, and the record clipped by the six face
planes), a float64 segment test; and the region populations of the tests.  A helper, not a test.  Everything is deterministic
and needs no device."""
import numpy as np

import closest_expect as ce
from overlap_expect import EPS, K, MAX_HITS, NONE, accepted_sets, chain, corners, random_scene, rows_of_table, same, walk_tree  # noqa: F401  (re-exported)
from query_accel_expect import records_of_rows
from trioverlap_expect import _cross, _dot, _segment_hits64, _sub

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)

FACES = [(0, 2, 4, 6), (1, 3, 5, 7), (0, 1, 4, 5), (2, 3, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7)]      # (a, b, c, d): diagonals a-d, b-c
EDGES = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
FACE_TRIANGLES = [t for a, b, c, d in FACES for t in ((a, b, d), (a, d, c))]


def queries_of(corners8):
    """(n, 32) float32, eight rows {C_k xyz, 0}, from (n, 8, 3) corners."""
    c = np.asarray(corners8, f32).reshape(-1, 8, 3)
    q = np.zeros((c.shape[0], 8, 4), f32)
    q[:, :, :3] = c
    return q.reshape(-1, 32)


def corners_of(queries):
    """(n, 8, 3): the eight corners of (n, 32) queries, the pads dropped."""
    return np.asarray(queries, f32).reshape(-1, 8, 4)[:, :, :3]


def _min_all(v):
    out = v[0]
    for x in v[1:]:
        out = np.fmin(out, x)
    return out


def _max_all(v):
    out = v[0]
    for x in v[1:]:
        out = np.fmax(out, x)
    return out


def _nan_any(v):
    out = np.isnan(v[0])
    for x in v[1:]:
        out = out | np.isnan(x)
    return out


def _moved(H):
    """C0 and h_1 .. h_7 as lists of three component arrays; h_0 is the literal 0."""
    C0 = [H[:, 0, k] for k in range(3)]
    zero = [np.zeros_like(C0[0]) for _ in range(3)]
    return C0, [zero] + [_sub([H[:, i, k] for k in range(3)], C0) for i in range(1, 8)]


def _diff(h, j, i):
    """h_j - h_i; h_0 is the literal 0, and x - 0 is x."""
    return h[j] if i == 0 else _sub(h[j], h[i])


def _face_normals(h):
    return [_cross(_diff(h, d, a), _diff(h, c, b)) for a, b, c, d in FACES]


def _axis_separates(x, rec, h):
    """The rule of one axis, as the header states it: the record's minimum > the region's maximum, or its maximum < the region's
    minimum, and none of the ten projections a NaN."""
    r = [_dot(x, v) for v in rec]
    q = [np.zeros_like(r[0])] + [_dot(x, v) for v in h[1:]]
    assert all(v.dtype == f32 for v in r + q)
    return ~_nan_any(r + q) & ((_min_all(r) > _max_all(q)) | (_max_all(r) < _min_all(q)))


def separated_pairs(H, A, B, C, e1, e2):
    """Steps 2 to 4 on m pairs: H (m, 8, 3) the corners, A, B, C, e1, e2 (m, 3) the record -> (m,) bool, true when one of the
    forty-three axes separates."""
    with np.errstate(all="ignore"):
        C0, h = _moved(H)
        a, b, c = (_sub([V[:, k] for k in range(3)], C0) for V in (A, B, C))
        E1, E2 = [e1[:, k] for k in range(3)], [e2[:, k] for k in range(3)]
        f = [E1, _sub(c, b), _sub(a, c)]
        axes = [_cross(E1, E2)] + _face_normals(h) + [_cross(fi, _diff(h, j, i)) for i, j in EDGES for fi in f]
        assert len(axes) == 43
        sep = np.zeros(H.shape[0], bool)
        for x in axes:
            sep |= _axis_separates(x, (a, b, c), h)
    return sep


def step1(queries, v0, e1, e2):
    """(N, T) bool: the box step, dense."""
    H = corners_of(queries)
    with np.errstate(all="ignore"):
        A, B, C = v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)
        finite = np.isfinite(H).all(axis=(1, 2))
        ok = np.broadcast_to(finite[:, None], (H.shape[0], v0.shape[0])).copy()
        for k in range(3):
            qmin = _min_all([H[:, i, k] for i in range(8)])[:, None]
            qmax = _max_all([H[:, i, k] for i in range(8)])[:, None]
            tmin = np.fmin(np.fmin(A[:, k], B[:, k]), C[:, k])[None, :]
            tmax = np.fmax(np.fmax(A[:, k], B[:, k]), C[:, k])[None, :]
            ok &= ~(np.isnan(B[:, k]) | np.isnan(C[:, k]))[None, :] & (tmin <= qmax) & (tmax >= qmin)
    return ok


def hexa_rule(queries, v0, e1, e2):
    """Every region against every record: queries (N, 32), v0, e1, e2 (T, 3) float32 -> (accepted, step 1) bool (N, T).  The text
    of include/rt_mi355x.h, one float32 operation per operation; steps 2-4 run on the pairs step 1 passes."""
    queries = np.asarray(queries, f32).reshape(-1, 32)
    v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (v0, e1, e2))
    s1 = step1(queries, v0, e1, e2)
    H = corners_of(queries)
    with np.errstate(all="ignore"):
        B, C = (v0 + e1).astype(f32), (v0 + e2).astype(f32)
    i, j = np.nonzero(s1)
    acc = np.zeros(s1.shape, bool)
    if i.size:
        acc[i, j] = ~separated_pairs(H[i], v0[j], B[j], C[j], e1[j], e2[j])
    return acc, s1


def pair_rule(H, v0, e1, e2):
    """The rule on m pairs (region r against record r): H (m, 8, 3), v0, e1, e2 (m, 3) -> (accepted (m,), step 1 (m,))."""
    H = np.asarray(H, f32).reshape(-1, 8, 3)
    v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (v0, e1, e2))
    with np.errstate(all="ignore"):
        B, C = (v0 + e1).astype(f32), (v0 + e2).astype(f32)
        s1 = np.isfinite(H).all(axis=(1, 2)) & ~(np.isnan(B) | np.isnan(C)).any(axis=1)
        for k in range(3):
            tmin, tmax = np.fmin(np.fmin(v0[:, k], B[:, k]), C[:, k]), np.fmax(np.fmax(v0[:, k], B[:, k]), C[:, k])
            s1 &= (tmin <= _max_all([H[:, i, k] for i in range(8)])) & (tmax >= _min_all([H[:, i, k] for i in range(8)]))
    acc = np.zeros(H.shape[0], bool)
    m = np.nonzero(s1)[0]
    if m.size:
        acc[m] = ~separated_pairs(H[m], v0[m], B[m], C[m], e1[m], e2[m])
    return acc, s1


def sphere_rule(queries, spheres):
    """(N, S) bool: the sphere rule, one float32 operation per operation (closest_expect.closest_triangle on the twelve face
    triangles for d2min)."""
    H = corners_of(queries)
    s = np.asarray(spheres, f32).reshape(-1, 4)
    out = np.zeros((H.shape[0], s.shape[0]), bool)
    with np.errstate(all="ignore"):
        finite = np.isfinite(H).all(axis=(1, 2))
        C0, h = _moved(H)
        normals = _face_normals(h)
        proj = [[np.zeros_like(C0[0])] + [_dot(x, v) for v in h[1:]] for x in normals]
        for j in range(s.shape[0]):
            S = [np.full_like(C0[0], s[j, k]) for k in range(3)]
            sm = _sub(S, C0)
            outside = np.zeros(H.shape[0], bool)
            for x, q in zip(normals, proj):
                ps = _dot(x, sm)
                outside |= ~_nan_any([ps] + q) & ((ps > _max_all(q)) | (ps < _min_all(q)))
            ts = [ce.closest_triangle(s[j:j + 1, :3], H[:, a], H[:, b] - H[:, a], H[:, c] - H[:, a])[0][0] for a, b, c in FACE_TRIANGLES]
            d2min = np.where(outside, _min_all(ts), f32(0))
            w = [[H[:, i, k] - s[j, k] for k in range(3)] for i in range(8)]
            d2max = _max_all([_dot(wi, wi) for wi in w])
            rr = s[j, 3] * s[j, 3]
            assert d2min.dtype == f32 and d2max.dtype == f32 and rr.dtype == f32
            out[:, j] = finite & (d2min <= rr) & (rr <= d2max)
    return out


def table(queries, rows, edges=False, spheres=None, block=512):
    """(N, P) bool, column = prim: the triangles' verdicts, then the spheres'."""
    queries = np.asarray(queries, f32).reshape(-1, 32)
    n = queries.shape[0]
    if rows is None or len(rows) == 0:
        acc = np.zeros((n, 0), bool)
    else:
        rec = records_of_rows(rows, edges)
        acc = np.concatenate([hexa_rule(queries[i:i + block], *rec)[0] for i in range(0, n, block)]) if n else np.zeros((0, rec[0].shape[0]), bool)
    if spheres is not None and len(spheres):
        acc = np.c_[acc, sphere_rule(queries, spheres)]
    return acc


def expected(queries, rows, max_hits, after=None, edges=False, spheres=None):
    """Brute force -> (prims (n, max_hits) int32, counts (n,) uint32)."""
    return rows_of_table(table(queries, rows, edges, spheres), max_hits, after)


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_hexahedra(nodes, recs, info, queries, rows, max_hits, after=None, edges=False, spheres=None, closed=True,
                        stack_cap=None, stats=None, acc=None):
    """overlap_expect.walk_tree (region_bvh_kernel in numpy) for hexahedra: the bounding box of the eight corners, all of them
    finite; the rule is looked up in table(), or in acc when given.  closed and stack_cap are walk_tree's."""
    queries = np.asarray(queries, f32).reshape(-1, 32)
    if acc is None:
        acc = table(queries, rows, edges, spheres)
    H = corners_of(queries)

    def bounds(i):
        return (H[i].min(axis=0), H[i].max(axis=0)) if np.isfinite(H[i]).all() else None
    return walk_tree(nodes, recs, info, acc, bounds, max_hits, after, closed, stack_cap, stats)


# ---- float64, written independently ---------------------------------------------------------------------------------------

def sat64(H, A, B, C):
    """Separating axes in float64 on the fp32 corners of m pairs (H (m, 8, 3) against the triangle A, B, C (m, 3)): the
    triangle's normal, the six face normals (each from two edges at a corner of the face and, where that corner is degenerate,
    at the opposite one) and the 36 edge-edge crosses -> (overlap (m,) bool, margin (m,): the least |signed separation| over
    the axes, each axis normalised, a degenerate axis left out; scale (m,): the largest |coordinate| of the pair).  Written on
    absolute coordinates with numpy's own cross and matrix products: nothing is shared with the fp32 rule."""
    H = np.asarray(H).astype(np.float64)
    R = np.stack([np.asarray(x).astype(np.float64) for x in (A, B, C)], axis=1)
    fe = [R[:, 1] - R[:, 0], R[:, 2] - R[:, 1], R[:, 0] - R[:, 2]]
    axes = [np.cross(fe[0], -fe[2])]
    for a, b, c, d in FACES:
        n1, n2 = np.cross(H[:, b] - H[:, a], H[:, c] - H[:, a]), np.cross(H[:, c] - H[:, d], H[:, b] - H[:, d])
        axes.append(np.where(((n1 * n1).sum(-1) > 0)[:, None], n1, n2))
    axes += [np.cross(f, H[:, j] - H[:, i]) for i, j in EDGES for f in fe]
    worst = np.full(H.shape[0], -np.inf)
    margin = np.full(H.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for ax in axes:
            ln = np.sqrt((ax * ax).sum(-1))
            pr = np.einsum("mck,mk->mc", R, ax)
            pq = np.einsum("mck,mk->mc", H, ax)
            sep = np.maximum(pr.min(axis=1) - pq.max(axis=1), pq.min(axis=1) - pr.max(axis=1)) / ln
            ok = ln > 0
            worst = np.where(ok, np.maximum(worst, sep), worst)
            margin = np.where(ok, np.minimum(margin, np.abs(sep)), margin)
    scale = np.maximum(np.abs(R).max(axis=(1, 2)), np.abs(H).max(axis=(1, 2)))
    return worst <= 0, margin, scale


def clip64(H, A, B, C):
    """The triangle clipped by the region's six face planes in float64 (Sutherland-Hodgman, every pair at once): (m,) bool,
    true when something of the triangle is left.  A face's plane passes through the mean of its four corners with the diagonals'
    cross product as its normal, turned away from the mean of all eight; a face without area (a pyramid's apex) bounds
    nothing and is left out.  For regions with volume in general position."""
    H = np.asarray(H).astype(np.float64)
    m = H.shape[0]
    V = 10                                                               # 3 corners and at most one more per plane
    poly = np.zeros((m, V, 3))
    poly[:, 0], poly[:, 1], poly[:, 2] = (np.asarray(x).astype(np.float64) for x in (A, B, C))
    cnt = np.full(m, 3)
    centre = H.mean(axis=1)
    rows = np.arange(m)
    for a, b, c, d in FACES:
        nrm = np.cross(H[:, d] - H[:, a], H[:, c] - H[:, b])
        p0 = (H[:, a] + H[:, b] + H[:, c] + H[:, d]) / 4
        flip = ((centre - p0) * nrm).sum(-1) > 0
        nrm = np.where(flip[:, None], -nrm, nrm)                         # outward
        live = (nrm * nrm).sum(-1) > 0
        dist = np.einsum("mvk,mk->mv", poly - p0[:, None, :], nrm)      # <= 0: inside
        out = np.zeros_like(poly)
        pos = np.zeros(m, np.int64)
        for v in range(V):
            here = (v < cnt) & live
            nxt = np.where(v + 1 < cnt, v + 1, 0)
            d0, d1 = dist[:, v], dist[rows, nxt]
            keep = here & (d0 <= 0)
            out[rows[keep], pos[keep]] = poly[keep, v]
            pos[keep] += 1
            cross = here & ((d0 <= 0) != (d1 <= 0))
            with np.errstate(all="ignore"):
                t = d0 / (d0 - d1)
                pt = poly[:, v] + t[:, None] * (poly[rows, nxt] - poly[:, v])
            out[rows[cross], pos[cross]] = pt[cross]
            pos[cross] += 1
        poly = np.where(live[:, None, None], out, poly)
        cnt = np.where(live, pos, cnt)
    return cnt > 0


def segment64(H, A, B, C):
    """For regions collapsed to a segment (C0 .. C3 equal, C4 .. C7 equal): the closed segment meets the closed triangle, in
    float64, general position -> (m,) bool."""
    H = np.asarray(H).astype(np.float64)
    T = np.stack([np.asarray(x).astype(np.float64) for x in (A, B, C)], axis=1)
    return _segment_hits64(H[:, 0], H[:, 4], T)


# ---- regions -----------------------------------------------------------------------------------------------------------------

def box_corners(lo, hi):
    """(n, 8, 3): the corners of axis-aligned boxes in the query's order (api.RayTracer.box_corners restated)."""
    lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
    pick = np.array([[(k >> ax) & 1 for ax in range(3)] for k in range(8)], bool)
    return np.where(pick[None], hi[:, None, :], lo[:, None, :]).astype(f32)


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def frusta(centres, seed, size=0.3, pyramid=False):
    """One frustum per centre (n, 3): an eye behind the centre, four corner rays of a random field of view, cut at near and far
    so that the region is about `size` long and wide and `centres` lies in its middle.  pyramid=True: near = 0, the four near
    corners are the apex bit for bit."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    n = c.shape[0]
    w = _directions(rng, n)
    u = np.cross(w, _directions(rng, n))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(w, u)
    far = rng.uniform(1.0, 2.0, n) * size
    near = np.zeros(n) if pyramid else far * rng.uniform(0.1, 0.6, n)
    eye = c - w * ((near + far) / 2)[:, None]
    tx, ty = rng.uniform(0.2, 0.7, (2, n))
    out = np.empty((n, 8, 3), f32)
    for k, (sx, sy) in enumerate(((-1, -1), (1, -1), (-1, 1), (1, 1))):
        d = w + sx * tx[:, None] * u + sy * ty[:, None] * v
        out[:, k] = (eye + near[:, None] * d).astype(f32)
        out[:, k + 4] = (eye + far[:, None] * d).astype(f32)
    if pyramid:
        out[:, 1:4] = out[:, :1]
    return out


def sheared_boxes(centres, seed, size=0.3):
    """One box per centre with three random, neither unit nor orthogonal half-axes of length about size / 2 (planar faces)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    n = c.shape[0]
    ax = _directions(rng, 3 * n).reshape(n, 3, 3) * rng.uniform(0.2, 0.6, (n, 3, 1)) * size
    ax[:, 2] = np.where((np.linalg.det(ax) < 0)[:, None], -ax[:, 2], ax[:, 2])
    out = np.empty((n, 8, 3), f32)
    for k in range(8):
        s = [1.0 if (k >> j) & 1 else -1.0 for j in range(3)]
        out[:, k] = (c + s[0] * ax[:, 0] + s[1] * ax[:, 1] + s[2] * ax[:, 2]).astype(f32)
    return out


def segments(p, q):
    """Regions collapsed to the segments p q: C0 .. C3 = p, C4 .. C7 = q."""
    p, q = np.asarray(p, f32).reshape(-1, 3), np.asarray(q, f32).reshape(-1, 3)
    return np.concatenate([np.repeat(p[:, None], 4, axis=1), np.repeat(q[:, None], 4, axis=1)], axis=1)


def random_segments(centres, seed, size=0.6):
    rng = np.random.default_rng(seed)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    half = _directions(rng, c.shape[0]) * rng.uniform(0.3, 1.0, (c.shape[0], 1)) * size / 2
    return segments(c - half, c + half)


def aligned_boxes(centres, seed, size=0.3):
    rng = np.random.default_rng(seed)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    half = rng.uniform(0.1, 0.5, c.shape) * size
    return box_corners(c - half, c + half)


def pair_population(kind, n, seed, reach=0.6, edge=0.5):
    """n pairs for the float64 comparisons: a random record (v0, e1, e2 float32, edges of about `edge`) and a region of `kind`
    ("frusta", "boxes", "pyramids", "segments") whose centre lies within `reach` of the record's centroid."""
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-edge / 2, edge / 2, (n, 3, 3))
    tri = tri.astype(f32)
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    off = _directions(rng, n) * (rng.uniform(0, 1, (n, 1)) ** (1 / 3)) * reach
    centres = tri.astype(np.float64).mean(axis=1) + off
    make = {"frusta": frusta, "boxes": sheared_boxes, "pyramids": lambda c, s: frusta(c, s, pyramid=True), "segments": random_segments}[kind]
    return make(centres, seed + 1), v0, e1, e2


def regions_near(rows, n, seed, size=0.5, edges=False):
    """n regions of all five kinds around random finite corners of the scene: most touch something."""
    rng = np.random.default_rng(seed)
    A, B, C = corners(rows, edges)
    fin = np.nonzero(np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1))[0]
    if fin.size:
        centres = A[fin[rng.integers(0, fin.size, n)]].astype(np.float64) + rng.uniform(-size / 2, size / 2, (n, 3))
    else:
        centres = rng.uniform(-1, 1, (n, 3))
    makers = [frusta, sheared_boxes, lambda c, s, size: frusta(c, s, size, pyramid=True), random_segments, aligned_boxes]
    parts = [mk(centres[k::5], seed + 1 + k, size) for k, mk in enumerate(makers) if centres[k::5].shape[0]]
    return queries_of(np.concatenate(parts))


BAD_VALUES = (NAN, INF, -INF)


def bad_queries(query):
    """The regions that accept nothing, made from one good region (32,): each of the 24 coordinates a NaN, +inf and -inf.
    -> (72, 32)."""
    out = np.repeat(np.asarray(query, f32).reshape(1, 32), 72, axis=0)
    for c in range(24):
        for v, bad in enumerate(BAD_VALUES):
            out[3 * c + v, 4 * (c // 3) + c % 3] = bad
    return out


def nan_pads(queries):
    """The same regions with NaNs in the eight pad floats."""
    out = np.array(queries, f32).reshape(-1, 32).copy()
    out[:, 3::4] = NAN
    return out


def mixed_queries(rows, n, seed, edges=False):
    """The device tests' batch of n regions: frusta, sheared boxes, pyramids, segments and aligned boxes around the scene, some
    wide ones, and the non-finite and NaN-pad regions, shuffled together deterministically."""
    rng = np.random.default_rng(seed)
    good = regions_near(rows, 1, seed + 3, edges=edges)[0]
    special = np.concatenate([bad_queries(good)[::5], nan_pads(regions_near(rows, 5, seed + 6, edges=edges))])[:max(n // 4, 0)]
    m = n - special.shape[0]
    wide = regions_near(rows, m // 4, seed + 4, size=4.0, edges=edges)
    rest = regions_near(rows, m - wide.shape[0], seed + 5, edges=edges)
    out = np.concatenate([special, wide, rest])
    assert out.shape == (n, 32)
    return np.ascontiguousarray(out[rng.permutation(n)])
