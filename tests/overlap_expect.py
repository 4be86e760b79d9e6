"""Test side of the region query (rt_tracer_overlap, csrc/rt_overlap.hpp): the triangle and sphere rules of
include/rt_mi355x.h in numpy float32, operation by operation, as a table boxes x prims; the expected rows and counts by brute
force; the traversal restated over a dumped tree, with two switches that break it; an independently written float64
separating-axis test with per-axis margins; and the box populations of the tests.  A helper, not a test.  Everything is
deterministic and needs no device."""
import numpy as np

from query_accel_expect import records_of_rows
from query_expect import cross3 as _cross, dot3 as _dot, tri_rows as _rows
from tree_walk_expect import note_high_water, walk

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)
MAX_HITS = 16                            # RT_MAX_HITS
NONE = -1                                # RT_PRIM_NONE
EPS = 2.0 ** -24
HALF = f32(0.5)
# The restatement against float64: a pair may be left out of the comparison only when, on some axis, the float64 margin (the
# distance by which the axis separates or fails to separate, the axis normalised) is below K * EPS * scale, scale the largest
# |coordinate| of the pair.  K by counting roundings: a projection p = f.y*V.z - f.z*V.y is formed from V = corner - c (the
# corner, c and the difference: three roundings of at most EPS * scale each), f (two), two products and a difference (three
# more, relative), and r likewise; each moves p / |f| by at most EPS * scale, and p and r together make 16.
K = 16.0


def boxes_of(lo, hi):
    """(n, 8) float32 {lo xyz, 0, hi xyz, 0}."""
    lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
    b = np.zeros((lo.shape[0], 8), f32)
    b[:, 0:3], b[:, 4:7] = lo, hi
    return b


def _axes(f, P, Q, h):
    """Step 3 for one edge vector f on the corners P, Q: separated on unit_x x f, unit_y x f or unit_z x f."""
    ax, ay, az = np.abs(f[0]), np.abs(f[1]), np.abs(f[2])
    x, y, z = 0, 1, 2
    sep = False
    for p0, p1, r in ((f[y] * P[z] - f[z] * P[y], f[y] * Q[z] - f[z] * Q[y], h[y] * az + h[z] * ay),
                      (f[z] * P[x] - f[x] * P[z], f[z] * Q[x] - f[x] * Q[z], h[x] * az + h[z] * ax),
                      (f[x] * P[y] - f[y] * P[x], f[x] * Q[y] - f[y] * Q[x], h[x] * ay + h[y] * ax)):
        assert p0.dtype == f32 and r.dtype == f32
        sep = sep | ((p0 > r) & (p1 > r)) | ((p0 < -r) & (p1 < -r))
    return sep


def triangle_rule(boxes, v0, e1, e2, box_step=True):
    """Every box against every record: boxes (N, 8), v0, e1, e2 (T, 3) float32 -> (accepted, step 1) bool (N, T).  The text of
    include/rt_mi355x.h, one float32 operation per operation.  box_step=False: a rule WITHOUT step 1's three box axes (it keeps
    lo <= hi), for the test that shows what step 1 is for."""
    boxes = np.asarray(boxes, f32).reshape(-1, 8)
    v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (v0, e1, e2))
    with np.errstate(all="ignore"):
        L = [boxes[:, k, None] for k in range(3)]
        H = [boxes[:, 4 + k, None] for k in range(3)]
        A = [v0[None, :, k] for k in range(3)]
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        B = [A[k] + E1[k] for k in range(3)]
        C = [A[k] + E2[k] for k in range(3)]
        valid = (L[0] <= H[0]) & (L[1] <= H[1]) & (L[2] <= H[2])
        step1 = np.broadcast_to(valid, (boxes.shape[0], v0.shape[0])).copy()
        for k in range(3):
            mn, mx = np.fmin(np.fmin(A[k], B[k]), C[k]), np.fmax(np.fmax(A[k], B[k]), C[k])
            step1 &= ~(np.isnan(B[k]) | np.isnan(C[k])) & (mn <= H[k]) & (mx >= L[k])
        c = [HALF * L[k] + HALF * H[k] for k in range(3)]
        h = [HALF * H[k] - HALF * L[k] for k in range(3)]
        n = _cross(E1, E2)
        a = [A[k] - c[k] for k in range(3)]
        b = [B[k] - c[k] for k in range(3)]
        cc = [C[k] - c[k] for k in range(3)]
        s = _dot(n, a)
        r = _dot(h, [np.abs(n[0]), np.abs(n[1]), np.abs(n[2])])
        assert s.dtype == f32 and r.dtype == f32
        sep = np.abs(s) > r
        sep = sep | _axes(E1, a, cc, h) | _axes([cc[k] - b[k] for k in range(3)], a, b, h) | _axes([a[k] - cc[k] for k in range(3)], a, b, h)
        acc = (step1 if box_step else np.broadcast_to(valid, step1.shape)) & ~sep
    return acc, step1


def sphere_rule(boxes, spheres):
    """(N, S) bool: the sphere rule, one float32 operation per operation."""
    boxes = np.asarray(boxes, f32).reshape(-1, 8)
    s = np.asarray(spheres, f32).reshape(-1, 4)
    zero = f32(0)
    with np.errstate(all="ignore"):
        a = [boxes[:, k, None] - s[None, :, k] for k in range(3)]
        b = [s[None, :, k] - boxes[:, 4 + k, None] for k in range(3)]
        g = [np.fmax(np.fmax(a[k], b[k]), zero) for k in range(3)]
        f = [np.fmax(np.abs(a[k]), np.abs(b[k])) for k in range(3)]
        d2min, d2max = _dot(g, g), _dot(f, f)
        rr = s[None, :, 3] * s[None, :, 3]
        assert d2min.dtype == f32 and rr.dtype == f32
        valid = (boxes[:, 0:3] <= boxes[:, 4:7]).all(axis=1)[:, None]
        return valid & (d2min <= rr) & (rr <= d2max)


def table(boxes, rows, edges=False, spheres=None, box_step=True, block=512):
    """(N, P) bool, column = prim: the triangles' verdicts, then the spheres'."""
    boxes = np.asarray(boxes, f32).reshape(-1, 8)
    n = boxes.shape[0]
    if rows is None or len(rows) == 0:
        acc = np.zeros((n, 0), bool)
    else:
        rec = records_of_rows(rows, edges)
        acc = np.concatenate([triangle_rule(boxes[i:i + block], *rec, box_step=box_step)[0] for i in range(0, n, block)]) if n else np.zeros((0, rec[0].shape[0]), bool)
    if spheres is not None and len(spheres):
        acc = np.c_[acc, sphere_rule(boxes, spheres)]
    return acc


def rows_of_table(acc, max_hits, after=None):
    """The cursor, the order and the cut on a table -> (prims (n, max_hits) int32, counts (n,) uint32, the TOTAL)."""
    n, P = acc.shape
    acc = acc.copy()
    if after is not None:
        a = np.asarray(after, np.int64).reshape(-1)
        assert a.shape[0] == n
        acc &= (a[:, None] == NONE) | (np.arange(P, dtype=np.int64)[None, :] > a[:, None])
    counts = acc.sum(axis=1).astype(np.uint32)
    prims = np.full((n, max_hits), NONE, np.int32)
    rank = np.cumsum(acc, axis=1) - 1
    i, j = np.nonzero(acc & (rank < max_hits))
    prims[i, rank[i, j]] = j
    return prims, counts


def expected(boxes, rows, max_hits, after=None, edges=False, spheres=None):
    """Brute force -> (prims (n, max_hits) int32, counts (n,) uint32)."""
    return rows_of_table(table(boxes, rows, edges, spheres), max_hits, after)


def accepted_sets(acc):
    return [np.nonzero(r)[0].astype(np.int32) for r in acc]


def chain(query, n, max_hits):
    """Enumerate through the cursor: query(live, after) -> (prims, counts) for the boxes `live`; repeats with after = the row's
    last prim while a count exceeds max_hits.  -> ([int32 (m_i,)] per box, rounds made)."""
    live = np.arange(n)
    after = None
    got = [[] for _ in range(n)]
    made = 0
    while live.size:
        prims, counts = query(live, after)
        made += 1
        for r, i in enumerate(live):
            got[i].append(prims[r, :min(int(counts[r]), max_hits)])
        more = counts > max_hits
        after = np.ascontiguousarray(prims[more, max_hits - 1])
        live = live[more]
    return [np.concatenate(g) if g else np.zeros(0, np.int32) for g in got], made


def same(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() and np.shape(x) == np.shape(y) for x, y in zip(a, b))


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree(nodes, recs, info, acc, bounds, max_hits, after=None, closed=True, stack_cap=None, stats=None):
    """region_bvh_kernel in numpy over a dumped tree (nodes, recs, info of api.bvh_build / query_tree), for every region shape:
    acc is the shape's rule as a table (queries x prims), bounds(i) the bounding box (lo, hi) of query i, or None for a query that
    accepts nothing.  A child is entered when its box and the query's bounding box overlap (closed comparisons, no inflation),
    every record met goes through the rule, then the always-tested list, then the spheres.  Returns (prims, counts, triangle
    tests made).  closed=False enters a child only on STRICT overlap, which breaks it.  stack_cap: the number of entries the
    stack holds (default 3 * depth, which never overflows); a walk that had to drop an entry starts again from every leaf
    record, as the kernel's overflow redo does."""
    n_tris = recs.shape[0]
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    met = np.zeros(acc.shape, bool)
    tests = 0
    cap = 3 * max(info["depth"], 1) if stack_cap is None else stack_cap
    with np.errstate(invalid="ignore"):
        for i in range(acc.shape[0]):
            box = bounds(i)
            if box is None:
                note_high_water(stats, 0)
                continue
            lo, hi = box

            def leaf(k):
                nonlocal tests
                assert not met[i, index[k]]                              # a walk visits every record at most once
                met[i, index[k]] = True
                tests += 1

            def child(nd):                                               # no key decides: the children are entered as stored
                if closed:
                    inn = ((nd["lo"] <= hi[:, None]) & (nd["hi"] >= lo[:, None])).all(axis=0)
                else:
                    inn = ((nd["lo"] < hi[:, None]) & (nd["hi"] > lo[:, None])).all(axis=0)
                return [INF if inn[c] else None for c in range(4)]

            mark, overflow = walk(nodes, cap, True, child, leaf, enforce_cap=stack_cap is None)     # 3 * depth entries always suffice
            note_high_water(stats, mark)
            if overflow:                                                 # from an empty list and count: every leaf record
                met[i, :n_tris] = False
                met[i, index[:n_leaf]] = True
                tests += n_leaf
            met[i, index[n_leaf:]] = True
            tests += n_tris - n_leaf
            met[i, n_tris:] = True                                       # the spheres, after the triangles
    prims, counts = rows_of_table(acc & met, max_hits, after)
    return prims, counts, tests


def walk_tree_overlap(nodes, recs, info, boxes, rows, max_hits, after=None, edges=False, spheres=None, closed=True, box_step=True,
                      stats=None):
    """walk_tree for boxes: the query's bounding box is the box itself, lo <= hi on every axis.  Switches that break one thing
    each, for tests of the tests: closed=False; box_step=False walks with the rule that lacks step 1."""
    boxes = np.asarray(boxes, f32).reshape(-1, 8)

    def bounds(i):
        lo, hi = boxes[i, 0:3], boxes[i, 4:7]
        return (lo, hi) if (lo <= hi).all() else None
    return walk_tree(nodes, recs, info, table(boxes, rows, edges, spheres, box_step=box_step), bounds, max_hits, after, closed,
                     stats=stats)


# ---- float64, written independently ---------------------------------------------------------------------------------------

def sat64(boxes, rows, edges=False):
    """The 13-axis separating-axis test in float64 on the fp32 corners A, fl(A + e1), fl(A + e2) -> (overlap (N, T) bool, margin
    (N, T) float64: the least |signed separation| over the axes, each axis normalised, a degenerate axis left out; scale (N, T):
    the largest |coordinate| of the pair).  separation > 0: the axis separates by that distance; <= 0: it does not."""
    b = np.asarray(boxes, f32).reshape(-1, 8).astype(np.float64)
    v0, e1, e2 = records_of_rows(rows, edges)
    A = v0.astype(np.float64)
    B, C = (v0 + e1).astype(np.float64), (v0 + e2).astype(np.float64)    # the fp32 corners
    c, h = (b[:, 0:3] + b[:, 4:7]) / 2, (b[:, 4:7] - b[:, 0:3]) / 2
    V = np.stack([A, B, C])[:, None, :, :] - c[None, :, None, :]         # (3 corners, N, T, 3)
    hh = h[:, None, :]
    axes = [np.broadcast_to(np.eye(3)[k], (1, A.shape[0], 3)) for k in range(3)]
    axes.append(np.cross(B - A, C - A)[None])
    for f in (B - A, C - B, A - C):
        for k in range(3):
            axes.append(np.cross(np.eye(3)[k], f)[None])
    worst = np.full(V.shape[1:3], -np.inf)
    margin = np.full(V.shape[1:3], np.inf)
    with np.errstate(all="ignore"):
        for ax in axes:
            ln = np.sqrt((ax * ax).sum(-1))
            p = (V * ax[None]).sum(-1)
            r = (hh * np.abs(ax)).sum(-1)
            sep = np.maximum(p.min(axis=0) - r, -p.max(axis=0) - r) / ln
            ok = ln > 0
            ok = np.broadcast_to(ok, sep.shape)
            worst = np.where(ok, np.maximum(worst, sep), worst)
            margin = np.where(ok, np.minimum(margin, np.abs(sep)), margin)
    scale = np.maximum(np.abs(b[:, [0, 1, 2, 4, 5, 6]]).max(axis=1)[:, None], np.maximum(np.abs(A), np.maximum(np.abs(B), np.abs(C))).max(axis=1)[None, :])
    return worst <= 0, margin, scale


# ---- scenes and boxes --------------------------------------------------------------------------------------------------------

def random_scene(n_tris, seed, edge=0.2, span=1.0, snap=None):
    """n_tris triangles of edge about `edge` with centres uniform in [-span, span]^3; snap: every coordinate rounded to a multiple
    of it (a dyadic snap makes touching exact)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-span, span, (n_tris, 1, 3)) + rng.uniform(-edge / 2, edge / 2, (n_tris, 3, 3))
    if snap:
        t = np.round(t / snap) * snap
    return _rows(t)


def corners(rows, edges=False):
    """The fp32 corners A, B, C the rule works on, each (T, 3)."""
    v0, e1, e2 = records_of_rows(rows, edges)
    return v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)


def random_boxes(rows, n, seed, width=0.5, snap=None, edges=False):
    """n boxes of sizes around a triangle's (each extent uniform in (0, width)), centred within a box width of a random corner."""
    rng = np.random.default_rng(seed)
    A, B, C = corners(rows, edges)
    fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1)
    pick = np.nonzero(fin)[0][rng.integers(0, fin.sum(), n)]
    centre = A[pick].astype(np.float64) + rng.uniform(-width, width, (n, 3))
    half = rng.uniform(0, width / 2, (n, 3))
    lo, hi = centre - half, centre + half
    if snap:
        lo, hi = np.floor(lo / snap) * snap, np.ceil(hi / snap) * snap
    return boxes_of(lo, hi)


def touching_boxes(rows, tris, edges=False):
    """For each triangle j of `tris` and each axis: a box around the triangle whose hi on that axis EQUALS the triangle's tmin
    (touching: step 1 accepts), and one whose hi is one ulp below it (step 1 rejects).  -> (boxes, tags [(j, axis, touches)])."""
    A, B, C = corners(rows, edges)
    mn, mx = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
    lo_all, hi_all, tags = [], [], []
    for j in tris:
        for a in range(3):
            for touches in (True, False):
                lo, hi = mn[j] - f32(0.5), mx[j] + f32(0.5)
                hi[a] = mn[j, a] if touches else np.nextafter(mn[j, a], -INF)
                lo[a] = mn[j, a] - f32(1.0)
                lo_all.append(lo), hi_all.append(hi), tags.append((int(j), a, touches))
    return boxes_of(lo_all, hi_all), tags


def point_boxes(rows, tris, edges=False):
    """lo == hi: on vertex A of each triangle of `tris`, and at A + e1/4 + e2/4 -- inside the face, exactly, when the record is
    dyadic with bits to spare."""
    v0, e1, e2 = records_of_rows(rows, edges)
    p = np.concatenate([v0[tris], (v0[tris] + f32(0.25) * e1[tris] + f32(0.25) * e2[tris]).astype(f32)])
    return boxes_of(p, p)


def whole_box(rows, spheres=None, edges=False):
    """The scene's bounds, one box (finite corners only; spheres by centre +- radius)."""
    A, B, C = corners(rows, edges) if rows is not None and len(rows) else (np.zeros((0, 3), f32),) * 3
    pts = [x[np.isfinite(x).all(axis=1)] for x in (A, B, C)]
    if spheres is not None and len(spheres):
        s = np.asarray(spheres, f32).reshape(-1, 4)
        pts += [s[:, :3] - s[:, 3:4], s[:, :3] + s[:, 3:4]]
    p = np.concatenate(pts)
    return boxes_of(p.min(axis=0), p.max(axis=0))


BAD_NAMES = ("inverted_x", "inverted_y", "inverted_z", "nan_lo", "nan_hi", "nan_all", "lo_plus_inf", "hi_minus_inf", "inf_inverted")


def bad_boxes(box):
    """The boxes that accept nothing, made from one good box (8,): inverted on one axis, a NaN bound, and infinite bounds on
    the wrong side (lo = +inf, hi = -inf).  -> (len(BAD_NAMES), 8)."""
    out = np.repeat(np.asarray(box, f32).reshape(1, 8), len(BAD_NAMES), axis=0)
    for a in range(3):
        out[a, a], out[a, 4 + a] = box[4 + a] + f32(1.0), box[a] - f32(1.0)   # (strictly inverted even for a point box)
    out[3, 1] = NAN
    out[4, 6] = NAN
    out[5, [0, 1, 2, 4, 5, 6]] = NAN
    out[6, 0] = INF
    out[7, 5] = -INF
    out[8, 0:3], out[8, 4:7] = INF, -INF
    return out


def nan_pads(boxes):
    """The same boxes with NaNs in the two pad floats."""
    out = np.array(boxes, f32).reshape(-1, 8).copy()
    out[:, 3] = out[:, 7] = NAN
    return out


def unbounded_boxes(box):
    """Infinite bounds on the right side: all of space, and the half spaces below hi.x and above lo.z of `box`.  Steps 2-3 then
    compute with inf and NaN and never separate: what step 1 accepts is accepted."""
    out = np.repeat(np.asarray(box, f32).reshape(1, 8), 3, axis=0)
    out[:, 0:3], out[:, 4:7] = -INF, INF
    out[1, 4] = box[4]
    out[2, 2] = box[2]
    return out


def sphere_boxes(sphere):
    """Around one sphere {centre, radius}: a box wholly inside the ball (touches nothing), one that contains it, one that cuts
    its surface, one that touches it from outside at +x, one beyond it.  -> ((5, 8), expected bool (5,)) for dyadic spheres."""
    s = np.asarray(sphere, f32).reshape(4)
    c, r = s[:3].astype(np.float64), float(s[3])
    e = np.array([1.0, 0.0, 0.0])
    lo = [c - r / 4, c - 2 * r, c + (r / 2) * e - r / 4, c + r * e - [0, r / 4, r / 4], c + 3 * r * e]
    hi = [c + r / 4, c + 2 * r, c + (r / 2) * e + [r, r / 4, r / 4], c + 2 * r * e + [0, r / 4, r / 4], c + 4 * r * e + r / 4]
    return boxes_of(lo, hi), np.array([False, True, True, True, False])
