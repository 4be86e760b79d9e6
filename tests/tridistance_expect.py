"""Test side of the triangle-shaped proximity query (rt_tracer_triangle_distance, csrc/rt_tridistance.hpp): the
rule of include/rt_mi355x.h in numpy float32, operation by operation, as tables queries x prims (t, u, v, the winning candidate
and its point); the expected two arrays by brute force under the point query's winner rule; the traversal restated over a dumped
tree, with two switches that break it; an independently written float64 distance of two triangles; and the populations of the
tests.  A helper, not a test.  Everything is deterministic and needs no device.

The triangle rule of the point query is stated here once more, elementwise on pairs (closest_pairs), because
closest_expect.closest_triangle answers every point against every record and this query asks one point per PAIR;
test_tridistance_expect.py pins the two to each other bit for bit."""
import numpy as np

import closest_expect as ce
import trioverlap_expect as te
from overlap_expect import corners
from query_accel_expect import records_of_rows
from query_expect import HIT_DTYPE, cross3 as _cross, dot3 as _dot
from tree_walk_expect import box_gap_lb, keys_of, note_high_water, walk

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)
ZERO, ONE = f32(0), f32(1)
WITNESS_DTYPE = np.dtype([("x", f32), ("y", f32), ("z", f32), ("where", np.int32)])
N_CANDIDATES = 21
EPS = 2.0 ** -24
# The accuracy statement: sqrt(t) >= D - K eps scale (all pairs), |sqrt(t) - D| <= K eps scale (pairs of two well-shaped
# triangles), scale = qabs + the largest |vertex coordinate| of the scene.  K_MEASURED is the largest K the restatement needs
# against distance64 over accuracy_cases() (test_tridistance_expect.py prints both sides per population); K is 4 x that, rounded
# up to a power of two.
K_MEASURED = 1.983
K = 8.0


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _add(a, b):
    return [a[k] + b[k] for k in range(3)]


def _clamp01(x):
    return np.fmin(np.fmax(x, ZERO), ONE)                                # (a NaN becomes 0)


def _along(g0, s, d):
    return [g0[k] + s * d[k] for k in range(3)]


def _isnan3(x):
    return np.isnan(x[0]) | np.isnan(x[1]) | np.isnan(x[2])


def closest_pairs(p, v0, e1, e2):
    """closest_expect.closest_triangle elementwise: p, v0, e1, e2 lists of three broadcastable float32 arrays -> t, u, v."""
    ap = _sub(p, v0)
    a, b, c = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    d1, d2 = _dot(e1, ap), _dot(e2, ap)
    d3, d4, d5, d6 = d1 - a, d2 - b, d1 - b, d2 - c
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0),
             (d3 >= 0) & (d4 <= d3),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0),
             (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d43 >= 0) & (d56 >= 0)]
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    w = d43 / (d43 + d56)
    den = one / ((va + vb) + vc)
    u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - w], vb * den)
    v = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w], vc * den)
    r = [(ap[k] - u * e1[k]) - v * e2[k] for k in range(3)]
    t = _dot(r, r)
    assert t.dtype == f32 and u.dtype == f32 and v.dtype == f32
    return t, u, v


def _seg_s(g0, d1, a, r0, d2, e):
    """The parameter of the FIRST segment g0 + s*d1 nearest to r0 + t*d2 (Ericson; the header's text)."""
    r = _sub(g0, r0)
    f, c, b = _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    denom = a * e - b * b
    s0 = np.where(denom == 0, ZERO, _clamp01((b * f - c * e) / denom))
    tnom = b * s0 + f
    low = (tnom < 0) | (e == 0)
    redo = low | (tnom > e)
    s1 = _clamp01(np.where(low, -c, b - c) / a)
    s = np.where(a == 0, ZERO, np.where(redo, s1, s0))
    assert s.dtype == f32
    return s


def _plane_s(da, db):
    present = (da * db <= 0) & (da != db)
    return _clamp01(da / (da - db)), present


class _Query:
    """What depends on the query alone, every member a list of three (N, 1) float32 arrays or an (N, 1) array."""

    def __init__(self, queries):
        q = np.asarray(queries, f32).reshape(-1, 12)
        P = te.corners_of(q)
        self.P = [[P[:, i, k, None] for k in range(3)] for i in range(3)]
        self.p1, self.p2 = _sub(self.P[1], self.P[0]), _sub(self.P[2], self.P[0])
        self.d = [self.p1, _sub(self.P[2], self.P[1]), _sub(self.P[0], self.P[2])]
        self.a = [_dot(d, d) for d in self.d]
        self.m = _cross(self.p1, self.p2)
        self.lo = [np.fmin(np.fmin(self.P[0][k], self.P[1][k]), self.P[2][k]) for k in range(3)]
        self.hi = [np.fmax(np.fmax(self.P[0][k], self.P[1][k]), self.P[2][k]) for k in range(3)]
        self.qabs = np.abs(P).reshape(-1, 9).max(axis=1)
        self.d2max = q[:, 3].copy()
        self.active = np.isfinite(P).all(axis=(1, 2)) & (self.d2max >= 0)

    def project(self, y):
        _, u, v = closest_pairs(y, self.P[0], self.p1, self.p2)
        return [(self.P[0][k] + u * self.p1[k]) + v * self.p2[k] for k in range(3)]

    def clamp(self, x):
        return [np.fmin(np.fmax(x[k], self.lo[k]), self.hi[k]) for k in range(3)]


class _Fold:
    """The least t_k so far, equal t to the lowest k; k < 0 = none yet."""

    def __init__(self, shape):
        self.t = np.full(shape, INF, f32)
        self.u, self.v = np.zeros(shape, f32), np.zeros(shape, f32)
        self.x = [np.zeros(shape, f32) for _ in range(3)]
        self.k = np.full(shape, -1, np.int32)

    def take(self, ok, t, u, v, x, k):
        ok = ok & ((t < self.t) | ((self.k < 0) & (t <= self.t)))
        self.t, self.k = np.where(ok, t, self.t), np.where(ok, np.int32(k), self.k)
        if u is not None:
            self.u, self.v = np.where(ok, u, self.u), np.where(ok, v, self.v)
        self.x = [np.where(ok, np.broadcast_to(x[i], ok.shape), self.x[i]) for i in range(3)]

    def done(self):
        self.t = np.where(self.k < 0, NAN, self.t)
        return self


def _triangle_table(Q, v0, e1, e2, only=None):
    """Every query of Q against every record: the fold over the 21 candidates (`only`: a set of candidate indices, for the tests
    that ask what one group of candidates is for)."""
    A = [v0[None, :, k] for k in range(3)]
    E1 = [e1[None, :, k] for k in range(3)]
    E2 = [e2[None, :, k] for k in range(3)]
    B, C = _add(A, E1), _add(A, E2)
    shape = (Q.qabs.shape[0], v0.shape[0])
    F = _Fold(shape)
    yes = np.ones(shape, bool)

    def attempt(x, present, k):
        if only is not None and k not in only:
            return
        x = [np.broadcast_to(c, shape) for c in x]
        ok = present & ~_isnan3(x)
        xc = Q.clamp(x)
        t, u, v = closest_pairs(xc, A, E1, E2)
        F.take(ok, t, u, v, xc, k)

    for i in range(3):
        attempt(Q.P[i], yes, i)
    for i, Y in enumerate((A, B, C)):
        attempt(Q.project(Y), yes, 3 + i)
    R = [A, B, C]
    dr = [_sub(B, A), _sub(C, B), _sub(A, C)]
    for i in range(3):
        e = _dot(dr[i], dr[i])
        for j in range(3):
            attempt(_along(Q.P[j], _seg_s(Q.P[j], Q.d[j], Q.a[j], R[i], dr[i], e), Q.d[j]), yes, 6 + 3 * i + j)
    n = _cross(E1, E2)
    dq = [_dot(n, _sub(Q.P[j], A)) for j in range(3)]
    for j in range(3):
        s, present = _plane_s(dq[j], dq[(j + 1) % 3])
        attempt(_along(Q.P[j], s, Q.d[j]), present, 15 + j)
    dp = [_dot(Q.m, _sub(R[i], Q.P[0])) for i in range(3)]
    for i in range(3):
        s, present = _plane_s(dp[i], dp[(i + 1) % 3])
        attempt(Q.project(_along(R[i], s, dr[i])), present, 18 + i)
    return F.done()


def _sphere_table(Q, queries, spheres):
    s = np.asarray(spheres, f32).reshape(-1, 4)
    S = [s[None, :, k] for k in range(3)]
    rad = s[None, :, 3]
    shape = (Q.qabs.shape[0], s.shape[0])
    F = _Fold(shape)
    for k, x in enumerate([Q.P[0], Q.P[1], Q.P[2], Q.project(S)]):
        x = [np.broadcast_to(c, shape) for c in x]
        ok = ~_isnan3(x)
        xc = Q.clamp(x)
        w = _sub(xc, S)
        d = np.abs(np.sqrt(_dot(w, w)) - rad)
        F.take(ok, d * d, None, None, xc, k)
    F.done()
    touching = te.sphere_rule(queries, spheres)
    F.t = np.where((F.k >= 0) & touching, ZERO, F.t)
    return F


def table(queries, rows, edges=False, spheres=None, only=None, chunk=400000):
    """The pairs' answers, column = prim (the triangles, then the spheres): dict t, u, v (N, P) float32, where (N, P) int32, x
    (N, P, 3) float32.  A query that accepts nothing has NaN in every t."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    n = queries.shape[0]
    n_tris = 0 if rows is None or len(rows) == 0 else np.asarray(rows).reshape(-1, 4).shape[0] // 3
    n_sph = 0 if spheres is None else len(spheres)
    out = {"t": np.full((n, n_tris + n_sph), NAN, f32), "u": np.zeros((n, n_tris + n_sph), f32), "v": np.zeros((n, n_tris + n_sph), f32),
           "where": np.full((n, n_tris + n_sph), -1, np.int32), "x": np.zeros((n, n_tris + n_sph, 3), f32)}
    rec = records_of_rows(rows, edges) if n_tris else None
    step = max(1, chunk // max(n_tris + n_sph, 1))
    with np.errstate(all="ignore"):
        for i0 in range(0, n, step):
            sl = slice(i0, min(i0 + step, n))
            Q = _Query(queries[sl])
            parts = []
            if n_tris:
                parts.append(_triangle_table(Q, *rec, only=only))
            if n_sph:
                parts.append(_sphere_table(Q, queries[sl], spheres))
            c0 = 0
            for F in parts:
                c1 = c0 + F.t.shape[1]
                out["t"][sl, c0:c1] = np.where(Q.active[:, None], F.t, NAN)
                out["u"][sl, c0:c1], out["v"][sl, c0:c1], out["where"][sl, c0:c1] = F.u, F.v, F.k
                for k in range(3):
                    out["x"][sl, c0:c1, k] = F.x[k]
                c0 = c1
    return out


def winners(tab, d2max):
    """The point query's winner rule on a table -> (HIT_DTYPE (n,), WITNESS_DTYPE (n,))."""
    hits = ce.winners((tab["t"], tab["u"], tab["v"], None), d2max)
    wit = np.zeros(hits.shape[0], WITNESS_DTYPE)
    wit["where"] = -1
    ok = hits["prim"] >= 0
    i, j = np.nonzero(ok)[0], hits["prim"][ok]
    wit["x"][ok], wit["y"][ok], wit["z"][ok] = tab["x"][i, j, 0], tab["x"][i, j, 1], tab["x"][i, j, 2]
    wit["where"][ok] = tab["where"][i, j]
    return hits, wit


def expected(queries, rows, edges=False, spheres=None):
    """Brute force: queries (n, 12) -> (HIT_DTYPE (n,), WITNESS_DTYPE (n,))."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    return winners(table(queries, rows, edges, spheres), queries[:, 3])


def same(a, b):
    """Two (hits, witness) pairs, byte for byte."""
    return all(np.ascontiguousarray(x).view(np.uint32).tobytes() == np.ascontiguousarray(y).view(np.uint32).tobytes() for x, y in zip(a, b))


def differing(a, b):
    """The rows in which two (hits, witness) pairs differ."""
    d = np.zeros(np.asarray(a[0]).reshape(-1).shape[0], bool)
    for x, y in zip(a, b):
        d |= (np.ascontiguousarray(x).view(np.uint32).reshape(-1, 4) != np.ascontiguousarray(y).view(np.uint32).reshape(-1, 4)).any(axis=1)
    return np.nonzero(d)[0]


def with_radius(queries, d2max):
    """The same (n, 12) queries with d2max (a scalar or (n,)) in column 3."""
    q = np.array(queries, f32).reshape(-1, 12).copy()
    q[:, 3] = np.asarray(d2max, f32)
    return q


def radius_families(queries, rows, edges=False, spheres=None, tab=None):
    """The five d2max of the tests as {name: (n, 12)}: inf, the median of the unbounded answers' t, 0, NaN, -1."""
    tab = table(queries, rows, edges, spheres) if tab is None else tab
    t = winners(tab, INF)[0]
    fin = t["t"][(t["prim"] >= 0) & np.isfinite(t["t"])]
    half = f32(np.median(fin)) if fin.size else f32(1.0)
    return {"inf": with_radius(queries, INF), "half": with_radius(queries, half), "zero": with_radius(queries, 0.0),
            "nan": with_radius(queries, np.nan), "negative": with_radius(queries, -1.0)}


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_tridistance(nodes, recs, info, queries, rows, edges=False, spheres=None, rho_c=ce.RHO_C, tie_rule=True, strict=True,
                          stats=None, tab=None):
    """tridistance_bvh_kernel in numpy: the fp32 box bound of csrc/rt_tridistance.hpp operation by operation over a dumped tree
    (nodes, recs, info of api.bvh_build / query_tree), the order-free winner rule, the pairs' answers looked up in table().
    Returns ((hits, witness), triangle tests made).  Switches that break one rule each, for tests of the tests: strict=False
    skips a child at lb >= best and drops a popped entry at lb >= best; tie_rule=False lets the first visited keep a tie."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    tab = table(queries, rows, edges, spheres) if tab is None else tab
    T = tab["t"]
    P = te.corners_of(queries)
    n_tris = recs.shape[0]
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    hits = np.zeros(queries.shape[0], HIT_DTYPE)
    wit = np.zeros(queries.shape[0], WITNESS_DTYPE)
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(queries.shape[0]):
            d2max = queries[i, 3]
            hits[i], wit[i] = (0, 0, 0, -1), (0, 0, 0, -1)
            if not (d2max >= 0 and np.isfinite(P[i]).all()):             # accepts nothing
                note_high_water(stats, 0)
                continue
            state = {"t": d2max, "i": -1}

            def keep(tj, j):
                if tj < state["t"] or (tj == state["t"] and (state["i"] < 0 or (tie_rule and j < state["i"]))):
                    state.update(t=tj, i=int(j))

            qmin = np.fmin(np.fmin(P[i, 0], P[i, 1]), P[i, 2])
            qmax = np.fmax(np.fmax(P[i, 0], P[i, 1]), P[i, 2])
            qabs = np.abs(P[i]).max()

            def stale(g):
                return (g < -state["t"]) if strict else (g <= -state["t"])

            def leaf(k):
                nonlocal tests
                tests += 1
                keep(T[i, index[k]], index[k])

            def child(nd):                                               # skipped where its entry would be stale at once
                lb = box_gap_lb(nd, qmin, qmax, qabs, rho_c)
                return keys_of(-lb, ~np.isnan(lb), stale(-lb))

            mark, _ = walk(nodes, cap, True, child, leaf, stale)
            note_high_water(stats, mark)
            for j in index[n_leaf:]:
                tests += 1
                keep(T[i, j], j)
            for s in range(n_tris, T.shape[1]):                          # the spheres, after the triangles
                keep(T[i, s], s)
            j = state["i"]
            if j >= 0:
                hits[i] = (state["t"], tab["u"][i, j], tab["v"][i, j], j)
                wit[i] = (tab["x"][i, j, 0], tab["x"][i, j, 1], tab["x"][i, j, 2], tab["where"][i, j])
    return (hits, wit), tests


# ---- float64, written independently ---------------------------------------------------------------------------------------

def _point_segment64(p, a, b):
    ab = b - a
    ll = (ab * ab).sum(-1)
    with np.errstate(all="ignore"):
        s = np.where(ll > 0, ((p - a) * ab).sum(-1) / np.where(ll > 0, ll, 1.0), 0.0)
    d = p - (a + np.clip(s, 0.0, 1.0)[..., None] * ab)
    return np.sqrt((d * d).sum(-1))


def _segment_segment64(a0, a1, b0, b1):
    """Two segments' distance without clamping logic: where the lines' common perpendicular meets both segments inside, its
    length; otherwise the least of the four end point to segment distances."""
    u, v, w = a1 - a0, b1 - b0, a0 - b0
    uu, uv, vv, uw, vw = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1), (u * w).sum(-1), (v * w).sum(-1)
    det = uu * vv - uv * uv
    with np.errstate(all="ignore"):
        s = (uv * vw - vv * uw) / det
        t = (uu * vw - uv * uw) / det
        inner = (det > 1e-30 * uu * vv) & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
        dd = w + np.where(inner, s, 0.0)[..., None] * u - np.where(inner, t, 0.0)[..., None] * v
        line = np.sqrt((dd * dd).sum(-1))
    ends = np.minimum(np.minimum(_point_segment64(a0, b0, b1), _point_segment64(a1, b0, b1)),
                      np.minimum(_point_segment64(b0, a0, a1), _point_segment64(b1, a0, a1)))
    return np.where(inner, np.minimum(line, ends), ends)


def _point_triangle64(p, T):
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    d = np.minimum(np.minimum(_point_segment64(p, a, b), _point_segment64(p, b, c)), _point_segment64(p, c, a))
    e1, e2 = b - a, c - a
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    ap = p - a
    with np.errstate(all="ignore"):
        s = (np.cross(ap, e2) * n).sum(-1) / nn
        t = (np.cross(e1, ap) * n).sum(-1) / nn
        inside = (nn > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
        plane = np.abs((ap * n).sum(-1)) / np.sqrt(nn)
    return np.where(inside, np.minimum(d, plane), d)


def distance64(Q, R):
    """(m,) float64 distances of the triangle pairs Q, R (m, 3, 3) (fp32 corners taken to float64): the least of nine
    segment-segment and six point-triangle distances, 0 where an edge of one passes through the other."""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    d = np.full(Q.shape[0], np.inf)
    hit = np.zeros(Q.shape[0], bool)
    E = ((0, 1), (1, 2), (2, 0))
    for a, b in E:
        for c, e in E:
            d = np.minimum(d, _segment_segment64(Q[:, a], Q[:, b], R[:, c], R[:, e]))
        hit |= te._segment_hits64(Q[:, a], Q[:, b], R) | te._segment_hits64(R[:, a], R[:, b], Q)
    for i in range(3):
        d = np.minimum(d, np.minimum(_point_triangle64(Q[:, i], R), _point_triangle64(R[:, i], Q)))
    return np.where(hit, 0.0, d)


def scene_corners(rows, edges=False):
    """(T, 3, 3) float32: the corners A, B, C the rule reads."""
    return np.stack(corners(rows, edges), axis=1)


def well_shaped_queries(queries):
    rows = np.zeros((np.asarray(queries).reshape(-1, 12).shape[0], 3, 4), f32)
    rows[:, :, :3] = te.corners_of(queries)
    return ce.well_shaped(rows.reshape(-1, 4))


def accuracy_sides(queries, rows, edges=False):
    """The accuracy statement per pair in units of eps * scale, every query against every record: (D - sqrt(t), |sqrt(t) - D|
    where both triangles are well shaped else NaN), each (N, T)."""
    queries = np.asarray(queries, f32).reshape(-1, 12)
    tab = table(queries, rows, edges)
    Qc, Rc = te.corners_of(queries), scene_corners(rows, edges)
    n, m = Qc.shape[0], Rc.shape[0]
    i, j = np.divmod(np.arange(n * m), m)
    D = distance64(Qc[i], Rc[j]).reshape(n, m)
    scale = (np.abs(Qc.astype(np.float64)).reshape(n, -1).max(axis=1) + np.abs(Rc.astype(np.float64)).max())[:, None]
    dist = np.sqrt(tab["t"].astype(np.float64))
    lower = (D - dist) / (EPS * scale)
    ws = well_shaped_queries(queries)[:, None] & ce.well_shaped(rows, edges)[None, :]
    both = np.where(ws, np.abs(dist - D) / (EPS * scale), np.nan)
    return lower, both, ws


# ---- populations ----------------------------------------------------------------------------------------------------------------

def near_queries(rows, n, seed, edge=0.6, gap=(1e-4, 0.3), edges=False):
    """n query triangles of edge about `edge` whose centres sit `gap` (log-uniform) off a random point of a random scene
    triangle: near-touching pairs, most of them edge against edge or corner against face."""
    rng = np.random.default_rng(seed)
    Rc = scene_corners(rows, edges).astype(np.float64)
    fin = np.nonzero(np.isfinite(Rc).all(axis=(1, 2)))[0]
    k = fin[rng.integers(0, fin.size, n)]
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    base = Rc[k, 0] + a[:, None] * (Rc[k, 1] - Rc[k, 0]) + b[:, None] * (Rc[k, 2] - Rc[k, 0])
    dirn = rng.normal(0, 1, (n, 3))
    dirn /= np.linalg.norm(dirn, axis=1)[:, None]
    off = 10.0 ** rng.uniform(np.log10(gap[0]), np.log10(gap[1]), n)
    c = base + dirn * (off + edge * 0.4)[:, None]
    return te.queries_of(c[:, None, :] + rng.uniform(-edge / 2, edge / 2, (n, 3, 3)))


def crossing_queries(rows, n, seed, edge=0.6, edges=False):
    """n query triangles around a random interior point of a random scene triangle: most of them intersect it."""
    rng = np.random.default_rng(seed)
    Rc = scene_corners(rows, edges).astype(np.float64)
    fin = np.nonzero(np.isfinite(Rc).all(axis=(1, 2)))[0]
    k = fin[rng.integers(0, fin.size, n)]
    c = Rc[k].mean(axis=1)
    return te.queries_of(c[:, None, :] + rng.uniform(-edge / 2, edge / 2, (n, 3, 3)))


def parallel_queries(rows, tris, edges=False):
    """For each listed record: the record moved along its normal by 1/4 (parallel, face against face), its reflection over BC
    moved likewise, the record moved by half of e1 in its own plane (coplanar and crossing), by three e1 (coplanar and apart), the
    record itself, and the segment B C as a needle."""
    Rc = scene_corners(rows, edges)
    out = []
    for j in tris:
        a, b, c = Rc[j]
        e1 = b - a
        n = np.cross(e1.astype(np.float64), (c - a).astype(np.float64))
        n = (n / np.linalg.norm(n) * 0.25).astype(f32)
        out += [[a + n, b + n, c + n], [b + n, c + n, (b + c) - a + n], [a + f32(0.5) * e1, b + f32(0.5) * e1, c + f32(0.5) * e1],
                [a + f32(3) * e1, b + f32(3) * e1, c + f32(3) * e1], [a, b, c], [b, c, c]]
    return te.queries_of(out)


def point_queries(points):
    """Queries collapsed to the points (m, 3)."""
    p = np.asarray(points, f32).reshape(-1, 3)
    return te.queries_of(np.repeat(p[:, None, :], 3, axis=1))


def populations(rows, seed, n=48, edges=False):
    """{name: (n', 12) queries, d2max = +inf} around one scene: general position, near-touching, intersecting, parallel and
    coplanar, much larger and much smaller than the records, and collapsed to points."""
    fin = np.nonzero(np.isfinite(scene_corners(rows, edges)).all(axis=(1, 2)))[0]
    some = fin[:: max(1, fin.size // 6)][:6]
    out = {"general": te.random_queries(n, seed, edge=0.6, span=3.0), "near": near_queries(rows, n, seed + 1, edges=edges),
           "crossing": crossing_queries(rows, n, seed + 2, edges=edges), "parallel": parallel_queries(rows, some, edges),
           "large": near_queries(rows, n // 2, seed + 3, edge=8.0, edges=edges), "small": near_queries(rows, n // 2, seed + 4, edge=0.01, edges=edges),
           "points": point_queries(ce.points_for(rows, n // 2, seed + 5, edges))}
    return {k: with_radius(v, INF) for k, v in out.items()}


def mixed_queries(rows, n, seed, edges=False):
    """The device tests' batch of n queries, d2max = +inf: the populations above in equal parts, trioverlap_expect's special
    queries (shared corners and edges, coplanar neighbours, non-finite corners, NaN pads), shuffled deterministically."""
    rng = np.random.default_rng(seed)
    special = te.mixed_queries(rows, max(n // 4, 1), seed + 10, edges)
    m = n - special.shape[0]
    per = m // 5
    parts = [special, te.random_queries(per, seed, edge=0.6, span=3.0), near_queries(rows, per, seed + 1, edges=edges),
             crossing_queries(rows, per, seed + 2, edges=edges), near_queries(rows, per, seed + 3, edge=4.0, edges=edges)]
    parts.append(near_queries(rows, n - sum(p.shape[0] for p in parts), seed + 4, edge=0.05, edges=edges))
    out = with_radius(np.concatenate(parts), INF)
    out[:, [7, 11]] = np.where(rng.uniform(0, 1, (n, 2)) < 0.25, NAN, f32(0))     # the pads that are never read
    assert out.shape == (n, 12)
    return np.ascontiguousarray(out[rng.permutation(n)])


def accuracy_cases():
    """{name: (rows, queries)} of the accuracy measurement: general position, 1000 from the origin on either side, intersecting."""
    out = {}
    for name, seed, off in (("random", 61, (0.0, 0.0, 0.0)), ("plus1000", 62, (1000.0, 1000.0, 1000.0)), ("minus1000", 63, (-1000.0, 250.0, -1000.0))):
        rows = ce.random_scene(60, seed, offset=off)
        q = np.concatenate([near_queries(rows, 60, seed + 100, gap=(1e-3, 1.0)), crossing_queries(rows, 20, seed + 200, edge=3.0)])
        out[name] = (rows, with_radius(q, INF))
    rows = ce.random_scene(60, 64)
    out["crossing"] = (rows, with_radius(crossing_queries(rows, 80, 264), INF))
    return out


def lattice_queries(n=4):
    """Query triangles of lattice_cases.rooms(n) that many records tie for, in small dyadic numbers: triangles lying in lattice
    faces (t = 0 against every coplanar triangle they touch), needles along lattice edges, triangles 1/4 and 1/2 off a wall
    (equal positive t against both triangles of a quad and against neighbouring quads), and the lattice points themselves."""
    from lattice_cases import SHIFT
    out = []
    g = np.arange(n, dtype=np.float64)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for i in range(n + 1):
            for j in g[: max(n - 1, 1)]:
                for off in (0.0, 0.25, 0.5):
                    if i + off > n:
                        continue
                    t = np.zeros((3, 3))
                    t[:, a] = i + off
                    t[0, b], t[0, c] = j + 0.25, j + 0.25                # inside one quad, straddling its diagonal
                    t[1, b], t[1, c] = j + 0.75, j + 0.25
                    t[2, b], t[2, c] = j + 0.25, j + 0.75
                    out.append(t)
                    w = t.copy()                                         # across the lattice edge into the next quad
                    w[1, b] = j + 1.25
                    out.append(w)
                e = np.zeros((3, 3))                                     # a needle along a lattice edge
                e[:, a] = [j, j + 1.0, j + 1.0]
                e[:, b], e[:, c] = i, j
                out.append(e)
    q = te.queries_of(np.asarray(out) - SHIFT)
    return with_radius(np.concatenate([q, point_queries(ce.lattice_points(n))]), INF)
