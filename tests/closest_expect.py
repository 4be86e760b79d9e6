"""Test side of the point query (rt_tracer_closest_point, csrc/rt_closest.hpp): the triangle and sphere
arithmetic of include/rt_mi355x.h in numpy float32, operation by operation; the expected answer by brute force under the winner
rule; an independently written float64 distance (the least of the three segment distances and the in-triangle plane distance);
the traversal restated over a dumped tree; and the point populations of the tests.  A helper, not a test.  Everything is
deterministic and needs no device."""
import numpy as np

from query_accel_expect import records_of_rows
from query_expect import HIT_DTYPE, dot3 as _dot, tri_rows as _rows
from tree_walk_expect import DEFLATE, box_gap_lb, keys_of, note_high_water, walk  # noqa: F401  (DEFLATE: re-exported)

f32 = np.float32
INF = f32(np.inf)
RHO_C = f32(2.0 ** -18)                 # RT_CLOSEST_RHO (csrc/rt_kernels.hpp)
EPS = 2.0 ** -24
WELL_SHAPED = 2.0 ** -6                 # smallest corner-angle sine of a well-shaped triangle
# The accuracy statement: sqrt(t) >= D - K eps scale (all triangles), sqrt(t) <= D_ws + K eps scale (well-shaped ones), with
# scale = max|p| + the largest |vertex coordinate|.  K_MEASURED is the largest K the restatement below needs against
# distance64 over accuracy_cases() (test_closest_expect.py prints both sides per population: lower side 1.14, upper side 14.29,
# both in the scene in general position, whose thinnest well-shaped triangles sit just above the shape bound); K is 4 x that,
# rounded up to a power of two.
K_MEASURED = 14.29
K = 64.0


def closest_triangle(p, v0, e1, e2):
    """Every point against every record: p (P, 3), v0, e1, e2 (T, 3) float32 -> t, u, v (float32) and the region 1..7, each
    (P, T).  The text of include/rt_mi355x.h, one float32 operation per operation."""
    p, v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (p, v0, e1, e2))
    with np.errstate(all="ignore"):
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        ap = [p[:, k, None] - v0[None, :, k] for k in range(3)]
        a, b, c = _dot(E1, E1), _dot(E1, E2), _dot(E2, E2)
        d1, d2 = _dot(E1, ap), _dot(E2, ap)
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
        region = np.select(conds, [1, 2, 3, 4, 5, 6], 7)
        r = [(ap[k] - u * E1[k]) - v * E2[k] for k in range(3)]
        t = _dot(r, r)
    assert t.dtype == f32 and u.dtype == f32 and v.dtype == f32
    return t, u, v, region


def closest_sphere(p, spheres):
    """t (P, S) float32 of every point against every sphere {centre, radius}: s = |sqrt(w.w) - radius|, t = s*s."""
    p = np.asarray(p, f32).reshape(-1, 3)
    s = np.asarray(spheres, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = [p[:, k, None] - s[None, :, k] for k in range(3)]
        d = np.abs(np.sqrt(_dot(w, w)) - s[None, :, 3])
        t = d * d
    assert t.dtype == f32
    return t


def table(pts, rows, edges=False, spheres=None):
    """(t, u, v, region) of closest_triangle for the points' xyz against the scene's records, the spheres' t (u = v = 0, region 0)
    appended as further columns: column = prim."""
    pts = np.asarray(pts, f32).reshape(-1, np.shape(pts)[-1])
    n = pts.shape[0]
    if rows is None or len(rows) == 0:
        t, u, v, reg = (np.zeros((n, 0), f32), np.zeros((n, 0), f32), np.zeros((n, 0), f32), np.zeros((n, 0), np.int64))
    else:
        t, u, v, reg = closest_triangle(pts[:, :3], *records_of_rows(rows, edges))
    if spheres is not None and len(spheres):
        ts = closest_sphere(pts[:, :3], spheres)
        z = np.zeros_like(ts)
        t, u, v, reg = np.c_[t, ts], np.c_[u, z], np.c_[v, z], np.c_[reg, z.astype(np.int64)]
    return t, u, v, reg


def winners(tab, d2max):
    """The winner rule on a table: accepted when t <= d2max (plain fp32; a NaN on either side never), the smallest (t, prim).
    -> HIT_DTYPE (n,)."""
    t, u, v, _ = tab
    d2max = np.broadcast_to(np.asarray(d2max, f32), (t.shape[0],))
    out = np.zeros(t.shape[0], HIT_DTYPE)
    out["prim"] = -1
    if t.shape[1] == 0:
        return out
    with np.errstate(invalid="ignore"):
        acc = t <= d2max[:, None]
    idx = np.argmin(np.where(acc, t, INF), axis=1)                   # the first of the smallest
    rows_ = np.arange(t.shape[0])
    first_acc = np.argmax(acc, axis=1)                                # (every accepted t is +inf when the least is unaccepted)
    idx = np.where(acc[rows_, idx], idx, first_acc)
    ok = acc.any(axis=1)
    out["t"][ok], out["u"][ok], out["v"][ok], out["prim"][ok] = t[rows_, idx][ok], u[rows_, idx][ok], v[rows_, idx][ok], idx[ok]
    return out


def expected(pts, rows, edges=False, spheres=None):
    """Brute force: pts (n, 4) {x, y, z, d2max} -> HIT_DTYPE (n,)."""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    return winners(table(pts, rows, edges, spheres), pts[:, 3])


def same_hits(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def differing(a, b):
    return np.nonzero((np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4) != np.ascontiguousarray(b).view(np.uint32).reshape(-1, 4)).any(axis=1))[0]


# ---- float64, written independently ---------------------------------------------------------------------------------------

def _segment64(p, a, b):
    ab = b - a
    ll = (ab * ab).sum(-1)
    with np.errstate(all="ignore"):
        s = np.where(ll > 0, ((p - a) * ab).sum(-1) / np.where(ll > 0, ll, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    d = p - (a + s[..., None] * ab)
    return np.sqrt((d * d).sum(-1))


def distance64(p, rows, edges=False):
    """(P, T) float64 distances from the points to the triangles of the records: the least of the three segment distances and,
    where the point's projection falls inside the triangle, its distance from the plane."""
    v0, e1, e2 = (x.astype(np.float64)[None, :, :] for x in records_of_rows(rows, edges))
    p = np.asarray(p, np.float64).reshape(-1, 3)[:, None, :]
    A, B, Cc = v0, v0 + e1, v0 + e2
    d = np.minimum(np.minimum(_segment64(p, A, B), _segment64(p, B, Cc)), _segment64(p, Cc, A))
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    ap = p - A
    with np.errstate(all="ignore"):
        # barycentrics of the projection: solve [e1 e2] (s, t) = ap in the plane
        s = (np.cross(ap, e2) * n).sum(-1) / nn
        t = (np.cross(e1, ap) * n).sum(-1) / nn
        inside = (nn > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
        plane = np.abs((ap * n).sum(-1)) / np.sqrt(nn)
    return np.where(inside, np.minimum(d, plane), d)


def well_shaped(rows, edges=False):
    """(T,) bool: the smallest corner-angle sine of the record's triangle is >= WELL_SHAPED, in float64."""
    _, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows, edges))
    e3 = e2 - e1
    with np.errstate(all="ignore"):
        def sine(a, b):
            return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        s = np.minimum(np.minimum(sine(e1, e2), sine(e1, e3)), sine(e2, e3))
    return s >= WELL_SHAPED                                              # (a NaN sine, a zero edge, is not well shaped)


def accuracy_sides(pts, rows, edges=False):
    """The two sides of the accuracy statement in units of eps * scale, per point: (D - sqrt(t), sqrt(t) - D_ws), t the
    restatement's winner without a radius.  NaN on the upper side where the scene has no well-shaped triangle."""
    pts = np.asarray(pts, f32).reshape(-1, np.shape(pts)[-1])[:, :3]
    got = winners(table(pts, rows, edges), INF)
    assert (got["prim"] >= 0).all()
    D = distance64(pts, rows, edges)
    ws = well_shaped(rows, edges)
    v0, e1, e2 = records_of_rows(rows, edges)
    vmax = max(np.abs(v0.astype(np.float64)).max(), np.abs(v0.astype(np.float64) + e1).max(), np.abs(v0.astype(np.float64) + e2).max())
    scale = np.abs(pts.astype(np.float64)).max(axis=1) + vmax
    dist = np.sqrt(got["t"].astype(np.float64))
    lower = (D.min(axis=1) - dist) / (EPS * scale)
    upper = (dist - D[:, ws].min(axis=1)) / (EPS * scale) if ws.any() else np.full(pts.shape[0], np.nan)
    return lower, upper


# ---- scenes and points ----------------------------------------------------------------------------------------------------

def random_scene(n_tris, seed, offset=(0.0, 0.0, 0.0), size=0.6):
    """n_tris triangles in general position, centres uniform in [-3, 3]^3 + offset."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, (n_tris, 1, 3)) + np.asarray(offset, np.float64)
    return _rows(c + rng.uniform(-size, size, (n_tris, 3, 3)))


def sliver_scene(n_tris, seed):
    """Random triangles of which every second is a sliver: its third vertex within 10^-3 .. 10^-7 of its first edge."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, (n_tris, 1, 3))
    t = c + rng.uniform(-0.6, 0.6, (n_tris, 3, 3))
    s = rng.uniform(0, 1, (n_tris, 1))
    off = rng.normal(0, 1, (n_tris, 3)) * 10.0 ** rng.uniform(-7, -3, (n_tris, 1))
    sl = np.arange(n_tris) % 2 == 1
    t[sl, 2] = (t[sl, 0] + s[sl] * (t[sl, 1] - t[sl, 0])) + off[sl]
    return _rows(t)


def degenerate_scene():
    """Zero-area triangles among a few ordinary ones: e1 = 0, e2 = 0, e1 parallel to e2 (both senses), all three vertices equal."""
    base = random_scene(6, 41).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    a = np.array([0.25, -0.5, -2.0])
    d = np.array([1.0, 0.5, -0.25])
    extra = [[a, a, a + d], [a + 1, a + 1 + d, a + 1], [a - 1, a - 1 + d, a - 1 + 2 * d], [a + 2, a + 2 + d, a + 2 - d], [a, a, a]]
    return _rows(np.concatenate([base[:3], np.asarray(extra), base[3:]]))


def points_for(rows, n, seed, edges=False, spread=40.0):
    """(n, 3) float32: the first half on or near the surfaces (a random point of a random triangle, jittered by up to 10^-1 ..
    10^-6 of its size or not at all, one in sixteen exactly its first vertex), the second half far away (uniform in a box `spread` times the scene's)."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows, edges))
    near = n - n // 2
    k = rng.integers(0, v0.shape[0], near)
    a, b = rng.uniform(0, 1, near), rng.uniform(0, 1, near)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    corner = rng.uniform(0, 1, near) < 0.0625                            # exactly the record's v0: t == 0 in fp32
    a, b = np.where(corner, 0.0, a), np.where(corner, 0.0, b)
    q = v0[k] + a[:, None] * e1[k] + b[:, None] * e2[k]
    amp = np.where(corner | (rng.uniform(0, 1, near) < 0.25), 0.0, 10.0 ** rng.uniform(-6, -1, near))
    q = q + rng.normal(0, 1, (near, 3)) * amp[:, None]
    fin = np.isfinite(v0).all(axis=1)
    lo, hi = v0[fin].min(axis=0), v0[fin].max(axis=0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    far = mid + rng.uniform(-1, 1, (n // 2, 3)) * half * spread
    pts = np.concatenate([q, far]).astype(f32)
    return np.ascontiguousarray(pts[rng.permutation(n)])


def with_radius(pts, d2max):
    """(n, 4) float32 {x, y, z, d2max}; d2max a scalar or (n,)."""
    p = np.asarray(pts, f32).reshape(-1, np.shape(pts)[-1])
    out = np.empty((p.shape[0], 4), f32)
    out[:, :3], out[:, 3] = p[:, :3], np.asarray(d2max, f32)
    return out


def radius_families(pts, rows, edges=False, spheres=None):
    """The five d2max of the tests as {name: (n, 4)}: inf, the median of the unbounded answers' t (cuts about half), 0, NaN, -1."""
    t = expected(with_radius(pts, INF), rows, edges, spheres)["t"]
    fin = t[np.isfinite(t)]
    half = f32(np.median(fin)) if fin.size else f32(1.0)
    return {"inf": with_radius(pts, INF), "half": with_radius(pts, half), "zero": with_radius(pts, 0.0),
            "nan": with_radius(pts, np.nan), "negative": with_radius(pts, -1.0)}


def accuracy_cases():
    """{name: (rows, points)} of the accuracy measurement: general position, slivers, and scenes 1000 from the origin on either
    side."""
    out = {}
    for name, rows in (("random", random_scene(300, 51)), ("slivers", sliver_scene(300, 52)),
                       ("plus1000", random_scene(300, 53, offset=(1000.0, 1000.0, 1000.0))),
                       ("minus1000", random_scene(300, 54, offset=(-1000.0, 250.0, -1000.0)))):
        out[name] = (rows, points_for(rows, 2000, 55, spread=3.0))
    return out


def lattice_points(n=4):
    """Points of lattice_cases.rooms(n) that several coplanar or adjacent triangles are exactly equidistant from, (m, 3)
    float32 in small dyadic numbers: the lattice vertices and edge midpoints (distance 0 to triangles of several leaves), the
    face centres (on the diagonal both triangles of a quad share), the cell centres (1/2 from the diagonals of six quads) and
    points 1/4 and 1/8 off a wall above a quad's diagonal midpoint."""
    from lattice_cases import SHIFT
    g = np.arange(n + 1, dtype=np.float64)
    half = np.arange(n, dtype=np.float64) + 0.5
    pts = [np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)]                       # vertices
    for a in range(3):                                                                              # edge midpoints, face centres
        ax = [g, g, g]
        ax[a] = half
        pts.append(np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3))
        ax = [half, half, half]
        ax[a] = g
        face = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
        pts.append(face)
        for off in (0.25, 0.125):
            f = face.copy()
            f[:, a] += off
            pts.append(f[f[:, a] < n])
    pts.append(np.stack(np.meshgrid(half, half, half, indexing="ij"), -1).reshape(-1, 3))           # cell centres
    return np.ascontiguousarray(np.concatenate(pts) - SHIFT, f32)


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_closest(nodes, recs, info, pts, rows, edges=False, spheres=None, rho_c=RHO_C, tie_rule=True, strict=True, stats=None):
    """closest_bvh_kernel in numpy: the fp32 box test of csrc/rt_closest.hpp operation by operation over a dumped tree (nodes,
    recs, info of api.bvh_build / query_tree), the order-free winner rule, the triangle arithmetic of closest_triangle (looked
    up in table(): the same function on the same operands).  pts (n, 4).  Returns (HIT_DTYPE array, triangle tests made).
    Switches that break one rule each, for tests of the tests: strict=False skips a child at lb >= best and drops a popped
    entry at lb >= best; tie_rule=False lets the first visited keep a tie.  stats: a dict that receives
    query_accel_expect.note_high_water's marks."""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    n_tris = recs.shape[0]
    tab = table(pts, rows, edges, spheres)
    T, U, V = tab[0], tab[1], tab[2]
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    out = np.zeros(pts.shape[0], HIT_DTYPE)
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(pts.shape[0]):
            p, d2max = pts[i, :3], pts[i, 3]
            if not d2max >= 0:                                           # a NaN or negative d2max accepts nothing
                out[i] = (0, 0, 0, -1)
                note_high_water(stats, 0)
                continue
            state = {"t": d2max, "i": -1}

            def keep(tj, j):
                if tj < state["t"] or (tj == state["t"] and (state["i"] < 0 or (tie_rule and j < state["i"]))):
                    state.update(t=tj, i=int(j))

            finite = bool(np.isfinite(p).all())
            pmax = np.abs(p).max()

            def stale(g):
                return (g < -state["t"]) if strict else (g <= -state["t"])

            def leaf(k):
                nonlocal tests
                tests += 1
                keep(T[i, index[k]], index[k])

            def child(nd):                                               # skipped where its entry would be stale at once
                lb = box_gap_lb(nd, p, p, pmax, rho_c)
                return keys_of(-lb, finite & ~np.isnan(lb), stale(-lb))

            mark, _ = walk(nodes, cap, True, child, leaf, stale)
            note_high_water(stats, mark)
            for j in index[n_leaf:]:
                tests += 1
                keep(T[i, j], j)
            for s in range(n_tris, T.shape[1]):                          # the spheres, after the triangles
                keep(T[i, s], s)
            j = state["i"]
            out[i] = (state["t"], U[i, j], V[i, j], j) if j >= 0 else (0, 0, 0, -1)
    return out, tests
