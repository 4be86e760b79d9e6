"""Test side of the swept query (rt_tracer_sphere_cast, csrc/rt_spherecast.hpp): the rule of
include/rt_mi355x.h in numpy, one operation per operation, in float32 (what the kernels compute, bit for bit) or, through the
same text, in float64; the expected answer by brute force under the winner rule; float64 distances written independently
(closest_expect.distance64); the residual and drop-rate measurement behind RT_SWEEP_SLACK; the traversal restated over a dumped
tree; and the sweep populations of the tests.  A helper, not a test.  Everything is deterministic and needs no device."""
import numpy as np

import closest_expect as ce
from query_accel_expect import records_of_rows
from query_expect import HIT_DTYPE, cross3 as _cross, dot3 as _dot
from tree_walk_expect import keys_of, note_high_water, slab, walk

f32 = np.float32
INF = f32(np.inf)
SLACK = f32(2.0 ** -11)                 # RT_SWEEP_SLACK (include/rt_mi355x.h)
RHO_S = f32(2.0 ** -16)                 # RT_SWEEP_RHO (csrc/rt_kernels.hpp)
TINY, HUGE = f32(2.0 ** -72), f32(2.0 ** 62)      # kSweepTiny, kSweepHuge (csrc/rt_spherecast.hpp: the range guard)
# The largest residual (sqrt(d2_float64) - r) / (max|c| + r) of an uncertified candidate that is a genuine first contact, over
# margin_families() (test_spherecast_expect.py measures it again and prints it per family); SLACK is the smallest power of two
# >= 4 x that.  DROP_BOUND: the share of genuine contacts certification drops, per family (measured: 23 of 3132 sliver pairs,
# none elsewhere -- on a sliver closest_triangle's own float32 distance is far off, the point query's "well shaped" clause).
RESIDUAL_MEASURED = 7.67e-05
DROP_BOUND = {"general r=0.1": 0.0, "general r=0.001": 0.0, "sliver": 0.008, "grazing": 0.0, "far origin": 0.0}
FEATURES = ("start", "face", "edge AB", "edge AC", "edge BC", "vertex A", "vertex B", "vertex C")


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _axpy(m, k, v):
    return [m[i] + k * v[i] for i in range(3)]


def _axmy(m, k, v):
    return [m[i] - k * v[i] for i in range(3)]


def _closest(p, v0, e1, e2):
    """closest_triangle of include/rt_mi355x.h on component lists that broadcast; any float type -> t, u, v."""
    ap = _sub(p, v0)
    a, b, c = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    d1, d2 = _dot(e1, ap), _dot(e2, ap)
    d3, d4, d5, d6 = d1 - a, d2 - b, d1 - b, d2 - c
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    w = d43 / (d43 + d56)
    den = one / ((va + vb) + vc)
    u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - w], vb * den)
    v = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w], vc * den)
    r = [(ap[k] - u * e1[k]) - v * e2[k] for k in range(3)]
    return _dot(r, r), u, v


def _entry(m, dv, a, rr):
    """sweep_entry: the entry root of m + t*dv into the ball of squared radius rr, +inf where there is none."""
    bp = -_dot(m, dv)
    l = _axpy(m, bp / a, dv)
    disc = rr - _dot(l, l)
    t = (_dot(m, m) - rr) / (bp + np.sqrt(a * disc))
    return np.where((bp > 0) & (disc >= 0) & (t > 0), t, np.inf).astype(t.dtype)


def _edge(m, e, d, rr):
    ee = _dot(e, e)
    s0, sd = _dot(m, e) / ee, _dot(d, e) / ee
    mp, dp = _axmy(m, s0, e), _axmy(d, sd, e)
    t = _entry(mp, dp, _dot(dp, dp), rr)
    s = s0 + t * sd
    return np.where((s >= 0) & (s <= 1), t, np.inf).astype(t.dtype)


def _face(w, e1, e2, d, r):
    n = _cross(e1, e2)
    nn = _dot(n, n)
    h, dn = _dot(n, w), _dot(n, d)
    num = np.abs(h) - r * np.sqrt(nn)
    den = np.where(h >= 0, -dn, dn)
    t = num / den
    q = _axpy(w, t, d)
    u, v = _dot(_cross(q, e2), n) / nn, _dot(_cross(e1, q), n) / nn
    ok = (num > 0) & (den > 0) & (t > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    return np.where(ok, t, np.inf).astype(t.dtype)


def _cols(x, dt):
    x = np.asarray(x, dt)
    return [x[:, k, None] for k in range(3)]


def _rowsT(x, dt):
    x = np.asarray(x, f32).astype(dt)
    return [x[None, :, k] for k in range(3)]


def triangle_rule(sweeps, v0, e1, e2, dt=f32, slack=SLACK):
    """Every sweep against every record -> dict of (P, T) arrays: t (+inf: no contact; tmax not applied), u, v, feature (index
    into FEATURES, -1: none), cand (the smallest root before certification, 0 at start overlap, +inf: none), certified."""
    sw = np.asarray(sweeps, dt).reshape(-1, 8)                        # (float64: a caller may pass a radius float32 does not hold)
    with np.errstate(all="ignore"):
        o, d = _cols(sw[:, 0:3], dt), _cols(sw[:, 3:6], dt)
        r = sw[:, 6, None].astype(dt)
        V0, E1, E2 = _rowsT(v0, dt), _rowsT(e1, dt), _rowsT(e2, dt)
        rr, dd = r * r, _dot(d, d)
        t0, u0, v0_ = _closest(o, V0, E1, E2)
        start = t0 <= rr
        w = _sub(o, V0)
        wb, wc = _sub(w, E1), _sub(w, E2)
        roots = [_face(w, E1, E2, d, r), _edge(w, E1, d, rr), _edge(w, E2, d, rr), _edge(wb, _sub(E2, E1), d, rr),
                 _entry(w, d, dd, rr), _entry(wb, d, dd, rr), _entry(wc, d, dd, rr)]
        roots = [np.broadcast_to(x, t0.shape) for x in roots]
        t = roots[0]
        for x in roots[1:]:
            t = np.fmin(t, x)
        feat = np.full(t0.shape, -1)
        for i in range(6, -1, -1):
            feat = np.where(roots[i] == t, i + 1, feat)
        has = t < np.inf
        c = _axpy(o, t, d)
        s = dt(slack) * (np.maximum(np.maximum(np.abs(c[0]), np.abs(c[1])), np.abs(c[2])) + r)
        rs = r + s
        d2, u1, v1 = _closest(c, V0, E1, E2)
        cert = has & (d2 <= rs * rs)
        zero = np.zeros_like(t0)
        out = {"t": np.where(start, zero, np.where(cert, t, np.inf)), "u": np.where(start, u0, np.where(cert, u1, zero)),
               "v": np.where(start, v0_, np.where(cert, v1, zero)), "feature": np.where(start, 0, np.where(has, feat, -1)),
               "cand": np.where(start, zero, t), "certified": start | cert}
    for k in ("t", "u", "v", "cand"):
        out[k] = out[k].astype(dt)
    return out


def sphere_rule(sweeps, spheres, dt=f32, slack=SLACK):
    """Every sweep against every sphere {centre, radius} of the scene -> t (P, S), +inf: no contact."""
    sw = np.asarray(sweeps, dt).reshape(-1, 8)
    sp = np.asarray(spheres, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        o, d = _cols(sw[:, 0:3], dt), _cols(sw[:, 3:6], dt)
        r = sw[:, 6, None].astype(dt)
        C, R = _rowsT(sp[:, :3], dt), sp[None, :, 3].astype(dt)
        rr, dd = r * r, _dot(d, d)
        w = _sub(o, C)
        ww = _dot(w, w)
        dist = np.sqrt(ww)
        s0 = np.abs(dist - R)
        start = s0 * s0 <= rr
        ro = R + r
        t_out = _entry(w, d, dd, ro * ro)
        ri = R - r
        rri = ri * ri
        bp = -_dot(w, d)
        l = _axpy(w, bp / dd, d)
        disc = rri - _dot(l, l)
        sq = np.sqrt(dd * disc)
        tx = np.where(bp > 0, (bp + sq) / dd, (rri - ww) / (sq - bp))
        t_in = np.where((disc >= 0) & (tx > 0), tx, np.inf)
        t = np.where(dist > R, t_out, np.where((dist < R) & (r < R), t_in, np.inf)).astype(dt)
        has = t < np.inf
        c = _axpy(o, t, d)
        s = dt(slack) * (np.maximum(np.maximum(np.abs(c[0]), np.abs(c[1])), np.abs(c[2])) + r)
        rs = r + s
        wc = _sub(c, C)
        s1 = np.abs(np.sqrt(_dot(wc, wc)) - R)
        cert = has & (s1 * s1 <= rs * rs)
        out = np.where(start, 0, np.where(cert, t, np.inf)).astype(dt)
    return out


def valid(sweeps):
    sw = np.asarray(sweeps, f32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return (sw[:, 6] >= 0) & (sw[:, 6] < INF) & (sw[:, 7] >= 0)


def table(sweeps, rows, edges=False, spheres=None, dt=f32, block=256):
    """(t, u, v, feature) per (sweep, prim), the spheres as further columns (u = v = 0, feature 0); tmax not applied.  With
    dt = float64 the sweeps may be float64 too (a radius float32 does not hold)."""
    sw = np.asarray(sweeps, dt).reshape(-1, 8)
    n = sw.shape[0]
    nt = 0 if rows is None else len(rows) // 3
    ns = 0 if spheres is None else len(spheres)
    t = np.full((n, nt + ns), np.inf, dt)
    u, v = np.zeros((n, nt + ns), dt), np.zeros((n, nt + ns), dt)
    feat = np.full((n, nt + ns), -1)
    if nt:
        rec = records_of_rows(rows, edges)
        for i in range(0, n, block):
            o = triangle_rule(sw[i:i + block], *rec, dt=dt)
            t[i:i + block, :nt], u[i:i + block, :nt], v[i:i + block, :nt], feat[i:i + block, :nt] = o["t"], o["u"], o["v"], o["feature"]
    if ns:
        t[:, nt:] = sphere_rule(sw, spheres, dt=dt)
        feat[:, nt:] = np.where(t[:, nt:] < np.inf, 0, -1)
    return t, u, v, feat


def winners(tab, sweeps):
    """The winner rule: accepted when the sweep is valid and t <= tmax; the smallest (t, prim).  -> HIT_DTYPE (n,), winning feature."""
    t, u, v, feat = tab
    sw = np.asarray(sweeps, f32).reshape(-1, 8)
    out = np.zeros(t.shape[0], HIT_DTYPE)
    out["prim"] = -1
    wf = np.full(t.shape[0], -1)
    if t.shape[1] == 0:
        return out, wf
    with np.errstate(invalid="ignore"):
        acc = (t < np.inf) & (t <= sw[:, 7, None].astype(t.dtype)) & valid(sw)[:, None]
    idx = np.argmin(np.where(acc, t, np.inf), axis=1)                 # the first of the smallest
    rows_ = np.arange(t.shape[0])
    ok = acc.any(axis=1)
    out["t"][ok], out["u"][ok], out["v"][ok], out["prim"][ok] = t[rows_, idx][ok], u[rows_, idx][ok], v[rows_, idx][ok], idx[ok]
    wf[ok] = feat[rows_, idx][ok]
    return out, wf


def expected(sweeps, rows, edges=False, spheres=None):
    """Brute force: sweeps (n, 8) -> HIT_DTYPE (n,)."""
    return winners(table(sweeps, rows, edges, spheres), sweeps)[0]


same_hits = ce.same_hits
differing = ce.differing


def centres(sweeps, t):
    """c = o + t*d in float32, the product, then the sum; and s = SLACK * (max|c| + r)."""
    sw = np.asarray(sweeps, f32).reshape(-1, 8)
    with np.errstate(all="ignore"):
        c = sw[:, 0:3] + np.asarray(t, f32)[:, None] * sw[:, 3:6]
        s = SLACK * (np.abs(c).max(axis=1) + sw[:, 6])
    assert c.dtype == f32 and s.dtype == f32
    return c, s


def distance64(p, rows, edges=False, spheres=None):
    """(P, prims) float64 distances from the points to the primitives, independent of the rule's operation order."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    cols = []
    if rows is not None and len(rows):
        cols.append(ce.distance64(p, rows, edges))
    if spheres is not None and len(spheres):
        sp = np.asarray(spheres, np.float64).reshape(-1, 4)
        cols.append(np.abs(np.linalg.norm(p[:, None, :] - sp[None, :, :3], axis=2) - sp[None, :, 3]))
    return np.concatenate(cols, axis=1) if cols else np.zeros((p.shape[0], 0))


def margin(sweeps, rows, edges=False, block=256):
    """What RT_SWEEP_SLACK is fixed from, over finite valid sweeps against the scene's finite triangles, pair by pair: a pair is
    GENUINE when the float64 run of the rule finds a contact at t64 > 0 and the float32 candidate lies within 2^-10 * (1 + t64) of
    it (the same root, well conditioned).  -> the largest residual (sqrt(d2_float64(c)) - r) / (max|c| + r) of the float32
    candidates of genuine pairs, the number of genuine pairs, and how many of them certification drops."""
    sw = np.asarray(sweeps, f32).reshape(-1, 8)
    sw = sw[valid(sw) & np.isfinite(sw[:, :7]).all(axis=1)]
    rec = records_of_rows(rows, edges)
    worst, genuine, dropped = 0.0, 0, 0
    for i in range(0, sw.shape[0], block):
        b = sw[i:i + block]
        a32, a64 = triangle_rule(b, *rec), triangle_rule(b, *rec, dt=np.float64)
        with np.errstate(all="ignore"):
            g = (a64["t"] > 0) & (a64["t"] < np.inf) & (a32["cand"] < INF) & (a32["cand"] > 0)
            g &= np.abs(a32["cand"].astype(np.float64) - a64["t"]) <= 2.0 ** -10 * (1.0 + a64["t"])
        if not g.any():
            continue
        pi, ti = np.nonzero(g)
        c, _ = centres(b[pi], a32["cand"][pi, ti])
        d = np.empty(len(pi))
        for t in np.unique(ti):
            m = ti == t
            d[m] = ce.distance64(c[m], rows[3 * t:3 * t + 3], edges)[:, 0]
        r = b[pi, 6].astype(np.float64)
        res = (d - r) / (np.abs(c.astype(np.float64)).max(axis=1) + r)
        worst = max(worst, float(res.max()))
        genuine += len(pi)
        dropped += int((~a32["certified"][pi, ti]).sum())
    return worst, genuine, dropped


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_spherecast(nodes, recs, info, sweeps, rows, edges=False, spheres=None, ks=f32(4.0) * SLACK, rho_s=RHO_S, tie_rule=True,
                         strict=True, stack_cap=None, stats=None, range_guard=True):
    """spherecast_bvh_kernel in numpy over a dumped tree (nodes, recs, info of api.bvh_build / query_tree), fp32, operation by
    operation: sweep_valid first (an invalid sweep answers prim -1 and never walks); occluded_prune's "prunes at all" (every
    component of o and d finite, d not zero), 1 / d and max|o|; sweep_range_guard: the sweep prunes only while (max|o| + the
    largest of the root's four cmax) + r < HUGE; best starts at tmax with no prim.  child() grows each child box by
      g = (r + TINY) + (ks * (cmax + r) + rho_s * ((max|o| + cmax) + r))
    in that association, runs tree_walk_expect.slab on it and skips the child when exit < enter, exit < 0 or enter > best; its
    key is -enter (the nearest entry first), and a sweep that does not prune or a child with a NaN among its six products takes
    no decision.  A popped entry is stale when key < -best.  A leaf's record goes through sweep_keep's order-free rule -- t <
    best, or t == best and (no prim yet or a lower prim) -- with the pair's entry of table(): the same arithmetic on the same
    operands.  The kernel skips the certification of a candidate that cannot win and table() certifies every pair; such a
    candidate is not kept either way, so the answer is the same.  A walk that had to drop an entry (stack_cap; default 3 * depth,
    which never overflows) starts again from best = tmax over every leaf record, as overlap_expect.walk_tree restates it.  The
    always-tested list and then the spheres follow the walk.  Returns (HIT_DTYPE array, triangle tests made).  Switches that break
    one thing each, for tests of the tests: strict=False skips a child at enter >= best and drops a popped entry at key <= -best;
    tie_rule=False lets the first visited keep a tie; ks = rho_s = 0 grows the box by r alone; range_guard=False is the walk
    without sweep_range_guard and without TINY, which loses records once r * r or (r + s)^2 underflows or overflows.  stats: a dict that receives
    tree_walk_expect.note_high_water's marks."""
    sw = np.asarray(sweeps, f32).reshape(-1, 8)
    ks, rho_s = f32(ks), f32(rho_s)
    n_tris = recs.shape[0]
    T, U, V, _ = table(sw, rows, edges, spheres)
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    out = np.zeros(sw.shape[0], HIT_DTYPE)
    ok = valid(sw)
    tests = 0
    cap = 3 * max(info["depth"], 1) if stack_cap is None else stack_cap
    with np.errstate(all="ignore"):
        for i in range(sw.shape[0]):
            if not ok[i]:
                out[i] = (0, 0, 0, -1)
                note_high_water(stats, 0)
                continue
            o, d, r, tmax = sw[i, 0:3], sw[i, 3:6], sw[i, 6], sw[i, 7]
            state = {"t": tmax, "i": -1}

            def keep(j):
                tj = T[i, j]
                if not tj < INF:                                         # no contact: sweep_triangle returns before sweep_keep
                    return
                if tj < state["t"] or (tj == state["t"] and (state["i"] < 0 or (tie_rule and j < state["i"]))):
                    state.update(t=tj, i=int(j))

            prunes = bool(np.isfinite(sw[i, :6]).all()) and bool((d != 0).any())
            inv = f32(1.0) / d
            omax = np.abs(o).max()
            rg = r
            if range_guard:
                if nodes.shape[0]:
                    prunes = prunes and bool((omax + np.fmax.reduce(nodes[0]["cmax"])) + r < HUGE)
                rg = r + TINY

            def stale(key):
                return (key < -state["t"]) if strict else (key <= -state["t"])

            def leaf(k):
                nonlocal tests
                tests += 1
                keep(index[k])

            def child(nd):
                g = rg + (ks * (nd["cmax"] + r) + rho_s * ((omax + nd["cmax"]) + r))
                assert g.dtype == f32
                enter, exit_, nan, _, _ = slab(nd, o, inv, g)
                skip = (exit_ < enter) | (exit_ < 0) | ((enter > state["t"]) if strict else (enter >= state["t"]))
                return keys_of(-enter, prunes & ~nan, skip)

            mark, overflow = walk(nodes, cap, True, child, leaf, stale, enforce_cap=stack_cap is None)
            note_high_water(stats, mark)
            if overflow:                                                 # every leaf record, from the start
                state.update(t=tmax, i=-1)
                for j in index[:n_leaf]:
                    tests += 1
                    keep(j)
            for j in index[n_leaf:]:
                tests += 1
                keep(j)
            for s in range(n_tris, T.shape[1]):                          # the spheres, after the triangles
                keep(s)
            j = state["i"]
            out[i] = (state["t"], U[i, j], V[i, j], j) if j >= 0 else (0, 0, 0, -1)
    return out, tests


# ---- scenes and sweeps ----------------------------------------------------------------------------------------------------

def scene(n_tris, seed=5, bad=True):
    """n_tris triangles: closest_expect.sliver_scene (every second one a sliver); from 5 up, two zero-area triangles (a segment,
    a point) and, with `bad`, one record with a NaN coordinate (the always-tested list of the tree)."""
    rows = ce.sliver_scene(n_tris, seed).reshape(-1, 3, 4)
    if n_tris >= 5:
        rows[2, 2, :3] = rows[2, 1, :3]                                     # a segment
        rows[3, 1, :3] = rows[3, 2, :3] = rows[3, 0, :3]                    # a point
        if bad:
            rows[4, 1, 0] = np.nan
    return np.ascontiguousarray(rows.reshape(-1, 4))


def three_spheres():
    """Two coincident spheres and one far away."""
    return np.array([[0.5, -0.25, 0.75, 0.5], [0.5, -0.25, 0.75, 0.5], [40.0, 30.0, -20.0, 2.0]], f32)


def _sweeps(o, d, r, tmax=np.inf):
    n = len(o)
    out = np.empty((n, 8), f32)
    out[:, 0:3], out[:, 3:6] = o, d
    out[:, 6], out[:, 7] = r, tmax
    return out


def _finite_records(rows, edges=False):
    v0, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows, edges))
    ok = np.isfinite(v0).all(1) & np.isfinite(e1).all(1) & np.isfinite(e2).all(1)
    return v0[ok], e1[ok], e2[ok]


def _unit(x):
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    return x / np.where(n > 0, n, 1.0)


def _perp(x, rng):
    """a unit vector perpendicular to each row of x"""
    p = np.cross(x, rng.normal(0, 1, x.shape))
    return _unit(np.where(np.linalg.norm(p, axis=1, keepdims=True) > 0, p, [[1.0, 0.0, 0.0]]))


def random_sweeps(rows, n, seed, edges=False, rmin=-3.0, rmax=-0.5, far=1.0, rel=False):
    """Aimed at and past triangles: from a random origin (`far` times 2 .. 6 away) at a random point of a random triangle moved
    sideways by 0 .. 3 r; the direction is not normalised.  rel: lengths in units of the target triangle's extent (scale free)."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _finite_records(rows, edges)
    k = rng.integers(0, len(v0), n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    target = v0[k] + a[:, None] * e1[k] + b[:, None] * e2[k]
    unit = np.maximum(np.abs(e1[k]).max(axis=1), np.abs(e2[k]).max(axis=1)) if rel else np.ones(n)
    r = 10.0 ** rng.uniform(rmin, rmax, n) * unit
    away = _unit(rng.normal(0, 1, (n, 3)))
    o = target + away * rng.uniform(2, 6, (n, 1)) * far * unit[:, None]
    target = target + _perp(away, rng) * (rng.uniform(0, 3, (n, 1)) * r[:, None]) * (rng.uniform(0, 1, (n, 1)) < 0.5)
    d = (target - o) * rng.uniform(0.25, 2.0, (n, 1))
    return _sweeps(o, d, r)


def graze_sweeps(rows, seed, edges=False, r=0.125, tris=8):
    """Lines that pass a face, an edge and a vertex of the first `tris` finite triangles at distance r * (1 +- 2^-k), k = 4 .. 20."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _finite_records(rows, edges)
    out = []
    for j in range(min(tris, len(v0))):
        A, a, b = v0[j], e1[j], e2[j]
        n = np.cross(a, b)
        if not np.linalg.norm(n) > 0:
            continue
        n = n / np.linalg.norm(n)
        m_edge = _unit(np.cross(a, n)[None])[0]                       # in the plane, perpendicular to AB
        m_edge = m_edge if np.dot(m_edge, b) < 0 else -m_edge         # away from C
        m_vert = _unit((-(a + b))[None])[0]                            # away from the triangle, at A
        feats = [(A + 0.3 * a + 0.3 * b, n, _unit(a[None])[0]),        # parallel to the face, above an interior point
                 (A + 0.5 * a, m_edge, n),                             # across the edge AB
                 (A, m_vert, _unit(np.cross(m_vert, n)[None])[0])]     # past the vertex A
        for f, m, g in feats:
            for k in range(4, 21):
                for sgn in (-1.0, 1.0):
                    rho = r * (1.0 + sgn * 2.0 ** -k)
                    p = f + rho * m
                    L = rng.uniform(1.0, 3.0)
                    out.append(np.r_[p - L * g, g * rng.uniform(0.5, 2.0), r, np.inf])
    return np.asarray(out, f32).reshape(-1, 8)


def start_sweeps(rows, n, seed, edges=False, r=0.05):
    """Origins within r of a triangle (start overlap), random directions."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _finite_records(rows, edges)
    k = rng.integers(0, len(v0), n)
    o = v0[k] + 0.25 * e1[k] + 0.25 * e2[k] + _unit(rng.normal(0, 1, (n, 3))) * rng.uniform(0, r, (n, 1))
    return _sweeps(o, rng.normal(0, 1, (n, 3)), r)


def whole_scene_sweeps(rows, edges=False):
    """Four sweeps whose sphere holds the whole scene, or most of it, at t = 0 (radius 3/4 .. 4 of the scene's largest extent,
    from its middle, the world origin, its lowest corner and one triangle): the records start in overlap and tie at t = 0, every
    child box is entered, and the walk's stack is as full as the tree lets it be."""
    v0, e1, e2 = _finite_records(rows, edges)
    pts = np.concatenate([v0, v0 + e1, v0 + e2])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext = (hi - lo).max()
    at = ((lo + hi) / 2, np.zeros(3), lo, v0[min(5, len(v0) - 1)])
    return _sweeps(np.asarray(at), np.tile([1.0, 0.5, -0.25], (4, 1)), ext * np.array([2.0, 4.0, 0.75, 1.0]))


def tmax_sweeps(base, rows, edges=False, spheres=None):
    """Hits of `base` again with tmax below, equal to and above their contact time."""
    h = expected(base, rows, edges, spheres)
    b = base[(h["prim"] >= 0) & (h["t"] > 0)]
    t = h["t"][(h["prim"] >= 0) & (h["t"] > 0)]
    out = []
    for tm in (t * f32(0.5), np.nextafter(t, f32(0)), t, np.nextafter(t, INF), t * f32(2)):
        x = b.copy()
        x[:, 7] = tm
        out.append(x)
    return np.concatenate(out)


def bad_sweeps(good):
    """NaN, +inf and -inf in each of the eight slots of one good sweep; zero direction; negative and NaN radius and tmax."""
    out = []
    for slot in range(8):
        for val in (np.nan, np.inf, -np.inf):
            x = good.copy()
            x[slot] = val
            out.append(x)
    z = good.copy()
    z[3:6] = 0.0
    out.append(z)
    z = z.copy()
    z[0:3] = [0.5, -0.25, 0.75]
    out.append(z)
    for slot, val in ((6, -1.0), (6, -0.0), (7, -1.0), (7, -0.0), (7, 0.0)):
        x = good.copy()
        x[slot] = val
        out.append(x)
    return np.asarray(out, f32)


def batch(rows, n, seed, edges=False, spheres=None):
    """The permuted batch of the device tests, exactly n sweeps: every population above, r = 0, r larger than the scene, the
    spheres' own sweeps, then random sweeps to fill."""
    rng = np.random.default_rng(seed)
    rnd = random_sweeps(rows, 600, seed + 1, edges)
    parts = [rnd, graze_sweeps(rows, seed + 2, edges), start_sweeps(rows, 100, seed + 3, edges), bad_sweeps(rnd[0])]
    zero_r = random_sweeps(rows, 100, seed + 4, edges)
    zero_r[:, 6] = 0.0
    huge = random_sweeps(rows, 50, seed + 5, edges, far=200.0)
    huge[:, 6] = 100.0
    back = rnd[:100].copy()                                              # the same lines from the other side
    back[:, 0:3] = rnd[:100, 0:3] + rnd[:100, 3:6] * f32(4)
    back[:, 3:6] = -rnd[:100, 3:6]
    parts += [zero_r, huge, back, tmax_sweeps(rnd[:150], rows, edges, spheres)]
    if spheres is not None and len(spheres):
        sp = np.asarray(spheres, np.float64)
        m = 150
        k = rng.integers(0, len(sp), m)
        dirs = _unit(rng.normal(0, 1, (m, 3)))
        inside = rng.uniform(0, 1, m) < 0.4
        o = sp[k, :3] + dirs * np.where(inside, rng.uniform(0, 0.8, m), rng.uniform(1.5, 6, m))[:, None] * sp[k, 3:4]
        aim = sp[k, :3] + _unit(rng.normal(0, 1, (m, 3))) * rng.uniform(0, 1.3, (m, 1)) * sp[k, 3:4]
        parts.append(_sweeps(o, aim - o, 10.0 ** rng.uniform(-2, 0, m)))
    have = sum(len(p) for p in parts)
    assert have <= n, have
    parts.append(random_sweeps(rows, n - have, seed + 6, edges, rmin=-2.5, rmax=0.0))
    out = np.concatenate(parts).astype(f32)
    return np.ascontiguousarray(out[rng.permutation(n)])


def margin_families():
    """{name: (rows, sweeps)}: what RT_SWEEP_SLACK is measured over."""
    gen, sliver = ce.random_scene(48, 11), ce.sliver_scene(48, 12)
    return {"general r=0.1": (gen, random_sweeps(gen, 3000, 21, rmin=-1.0, rmax=-1.0)),
            "general r=0.001": (gen, random_sweeps(gen, 3000, 22, rmin=-3.0, rmax=-3.0)),
            "sliver": (sliver, random_sweeps(sliver, 3000, 23)),
            "grazing": (gen, graze_sweeps(gen, 24, tris=48)),
            "far origin": (gen, random_sweeps(gen, 3000, 25, far=100.0))}
