"""Test side of the k-nearest point query (rt_tracer_closest_all, csrc/rt_nearest.hpp): the expected rows by
brute force from closest_expect.table -- accept, apply the cursor, sort by (t, prim), cut, pad --, the traversal restated over a
dumped tree with the list in place of one best, the "kth" radius family and the chaining of calls through the cursor.  A
helper, not a test.  Everything is deterministic and needs no device."""
import numpy as np

import closest_expect as ce
from query_expect import HIT_DTYPE
from tree_walk_expect import box_gap_lb, keys_of, note_high_water, walk

f32 = np.float32
INF = ce.INF
MAX_HITS = 16                            # RT_MAX_HITS


def no_cursor(n):
    """n cursor records that are none: prim = -1."""
    a = np.zeros(n, HIT_DTYPE)
    a["prim"] = -1
    return a


def accepted(tab, d2max, after=None):
    """(n, P) bool: t <= d2max in plain fp32 (a NaN on either side never) and, where the point has a cursor, strictly behind it:
    t > after.t, or t == after.t and prim > after.prim (a NaN after.t: nothing)."""
    t = tab[0]
    d2max = np.broadcast_to(np.asarray(d2max, f32), (t.shape[0],))
    with np.errstate(invalid="ignore"):
        acc = t <= d2max[:, None]
        if after is not None:
            a = np.asarray(after).reshape(-1)
            assert a.dtype == HIT_DTYPE and a.shape[0] == t.shape[0]
            prim = np.arange(t.shape[1], dtype=np.int64)[None, :]
            at, ap = a["t"][:, None], a["prim"].astype(np.int64)[:, None]
            behind = (t > at) | ((t == at) & (prim > ap))
            acc &= (ap == -1) | behind
    return acc


def presort(tab):
    """(n, P) columns of every row in ascending (t, prim), NaN t last: the order of every accepted set, whatever is accepted."""
    t = tab[0]
    if t.shape[1] == 0:
        return np.zeros(t.shape, np.int64)
    prim = np.broadcast_to(np.arange(t.shape[1], dtype=np.int64)[None, :], t.shape)
    return np.lexsort((prim, t), axis=1)


def sorted_accepted(tab, d2max, after=None, order=None):
    """-> (order, first (n,), number accepted (n,)): the accepted candidates of row i are order[i, first[i] : first[i] + number[i]]
    -- in (t, prim) order "at most d2max" is a prefix and "behind the cursor" a suffix, so the accepted ones are one run."""
    if order is None:
        order = presort(tab)
    acc = np.take_along_axis(accepted(tab, d2max, after), order, axis=1)
    n_acc = acc.sum(axis=1)
    first = acc.argmax(axis=1) if acc.shape[1] else np.zeros(acc.shape[0], np.int64)
    last = acc.shape[1] - 1 - acc[:, ::-1].argmax(axis=1) if acc.shape[1] else first
    assert ((n_acc == 0) | (last - first + 1 == n_acc)).all()            # one run
    return order, first, n_acc


def expected_all(tab, d2max, max_hits, after=None, order=None):
    """Brute force on a table: -> (hits (n, max_hits) HIT_DTYPE, counts (n,) uint32).  Row i: the first max_hits accepted
    candidates in ascending (t, prim), then {0, 0, 0, -1}.  order: presort(tab), when the caller has it already."""
    t, u, v, _ = tab
    n = t.shape[0]
    hits = np.zeros((n, max_hits), HIT_DTYPE)
    hits["prim"] = -1
    order, first, n_acc = sorted_accepted(tab, d2max, after, order)
    counts = np.minimum(n_acc, max_hits).astype(np.uint32)
    rows_ = np.arange(n)
    for s in range(min(max_hits, t.shape[1])):
        ok = counts > s
        j = order[rows_, np.minimum(first + s, t.shape[1] - 1)]
        for name, src in (("t", t), ("u", u), ("v", v)):
            hits[name][ok, s] = src[rows_, j][ok]
        hits["prim"][ok, s] = j[ok]
    return hits, counts


def cut(hits, counts, max_hits):
    """The answer for a smaller max_hits from the one for a larger: the row's first max_hits records, the count capped."""
    return np.ascontiguousarray(hits[:, :max_hits]), np.minimum(counts, max_hits).astype(np.uint32)


def accepted_lists(tab, d2max):
    """The full accepted list of every point in order: [HIT_DTYPE (m_i,)] -- what chaining the cursor has to reproduce."""
    t, u, v, _ = tab
    order, first, n_acc = sorted_accepted(tab, d2max)
    out = []
    for i in range(t.shape[0]):
        j = order[i, first[i]:first[i] + n_acc[i]]
        h = np.zeros(j.shape[0], HIT_DTYPE)
        h["t"], h["u"], h["v"], h["prim"] = t[i, j], u[i, j], v[i, j], j
        out.append(h)
    return out


def chain(query, n, max_hits, rounds=None):
    """Enumerate through the cursor: query(live, after) -> (hits, counts) for the points `live` (indices; after None in the
    first round, else one record per live point).  Repeats with after = each saturated row's last record until no row is
    saturated.  -> ([HIT_DTYPE (m_i,)] per point, rounds made).  rounds: fail when more are needed."""
    live = np.arange(n)
    after = None
    got = [[] for _ in range(n)]
    made = 0
    while live.size:
        assert rounds is None or made < rounds, "more than %r rounds" % rounds
        hits, counts = query(live, after)
        made += 1
        for r, i in enumerate(live):
            got[i].append(hits[r, :counts[r]])
        more = counts == max_hits
        after = np.ascontiguousarray(hits[more, max_hits - 1])
        live = live[more]
    return [np.concatenate(g) if g else np.zeros(0, HIT_DTYPE) for g in got], made


def kth_radius(tab, q):
    """The "kth" radius family: per point d2max = the t of its q-th nearest primitive of the table (its farthest when the table
    has fewer), so that q are accepted where no t ties at the boundary.  NaN t sort last."""
    t = tab[0]
    if t.shape[1] == 0:
        return np.zeros(t.shape[0], f32)
    return np.ascontiguousarray(np.sort(t, axis=1)[:, min(q, t.shape[1]) - 1])


def same_rows(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def differing_rows(got, exp, got_counts=None, exp_counts=None):
    """Indices of the points whose row (or count) differs in any bit."""
    k = got.shape[1]
    bad = (np.ascontiguousarray(got).view(np.uint32).reshape(-1, k * 4) != np.ascontiguousarray(exp).view(np.uint32).reshape(-1, k * 4)).any(axis=1)
    if got_counts is not None:
        bad |= np.asarray(got_counts).astype(np.int64) != np.asarray(exp_counts).astype(np.int64)
    return np.nonzero(bad)[0]


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree_nearest(nodes, recs, info, pts, rows, max_hits, after=None, edges=False, spheres=None, rho_c=ce.RHO_C, tie_rule=True,
                      strict=True, stats=None):
    """nearest_bvh_kernel in numpy: closest_expect.walk_tree_closest with the sorted list of max_hits (t, prim) pairs in place
    of (best, best_i) and  bound = min(d2max, t_last)  (t_last = +inf while the list is not full) in place of best; the cursor is
    applied before the insert and prunes nothing.  pts (n, 4).  Returns (hits (n, max_hits), counts, triangle tests made).
    Switches that break one rule each, for tests of the tests: strict=False skips a child at lb >= bound and drops a popped
    entry at lb >= bound; tie_rule=False orders by t alone (the first visited keeps a tie, in the list and at the cut).  stats: a dict that
    receives query_accel_expect.note_high_water's marks."""
    pts = np.asarray(pts, f32).reshape(-1, 4)
    n_tris = recs.shape[0]
    tab = ce.table(pts, rows, edges, spheres)
    T, U, V = tab[0], tab[1], tab[2]
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    hits = np.zeros((pts.shape[0], max_hits), HIT_DTYPE)
    hits["prim"] = -1
    counts = np.zeros(pts.shape[0], np.uint32)
    cur_t = None if after is None else np.asarray(after)["t"]
    cur_p = None if after is None else np.asarray(after)["prim"].astype(np.int64)
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(pts.shape[0]):
            p, d2max = pts[i, :3], pts[i, 3]
            if not d2max >= 0:                                           # a NaN or negative d2max accepts nothing
                note_high_water(stats, 0)
                continue
            has = cur_p is not None and cur_p[i] != -1
            lst = []                                                     # [(t, prim)] in order, at most max_hits

            def before(ta, pa, tb, pb):
                return ta < tb or (ta == tb and tie_rule and pa < pb)

            def keep(tj, j):
                if not tj <= d2max:
                    return
                if has and not (tj > cur_t[i] or (tj == cur_t[i] and j > cur_p[i])):
                    return
                if len(lst) == max_hits:
                    if not before(tj, j, *lst[-1]):
                        return
                    lst.pop()
                s = len(lst)
                while s > 0 and before(tj, j, *lst[s - 1]):
                    s -= 1
                lst.insert(s, (tj, int(j)))

            def bound():
                return np.fmin(d2max, lst[-1][0]) if len(lst) == max_hits else d2max

            finite = bool(np.isfinite(p).all())
            pmax = np.abs(p).max()

            def stale(g):
                return (g < -bound()) if strict else (g <= -bound())

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
            counts[i] = len(lst)
            for s, (tj, j) in enumerate(lst):
                hits[i, s] = (tj, U[i, j], V[i, j], j)
    return hits, counts, tests
