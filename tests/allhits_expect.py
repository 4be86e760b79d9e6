"""Test side of the all-hits query (RayTracer.IntersectAll / rt_tracer_intersect_all): what every ray must answer, computed
from a table of the oracle's HitTriangle and ray-sphere test over every primitive (with u and v), the closed fp32 interval and
the order rule -- ascending t, equal t by ascending prim; the BVH contract of include/rt_mi355x.h as a per-ray check; a numpy
restatement of the traversal that walks a dumped tree without a GPU; and a scene of stacked sheets with many hits per ray."""
import ctypes as C

import numpy as np

from occluded_expect import conditioning_matrix
from query_accel_expect import RHO, WELL_CONDITIONED
from query_expect import HIT_DTYPE
from tree_walk_expect import EMPTY, keys_of, note_box_arithmetic, note_high_water, ray_slab, walk

INF = np.float32(np.inf)
MAX_HITS = 16                                                            # RT_MAX_HITS


def hit_table_uv(orc, rays, tri_rows, spheres=None, contract=None):
    """Per ray and primitive (triangles in upload order, then spheres): (hit (n, P) bool, t, u, v (n, P) float32) of the
    oracle's HitTriangle on absolute triangle rows (3N, 4) and of its ray-sphere test (u = v = 0).  rays: (n, 6) or the first
    six columns of (n, 8) segments."""
    contract = orc.FMA if contract is None else contract
    L = orc.lib()
    f3 = C.c_float * 3
    fp = C.POINTER(C.c_float)
    tris = np.ascontiguousarray(np.asarray(tri_rows, np.float32).reshape(-1, 3, 4)[:, :, :3])
    sph = np.ascontiguousarray(np.zeros((0, 4), np.float32) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4))
    verts = [[f3(*map(float, tris[j, k])) for k in range(3)] for j in range(tris.shape[0])]
    sphs = [(C.c_float * 4)(*map(float, s)) for s in sph]
    rays = np.ascontiguousarray(np.asarray(rays, np.float32)[:, :6])
    nt = len(verts)
    hit = np.zeros((rays.shape[0], nt + len(sphs)), bool)
    tt, uu, vv = (np.zeros(hit.shape, np.float32) for _ in range(3))
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    rt, ru, rv = C.byref(t), C.byref(u), C.byref(v)
    for i in range(rays.shape[0]):
        ray = rays[i].ctypes.data_as(fp)
        for j, (a, b, c) in enumerate(verts):
            if L.orc_hit_triangle(ray, a, b, c, contract, 0, rt, ru, rv):
                hit[i, j] = True
                tt[i, j], uu[i, j], vv[i, j] = t.value, u.value, v.value
        for s, sp in enumerate(sphs):
            if L.orc_hit_sphere(ray, sp, contract, rt):
                hit[i, nt + s] = True
                tt[i, nt + s] = t.value
    return hit, tt, uu, vv


def take(table, sel):
    """The rows `sel` of a hit table."""
    return tuple(x[sel] for x in table)


def exact_set(table, segs, i, row=None):
    """E of segment i (a ray of table row `row`, i by default): every in-interval hit as a HIT_DTYPE array in the order of the
    rule (fp32 comparisons: a NaN t or bound is outside; a stable sort by t of the ascending prims, so that equal t -- -0 == +0
    included -- stays in prim order)."""
    hit, t, u, v = table
    r = i if row is None else row
    seg = np.asarray(segs, np.float32).reshape(-1, 8)[i]
    with np.errstate(invalid="ignore"):
        prims = np.nonzero(hit[r] & (seg[6] <= t[r]) & (t[r] <= seg[7]))[0]
    prims = prims[np.argsort(t[r, prims], kind="stable")]
    out = np.zeros(prims.shape[0], HIT_DTYPE)
    out["t"], out["u"], out["v"], out["prim"] = t[r, prims], u[r, prims], v[r, prims], prims
    return out


def expected_all_hits(table, segs, max_hits, idx=None):
    """(hits (n, max_hits) HIT_DTYPE, counts (n,) uint32): the first max_hits elements of every segment's exact set, then
    records {0, 0, 0, -1}.  idx: the table row of each segment's ray (its own index by default).  The order of a ray's hits does
    not depend on the interval, so every table row is sorted once -- stable, by t, from ascending prims; the misses and the NaN
    t last -- and a segment takes the first max_hits sorted entries that lie in its interval."""
    hit, t, u, v = table
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    n = segs.shape[0]
    idx = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    key = np.where(hit, t, np.float32(np.nan))
    order = np.argsort(key, axis=1, kind="stable")
    key = np.take_along_axis(key, order, axis=1)
    hits = np.zeros((n, max_hits), HIT_DTYPE)
    hits["prim"] = -1
    counts = np.zeros(n, np.uint32)
    for c0 in range(0, n, 4096):
        sl = slice(c0, min(c0 + 4096, n))
        rows = idx[sl]
        st = key[rows]
        with np.errstate(invalid="ignore"):
            inside = (segs[sl, 6:7] <= st) & (st <= segs[sl, 7:8])
        rank = np.cumsum(inside, axis=1)
        a, b = np.nonzero(inside & (rank <= max_hits))
        prim = order[rows[a], b]
        slot = rank[a, b] - 1
        block = hits[sl]
        block["t"][a, slot], block["u"][a, slot], block["v"][a, slot] = st[a, b], u[rows[a], prim], v[rows[a], prim]
        block["prim"][a, slot] = prim
        counts[sl] = np.minimum(rank[:, -1], max_hits) if rank.shape[1] else 0
    return hits, counts


def truncated(answer, max_hits):
    """The answer for a smaller max_hits from the one for a larger: the leading columns, the counts clipped."""
    return np.ascontiguousarray(answer[0][:, :max_hits]), np.minimum(answer[1], max_hits).astype(answer[1].dtype)


def same_rows(a, b):
    """Bit-exact equality of two (hits, counts) answers."""
    return (a[0].shape == b[0].shape and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint32), np.ascontiguousarray(b[0]).view(np.uint32))
            and np.array_equal(np.asarray(a[1]).astype(np.int64), np.asarray(b[1]).astype(np.int64)))


def sets_from_table(table, segs, tri_rows, idx=None):
    """(E, W) of the segments of a hit table as callables of the segment index: E(i) the exact set in order (HIT_DTYPE), W(i)
    the mask over E(i) of the spheres and the well-conditioned triangles (ratio >= 2^-10 in float64).  idx: the table row of
    each segment's ray."""
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    nt = np.asarray(tri_rows).reshape(-1, 3, 4).shape[0]

    def E(i):
        return exact_set(table, segs, i, None if idx is None else int(idx[i]))

    def W(i):
        e = E(i)
        ratio = conditioning_matrix(segs[i:i + 1], tri_rows)[0] if nt else np.zeros(0)
        tri = e["prim"] < nt
        out = np.ones(e.shape[0], bool)
        out[tri] = ratio[e["prim"][tri]] >= WELL_CONDITIONED
        return out

    return E, W


def sets_from_oracle(orc, segs, tri_rows, spheres=None, contract=None):
    """The same, asking the oracle about a ray only when the check wants it (the device comparisons: the rays that differ)."""
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    cache = {}

    def both(i):
        if i not in cache:
            table = hit_table_uv(orc, segs[i:i + 1], tri_rows, spheres, contract)
            E1, W1 = sets_from_table(table, segs[i:i + 1], tri_rows)
            cache.clear()
            cache[i] = (E1(0), W1(0))
        return cache[i]

    return (lambda i: both(i)[0]), (lambda i: both(i)[1])


def _before(a, b):
    """(t, prim) of a sorts strictly before b's."""
    return bool(a["t"] < b["t"]) or (bool(a["t"] == b["t"]) and int(a["prim"]) < int(b["prim"]))


def check_bvh_all_hits(got, ref, E, W, max_hits, cap=None, label="", every=False):
    """The BVH contract, per ray: the stored entries are elements of E with equal bits, strictly ascending in (t, prim), padded
    with {0, 0, 0, -1}, and  got == the first max_hits of (W u got)  -- which says that got is the first max_hits elements of
    some E' with W <= E' <= E.  ref is the scan's (or the expected) answer: a ray whose answer equals it bit for bit is the
    first max_hits of E itself and is checked no further unless `every`.  Returns and prints how many rays differ from ref;
    cap: at most this share of the rays may."""
    hits, counts = np.asarray(got[0]), np.asarray(got[1]).astype(np.int64)
    rhits, rcounts = np.asarray(ref[0]), np.asarray(ref[1]).astype(np.int64)
    n = counts.shape[0]
    assert hits.shape == rhits.shape == (n, max_hits) and rcounts.shape == (n,), (label, hits.shape, rhits.shape)
    gb = np.ascontiguousarray(hits).view(np.uint32).reshape(n, max_hits * 4)
    rb = np.ascontiguousarray(rhits).view(np.uint32).reshape(n, max_hits * 4)
    differ = (gb != rb).any(axis=1) | (counts != rcounts)
    if cap is not None:                                                  # (before the oracle is asked about each of them)
        assert differ.sum() <= cap * n, (label, int(differ.sum()))
    pad = np.zeros(1, HIT_DTYPE)
    pad["prim"] = -1
    for i in (range(n) if every else np.nonzero(differ)[0]):
        c = int(counts[i])
        assert 0 <= c <= max_hits, (label, i, c)
        row = hits[i]
        assert (row[c:].view(np.uint32).reshape(-1, 4) == pad.view(np.uint32)).all(), (label, i, "padding", row)
        assert (row["prim"][:c] >= 0).all(), (label, i, "an empty record inside the count", row)
        e, w = E(i), W(i)
        where = {int(p): k for k, p in enumerate(e["prim"])}
        for k in range(c):
            p = int(row["prim"][k])
            assert p in where, (label, i, "a stored hit is not in the exact set", row[k])
            assert row[k:k + 1].view(np.uint32).tolist() == e[where[p]:where[p] + 1].view(np.uint32).tolist(), \
                (label, i, "bits differ", row[k], e[where[p]])
            assert k == 0 or _before(row[k - 1], row[k]), (label, i, "not strictly ascending", row[:c])
        keep = w.copy()
        keep[[where[int(p)] for p in row["prim"][:c]]] = True            # W u got, in E's order
        want = e["prim"][keep][:max_hits]
        assert want.tolist() == row["prim"][:c].tolist(), (label, i, "a well-conditioned hit was lost", row[:c], e[keep][:max_hits])
    used = int(differ.sum())
    print("%s: %d rays, max_hits %d, mean count %.2f, %d full, %d differ from the scan (ill-conditioned hits only)"
          % (label, n, max_hits, float(counts.mean()) if n else 0.0, int((counts == max_hits).sum()), used))
    return used


# ---- the traversal, restated ---------------------------------------------------------------------------------------------

def walk_tree_all_hits(orc, nodes, recs, info, segs, rows, max_hits, spheres=None, contract=None, rho=RHO, tie_rule=True, strict=True,
                       stats=None):
    """allhits_bvh_kernel in numpy: the tree with the fp32 box test of csrc/rt_allhits.hpp operation by operation -- a child is
    skipped when exit < enter, exit < tmin, enter > tmax or, once the list holds max_hits entries, enter > t_last, unless the
    ray has a non-finite component or a zero direction or the child's arithmetic holds a NaN; the nearest child is entered
    first; a popped entry whose enter fell strictly behind t_last is dropped -- then the always-tested list and the spheres,
    with the oracle's HitTriangle on absolute rows.  Returns (hits, counts, triangle tests made).
    Switches that break one rule each, for tests of the tests: tie_rule=False keeps equal t in the order of arrival; strict=False
    also skips a child whose exit EQUALS tmin or whose enter EQUALS tmax or t_last, and drops a popped entry whose enter EQUALS
    t_last.  stats: a dict that receives note_box_arithmetic's counters and note_high_water's marks."""
    contract = orc.FMA if contract is None else contract
    L = orc.lib()
    fp = C.POINTER(C.c_float)
    tris = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3])
    nt = tris.shape[0]
    sph = np.ascontiguousarray(np.zeros((0, 4), np.float32) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4))
    segs = np.ascontiguousarray(np.asarray(segs, np.float32).reshape(-1, 8))
    n_leaf = recs.shape[0] - info["always_tested"]
    index = recs["index"].astype(np.int64)
    hits = np.zeros((segs.shape[0], max_hits), HIT_DTYPE)
    hits["prim"] = -1
    counts = np.zeros(segs.shape[0], np.uint32)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    f32, inf = np.float32, np.float32(np.inf)
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(segs.shape[0]):
            ray = segs[i].ctypes.data_as(fp)
            o, d, tmin, tmax = segs[i, :3], segs[i, 3:6], segs[i, 6], segs[i, 7]
            lst = []                                                     # (t, prim, u, v), sorted, at most max_hits

            def t_last():
                return lst[-1][0] if len(lst) == max_hits else inf

            def insert(tj, prim, uj, vj):
                if not (bool(tmin <= tj) and bool(tj <= tmax)):
                    return
                k = len(lst)
                while k > 0 and (tj < lst[k - 1][0] or (tie_rule and tj == lst[k - 1][0] and prim < lst[k - 1][1])):
                    k -= 1
                lst.insert(k, (tj, prim, uj, vj))
                del lst[max_hits:]

            def test(j):
                a, b, c = tris[j]
                if L.orc_hit_triangle(ray, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp), contract, 0,
                                      C.byref(t), C.byref(u), C.byref(v)):
                    insert(f32(t.value), int(j), f32(u.value), f32(v.value))

            active = bool(tmin <= tmax)
            prunes = bool(np.isfinite(segs[i, :6]).all()) and bool((d != 0).any())
            inv = f32(1.0) / d
            omax = np.abs(o).max()
            seen = {}

            def stale(g):
                return (g < -t_last()) if strict else (g <= -t_last())

            def leaf(k):
                nonlocal tests
                tests += 1
                test(index[k])

            def child(nd):
                enter, exit_, nan, t1, t2 = ray_slab(nd, o, inv, omax, rho)
                skip = (exit_ < enter) | (exit_ < tmin) | (enter > tmax) | (enter > t_last())
                if not strict:
                    skip |= (exit_ == tmin) | (enter == tmax) | (enter == t_last())
                note_box_arithmetic(stats, seen, t1, t2, nd["child"] != EMPTY)
                return keys_of(-enter, prunes & ~nan, skip)

            mark, _ = walk(nodes, cap, active, child, leaf, stale)
            note_high_water(stats, mark)
            if active:
                for j in index[n_leaf:]:
                    tests += 1
                    test(j)
                for s in range(sph.shape[0]):
                    if L.orc_hit_sphere(ray, sph[s].ctypes.data_as(fp), contract, C.byref(t)):
                        insert(f32(t.value), nt + s, f32(0), f32(0))
            for k, (tj, prim, uj, vj) in enumerate(lst):
                hits[i, k] = (tj, uj, vj, prim)
            counts[i] = len(lst)
    return hits, counts, tests


# ---- a scene with many hits per ray --------------------------------------------------------------------------------------

def layered_scene(layers, cells, seed):
    """`layers` sheets z = -2 - 0.25 k over [-3, 3]^2, each cells x cells quads of two triangles; every vertex of every triangle
    jittered by N(0, 0.02) per coordinate; the winding alternates with (k + i + j) % 2, so that about every second sheet faces
    a ray.  (3N, 4) float32 upload rows, N = 2 layers cells^2."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-3.0, 3.0, cells + 1)
    tris = []
    for k in range(layers):
        z = -2.0 - 0.25 * k
        for i in range(cells):
            for j in range(cells):
                p = [[xs[i], xs[j], z], [xs[i + 1], xs[j], z], [xs[i + 1], xs[j + 1], z], [xs[i], xs[j + 1], z]]
                for a, b, c in ((0, 1, 2), (0, 2, 3)):
                    tris.append([p[a], p[c], p[b]] if (k + i + j) % 2 else [p[a], p[b], p[c]])
    v = np.asarray(tris, np.float64) + rng.normal(0.0, 0.02, (len(tris), 3, 3))
    rows = np.zeros((len(tris), 3, 4), np.float32)
    rows[:, :, :3] = v
    return rows.reshape(-1, 4)
