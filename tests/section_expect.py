"""Test side of the section queries (rt_tracer_section, rt_tracer_section_segments, csrc/rt_section.hpp): the
triangle and sphere rules of include/rt_mi355x.h in numpy float32, operation by operation, as a table planes x prims; the
expected rows and counts by brute force; the traversal restated over a dumped tree (tree_walk_expect.walk with the slab's own
child test), with two switches that break it; the cut records, in float32 as the kernel makes them and in float64 by the same
rule on the same fp32 inputs; and the plane populations of the tests.  A helper, not a test.  Everything is deterministic and
needs no device."""
import numpy as np

from overlap_expect import rows_of_table, same, chain, corners, random_scene         # noqa: F401  (the tests take them from here)
from query_accel_expect import records_of_rows
from query_expect import dot3 as _dot, tri_rows                                      # noqa: F401
from tree_walk_expect import note_high_water, walk

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)
MAX_HITS = 16                            # RT_MAX_HITS
NONE = -1                                # RT_PRIM_NONE
CUT_DTYPE = np.dtype([("p0", f32, 3), ("kind", np.int32), ("p1", f32, 3), ("features", np.int32)])
CUT64_DTYPE = np.dtype([("p0", np.float64, 3), ("kind", np.int32), ("p1", np.float64, 3), ("features", np.int32)])
CUT_NONE, CUT_SEGMENT, CUT_TOUCH, CUT_COPLANAR, CUT_CIRCLE = 0, 1, 2, 3, 4


def planes_of(normal, d0, d1=None):
    """(n, 8) float32 {nx, ny, nz, d0, d1, 0, 0, 0}; d1 None: planes (d1 = d0)."""
    nrm = np.asarray(normal, f32).reshape(-1, 3)
    a = np.asarray(d0, f32).reshape(-1)
    b = a if d1 is None else np.asarray(d1, f32).reshape(-1)
    out = np.zeros((max(nrm.shape[0], a.shape[0], b.shape[0]), 8), f32)
    out[:, 0:3], out[:, 3], out[:, 4] = nrm, a, b
    return out


def valid(planes):
    """(n,) bool: nx, ny, nz finite and d0 <= d1 as a plain comparison."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p[:, 0:3]).all(axis=1) & (p[:, 3] <= p[:, 4])


def project(planes, X):
    """p(X) = (nx X.x + ny X.y) + nz X.z for every plane (N) against every point X (T, 3) -> (N, T) float32."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    out = _dot([p[:, k, None] for k in range(3)], [X[None, :, k] for k in range(3)])
    assert out.dtype == f32
    return out


def triangle_rule(planes, v0, e1, e2):
    """Every plane against every record: planes (N, 8), v0, e1, e2 (T, 3) float32 -> accepted (N, T) bool."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    v0, e1, e2 = (np.asarray(x, f32).reshape(-1, 3) for x in (v0, e1, e2))
    with np.errstate(all="ignore"):
        pa, pb, pc = project(p, v0), project(p, v0 + e1), project(p, v0 + e2)
        mn, mx = np.fmin(np.fmin(pa, pb), pc), np.fmax(np.fmax(pa, pb), pc)
        nan = np.isnan(pa) | np.isnan(pb) | np.isnan(pc)
        return valid(p)[:, None] & ~nan & (mn <= p[:, 4, None]) & (mx >= p[:, 3, None])


def sphere_rule(planes, spheres):
    """(N, S) bool: the sphere rule, one float32 operation per operation."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    s = np.asarray(spheres, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        pc = project(p, s[:, :3])
        n = [p[:, k] for k in range(3)]
        rn = s[None, :, 3] * np.sqrt(_dot(n, n))[:, None]
        assert rn.dtype == f32
        return valid(p)[:, None] & (pc - rn <= p[:, 4, None]) & (pc + rn >= p[:, 3, None])


def table(planes, rows, edges=False, spheres=None, block=512):
    """(N, P) bool, column = prim: the triangles' verdicts, then the spheres'."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    n = p.shape[0]
    if rows is None or len(rows) == 0:
        acc = np.zeros((n, 0), bool)
    else:
        rec = records_of_rows(rows, edges)
        acc = np.concatenate([triangle_rule(p[i:i + block], *rec) for i in range(0, n, block)]) if n else np.zeros((0, rec[0].shape[0]), bool)
    if spheres is not None and len(spheres):
        acc = np.c_[acc, sphere_rule(p, spheres)]
    return acc


def expected(planes, rows, max_hits, after=None, edges=False, spheres=None):
    """Brute force -> (prims (n, max_hits) int32, counts (n,) uint32)."""
    return rows_of_table(table(planes, rows, edges, spheres), max_hits, after)


# ---- the traversal, restated ------------------------------------------------------------------------------------------------

def walk_tree(nodes, recs, info, planes, rows, max_hits, after=None, edges=False, spheres=None, closed=True, signed=True,
              stack_cap=None, stats=None):
    """section_bvh_kernel in numpy over a dumped tree (nodes, recs, info of api.bvh_build / query_tree).  For a child box take per
    axis xlo = (n_axis >= 0 ? lo : hi) and xhi the other end, pmin = p(xlo), pmax = p(xhi); the child is skipped only when
    pmin > d1 or pmax < d0 (a NaN never skips).  Every record met goes through the rule, then the always-tested list, then the
    spheres.  Returns (prims, counts, triangle tests made).  Switches that break one thing each, for tests of the tests:
    closed=False skips on >= and <=; signed=False takes xlo = lo and xhi = hi whatever the sign of n.  stack_cap: the number of
    entries the stack holds (default 3 * depth, which never overflows); a walk that had to drop an entry starts again from every
    leaf record, as the kernel's overflow redo does."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    acc = table(p, rows, edges, spheres)
    ok = valid(p)
    n_tris = recs.shape[0]
    n_leaf = n_tris - info["always_tested"]
    index = recs["index"].astype(np.int64)
    met = np.zeros(acc.shape, bool)
    tests = 0
    cap = 3 * max(info["depth"], 1) if stack_cap is None else stack_cap
    with np.errstate(all="ignore"):
        for i in range(p.shape[0]):
            if not ok[i]:
                note_high_water(stats, 0)
                continue
            n, d0, d1 = p[i, 0:3], p[i, 3], p[i, 4]
            pos = (n >= 0) if signed else np.ones(3, bool)

            def leaf(k):
                nonlocal tests
                assert not met[i, index[k]]                              # a walk visits every record at most once
                met[i, index[k]] = True
                tests += 1

            def child(nd):                                               # no key decides: the children are entered as stored
                xlo = np.where(pos[:, None], nd["lo"], nd["hi"])        # (3, 4)
                xhi = np.where(pos[:, None], nd["hi"], nd["lo"])
                pmin = (n[0] * xlo[0] + n[1] * xlo[1]) + n[2] * xlo[2]
                pmax = (n[0] * xhi[0] + n[1] * xhi[1]) + n[2] * xhi[2]
                assert pmin.dtype == f32 and pmax.dtype == f32
                skip = ((pmin > d1) | (pmax < d0)) if closed else ((pmin >= d1) | (pmax <= d0))
                return [None if skip[c] else INF for c in range(4)]

            mark, overflow = walk(nodes, cap, True, child, leaf, enforce_cap=stack_cap is None)
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


# ---- the cut ------------------------------------------------------------------------------------------------------------------

def _crossing(L, U, sL, sU):
    """The edge's crossing from the below end L (m, 3) to the above end U: t = sL / (sL - sU), X = L + t (U - L) per component."""
    t = sL / (sL - sU)
    return L + t[:, None] * (U - L)


def cuts(planes, prims, rows, edges=False, spheres=None, side=0, dtype=f32):
    """section_segments_kernel for all records at once: planes (n, 8), prims (n,) or (n, per_plane) int -> CUT_DTYPE of prims'
    shape.  dtype=np.float64: the same rule on the same fp32 inputs (the corners A, fl(A + e1), fl(A + e2) stay the fp32 ones),
    every operation in float64 -> CUT64_DTYPE; the case it finds may differ from the fp32 one where a sign does."""
    p = np.asarray(planes, f32).reshape(-1, 8)
    r = np.asarray(prims, np.int64)
    per = 1 if r.ndim == 1 else r.shape[1]
    flat = r.reshape(-1)
    m = flat.shape[0]
    own = np.arange(m) // per
    T = dtype
    out = np.zeros(m, CUT_DTYPE if dtype is f32 else CUT64_DTYPE)
    if m == 0:
        return out.reshape(r.shape)
    ok = valid(p)[own]
    n = p[own, 0:3].astype(T)
    d = p[own, 4 if side else 3].astype(T)
    if rows is not None and len(rows):
        A, B, C = corners(rows, edges)
    else:
        A = B = C = np.zeros((0, 3), f32)
    n_tris = A.shape[0]
    sph = np.zeros((0, 4), f32) if spheres is None else np.asarray(spheres, f32).reshape(-1, 4)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    p0, p1 = np.zeros((m, 3), T), np.zeros((m, 3), T)
    kind, f0, f1 = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)

    def put(mask, which, point, feature):
        pt, ft = (p0, f0) if which == 0 else (p1, f1)
        pt[mask] = point[mask]
        ft[mask] = feature

    with np.errstate(all="ignore"):
        tri = (flat >= 0) & (flat < n_tris)
        if tri.any():
            idx = np.where(tri, flat, 0)
            P = [A[idx].astype(T), B[idx].astype(T), C[idx].astype(T)]
            s = [dot(n, X) - d for X in P]
            assert s[0].dtype == T
            nan = np.isnan(s[0]) | np.isnan(s[1]) | np.isnan(s[2])
            above = sum((x > 0).astype(int) for x in s)
            below = sum((x < 0).astype(int) for x in s)
            on = 3 - above - below
            live = tri & ok & ~nan & (above != 3) & (below != 3)
            coplanar = live & (on == 3)
            touch = live & ~coplanar & ((above == 0) | (below == 0))
            segment = live & ~coplanar & ~touch
            kind[coplanar], kind[touch], kind[segment] = CUT_COPLANAR, CUT_TOUCH, CUT_SEGMENT
            for k in range(3):
                k1, k2 = (k + 1) % 3, (k + 2) % 3
                first = touch & (s[k] == 0) & (s[k2] != 0)               # the first on-corner of the walk A -> B -> C -> A
                two = first & (s[k1] == 0)
                put(first, 0, P[k], 4 + k)
                put(first & ~two, 1, P[k], 4 + k)
                put(two, 1, P[k1], 4 + k1)
                down, up = segment & (s[k] > 0) & (s[k1] < 0), segment & (s[k] < 0) & (s[k1] > 0)
                put(down, 0, _crossing(P[k1], P[k], s[k1], s[k]), k)     # the walk leaves the above side
                put(up, 1, _crossing(P[k], P[k1], s[k], s[k1]), k)       # ... enters it
                put(segment & (s[k] == 0) & (s[k2] > 0), 0, P[k], 4 + k)
                put(segment & (s[k] == 0) & (s[k2] < 0), 1, P[k], 4 + k)
        ball = (flat >= n_tris) & (flat < n_tris + sph.shape[0])
        if ball.any():
            S = sph[np.where(ball, flat - n_tris, 0)].astype(T)
            pc, nn = dot(n, S), dot(n, n)
            rn, e = S[:, 3] * np.sqrt(nn), d - pc
            circle = ball & ok & (np.abs(pc - d) <= rn)
            k = e / nn
            rad = np.sqrt(np.fmax(S[:, 3] * S[:, 3] - (e * e) / nn, T(0)))
            assert rad.dtype == T and k.dtype == T
            kind[circle] = CUT_CIRCLE
            p0[circle] = (S[:, :3] + k[:, None] * n)[circle]
            p1[circle, 0] = rad[circle]
    assert p0.dtype == T and p1.dtype == T
    out["p0"], out["kind"], out["p1"], out["features"] = p0, kind, p1, f0 | (f1 << 8)
    return out.reshape(r.shape)


def same_cuts(a, b):
    """Two CUT_DTYPE arrays hold the same bytes (NaN payloads included)."""
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def residual(cut64_or_32, planes, owner, scale, side=0):
    """|n.X - d| / (|n| scale) in float64 of both endpoints of every record -> (m, 2); owner (m,): the plane of each record."""
    p = np.asarray(planes, f32).reshape(-1, 8).astype(np.float64)[owner]
    n, d = p[:, 0:3], p[:, 4 if side else 3]
    ln = np.sqrt((n * n).sum(axis=1))
    out = [np.abs((n * cut64_or_32[k].astype(np.float64)).sum(axis=1) - d) / (ln * scale) for k in ("p0", "p1")]
    return np.stack(out, axis=1)


# ---- loops ---------------------------------------------------------------------------------------------------------------------

def loops(segments):
    """Chain CUT_SEGMENT records into closed loops by == of the endpoints: every p1 must be the p0 of exactly one other record.
    -> list of lists of record indices, or None when the records do not chain into closed loops."""
    seg = np.asarray(segments)
    start = {}
    for j, c in enumerate(seg):
        key = tuple(float(x) for x in c["p0"])
        if key in start:
            return None
        start[key] = j
    left = set(range(seg.shape[0]))
    out = []
    while left:
        j0 = j = min(left)
        loop = []
        while True:
            if j not in left:
                return None
            left.discard(j)
            loop.append(j)
            j = start.get(tuple(float(x) for x in seg[j]["p1"]))
            if j is None:
                return None
            if j == j0:
                break
        out.append(loop)
    return out


def loop_area(segments, loop, normal):
    """The signed area of a closed loop about `normal` (float64): positive when it runs counter-clockwise seen from its tip."""
    pts = np.asarray(segments)["p0"][loop].astype(np.float64)
    n = np.asarray(normal, np.float64)
    total = np.zeros(3)
    for a, b in zip(pts, np.roll(pts, -1, axis=0)):
        total += np.cross(a, b)
    return 0.5 * float(total @ n) / float(np.sqrt(n @ n))


# ---- scenes and planes ----------------------------------------------------------------------------------------------------------

def cube(lo=(0, 0, 0), hi=(2, 2, 2)):
    """A closed cube of 12 outward-wound triangles with small-integer corners -> (36, 4) float32 upload rows.  Triangles 2f and
    2f + 1 are face f: -x, +x, -y, +y, -z, +z."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    tris = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for sgn, at in ((-1, lo[ax]), (1, hi[ax])):
            q = []
            for su, sv in ((0, 0), (1, 0), (1, 1), (0, 1)):              # counter-clockwise about +axis
                c = np.zeros(3)
                c[ax], c[u], c[v] = at, (hi if su else lo)[u], (hi if sv else lo)[v]
                q.append(c)
            if sgn < 0:
                q = q[::-1]
            tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return tri_rows(np.array(tris))


def random_planes(rows, n, seed, thick=0.0, edges=False):
    """n slabs of random orientation through (or, thick > 0, around) random corners of the scene; normals are not unit."""
    rng = np.random.default_rng(seed)
    A, B, C = corners(rows, edges)
    fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1)
    pick = np.nonzero(fin)[0][rng.integers(0, fin.sum(), n)]
    nrm = rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1))
    at = (nrm * (A[pick].astype(np.float64) + rng.uniform(-0.1, 0.1, (n, 3)))).sum(axis=1)
    half = rng.uniform(0, thick, n) * np.sqrt((nrm * nrm).sum(axis=1))
    return planes_of(nrm, at - half, at + half)


def corner_planes(rows, tris, normals, edges=False):
    """For each triangle j of `tris` and each normal: the plane through corner A's own p value (d0 = d1 = p(A): the closed
    comparisons accept), and the slabs that end one ulp below it and begin one ulp above it (which reject the corner).
    -> (planes, tags [(j, which)]), which in ("on", "below", "above")."""
    A, _, _ = corners(rows, edges)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    out, tags = [], []
    for j in tris:
        for n in nrm:
            pa = project(planes_of(n, 0), A[j:j + 1])[0, 0]
            out.append(planes_of(n, pa)[0]), tags.append((int(j), "on"))
            out.append(planes_of(n, -INF, np.nextafter(pa, -INF))[0]), tags.append((int(j), "below"))
            out.append(planes_of(n, np.nextafter(pa, INF), INF)[0]), tags.append((int(j), "above"))
    return np.array(out, f32), tags


BAD_NAMES = ("inverted", "nan_nx", "nan_nz", "nan_d0", "nan_d1", "inf_ny", "minus_inf_nx", "d0_plus_inf_d1_finite", "nan_all")


def bad_planes(plane):
    """The planes that accept nothing, made from one good plane (8,) -> (len(BAD_NAMES), 8)."""
    out = np.repeat(np.asarray(plane, f32).reshape(1, 8), len(BAD_NAMES), axis=0)
    out[0, 3], out[0, 4] = plane[4] + f32(1.0), plane[3] - f32(1.0)
    out[1, 0] = NAN
    out[2, 2] = NAN
    out[3, 3] = NAN
    out[4, 4] = NAN
    out[5, 1] = INF
    out[6, 0] = -INF
    out[7, 3] = INF
    out[8, 0:5] = NAN
    return out


def nan_pads(planes):
    """The same planes with NaNs in the three pad floats."""
    out = np.array(planes, f32).reshape(-1, 8).copy()
    out[:, 5:8] = NAN
    return out


# ---- Slice, restated -------------------------------------------------------------------------------------------------------------

def pairs(planes, rows, edges=False, spheres=None):
    """Every accepted (plane, prim) pair, plane-major and prims ascending: what SectionAll enumerates -> (owner (m,), prims (m,))."""
    owner, prims = np.nonzero(table(planes, rows, edges, spheres))
    return owner, prims.astype(np.int32)


def slice_expected(normal, offsets, rows, edges=False, spheres=None):
    """RayTracer.Slice by brute force -> (CUT_DTYPE records of kind CUT_SEGMENT, flat; layer offsets (n + 1,) int64)."""
    planes = planes_of(normal, np.asarray(offsets, f32).reshape(-1))
    owner, prims = pairs(planes, rows, edges, spheres)
    c = cuts(planes[owner], prims, rows, edges, spheres)
    keep = c["kind"] == CUT_SEGMENT
    off = np.zeros(planes.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(owner[keep], minlength=planes.shape[0]), out=off[1:])
    return c[keep], off


# ---- the accuracy of a segment ----------------------------------------------------------------------------------------------------
# The residual |n.X - d| / (|n| max|corner|) of an endpoint X of a CUT_SEGMENT record, evaluated in float64: how far off the plane,
# in units of the record's largest |coordinate|, the point the kernel reports lies.  A pair enters when the float64 run of the same
# rule on the same fp32 inputs finds the same kind and the same features; the others ("float64 finds another case": a corner whose
# s changes sign or becomes 0 under fp32 rounding) are counted, and no family may leave out more than EXCLUDED_CAP of its pairs.
EXCLUDED_CAP = 0.01
GRAZE_KS = tuple(range(4, 21))


def _unit_triangles(n, seed, edge=1.0, span=0.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-span, span, (n, 1, 3)) + rng.uniform(-edge / 2, edge / 2, (n, 3, 3))


def _through(tris, seed, frac=None):
    """One plane per triangle with a random normal (not unit): through a random point of its p-range, or, frac given, at that
    fraction of the range below its highest corner.  float64 -> fp32 rows."""
    rng = np.random.default_rng(seed)
    n = tris.shape[0]
    nrm = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1))).astype(f32).astype(np.float64)
    pr = (tris.astype(f32).astype(np.float64) * nrm[:, None, :]).sum(axis=2)
    lo, hi = pr.min(axis=1), pr.max(axis=1)
    f = rng.uniform(0.05, 0.95, n) if frac is None else frac
    return planes_of(nrm, hi - f * (hi - lo))


def margin_families():
    """{name: (rows, planes)}: plane i cuts triangle i.  general: 20 000 triangles of edge about 1 around the origin, a plane
    through each; graze_k: the plane passes a corner at 2^-k of the triangle's extent along n, k = 4 .. 20; slivers: triangles
    whose third corner lies within 2^-10 .. 2^-18 of the opposite edge's line; far: the general family moved 200 to 600 scene
    sizes from the origin."""
    fam = {}
    t = _unit_triangles(20000, 101)
    fam["general"] = (tri_rows(t), _through(t, 102))
    for k in GRAZE_KS:
        t = _unit_triangles(4000, 200 + k)
        fam["graze_%d" % k] = (tri_rows(t), _through(t, 300 + k, frac=2.0 ** -k))
    rng = np.random.default_rng(401)
    t = _unit_triangles(20000, 402)
    w = rng.uniform(0.1, 0.9, (20000, 1))
    t[:, 2] = t[:, 0] + w * (t[:, 1] - t[:, 0]) + rng.normal(size=(20000, 3)) * 2.0 ** -rng.integers(10, 19, (20000, 1))
    fam["slivers"] = (tri_rows(t), _through(t, 403))
    t = _unit_triangles(20000, 501)
    shift = rng.normal(size=(20000, 1, 3))
    shift *= rng.uniform(200.0, 600.0, (20000, 1, 1)) / np.sqrt((shift * shift).sum(axis=2, keepdims=True))
    t = t + shift
    fam["far"] = (tri_rows(t), _through(t, 502))
    return fam


def margin(rows, planes):
    """-> (largest residual, pairs that entered, pairs left out, pairs in all) of a family: plane i against triangle i."""
    n = planes.shape[0]
    prims = np.arange(n)
    c32, c64 = cuts(planes, prims, rows), cuts(planes, prims, rows, dtype=np.float64)
    seg = c32["kind"] == CUT_SEGMENT
    agree = seg & (c64["kind"] == CUT_SEGMENT) & (c64["features"] == c32["features"])
    total = int((seg | (c64["kind"] == CUT_SEGMENT)).sum())
    left_out = total - int(agree.sum())
    A, B, C = corners(rows)
    scale = np.abs(np.concatenate([A, B, C], axis=1)).max(axis=1).astype(np.float64)
    res = residual(c32[agree], planes, prims[agree], scale[agree])
    return float(res.max()), int(agree.sum()), left_out, total


# measured by tests/test_section_expect.py (profiles/section_margin_*.json holds the figure per family)
RESIDUAL_MEASURED = 2.939058e-07          # 4.93 x 2^-24, in graze_16
CUT_SLACK = 2.0 ** -19                    # the smallest power of two >= 4 x RESIDUAL_MEASURED (RT_SWEEP_SLACK's convention)
