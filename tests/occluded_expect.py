"""Test side of the visibility query (RayTracer.Occluded / rt_tracer_occluded): what every ray must answer, computed as an OR
over every primitive with the oracle's HitTriangle and ray-sphere test and the closed fp32 interval; the any-hit form of the
BVH contract (include/rt_mi355x.h) with its exclusion; the interval families of the tests; and a numpy restatement of the
any-hit traversal that walks a dumped tree without a GPU."""
import ctypes as C

import numpy as np

from query_accel_expect import RHO, WELL_CONDITIONED, records_of_rows
from tree_walk_expect import EMPTY, keys_of, note_box_arithmetic, note_high_water, ray_slab, walk

INF = np.float32(np.inf)


def hit_table(orc, rays, tri_rows, spheres=None, contract=None):
    """Per ray and primitive (triangles in upload order, then spheres): (hit (n, P) bool, t (n, P) float32) of the oracle's
    HitTriangle on absolute triangle rows (3N, 4) and of its ray-sphere test.  rays: (n, 6) or the first six columns of
    (n, 8) segments."""
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
    tt = np.zeros(hit.shape, np.float32)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    rt, ru, rv = C.byref(t), C.byref(u), C.byref(v)
    for i in range(rays.shape[0]):
        ray = rays[i].ctypes.data_as(fp)
        for j, (a, b, c) in enumerate(verts):
            if L.orc_hit_triangle(ray, a, b, c, contract, 0, rt, ru, rv):
                hit[i, j] = True
                tt[i, j] = t.value
        for s, sp in enumerate(sphs):
            if L.orc_hit_sphere(ray, sp, contract, rt):
                hit[i, nt + s] = True
                tt[i, nt + s] = t.value
    return hit, tt


def in_interval(segs, table):
    """(n, P) bool: primitive p is hit by ray i with tmin <= t <= tmax -- fp32 comparisons, so a NaN t or bound is False."""
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    hit, t = table
    with np.errstate(invalid="ignore"):
        return hit & (segs[:, 6:7] <= t) & (t <= segs[:, 7:8])


def expected_occluded(orc, segs, tri_rows, spheres=None, contract=None, table=None):
    """The OR over every primitive, as (n,) bool.  table: a hit_table of the same rays (the intervals may differ), to reuse."""
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    if table is None:
        table = hit_table(orc, segs, tri_rows, spheres, contract)
    return in_interval(segs, table).any(axis=1)


def conditioning_matrix(rays, tri_rows):
    """det / (|d| |e1| |e2|) in float64 for every (ray, triangle), from the records the kernel intersects; NaN -> -inf."""
    _, e1, e2 = (x.astype(np.float64) for x in records_of_rows(tri_rows))
    d = np.asarray(rays, np.float32)[:, 3:6].astype(np.float64)
    with np.errstate(all="ignore"):
        det = np.einsum("tj,rtj->rt", e1, np.cross(d[:, None, :], e2[None, :, :]))
        r = det / (np.linalg.norm(d, axis=1)[:, None] * (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))[None, :])
    return np.where(np.isnan(r), -np.inf, r)


def in_interval_conditioning(orc, segs, tri_rows, spheres=None, contract=None, table=None):
    """Per ray: some accepted in-interval occluder is a sphere, or a triangle that is well conditioned (ratio >= 2^-10 in
    float64).  For such a ray the BVH must give the scan's answer."""
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    rows = np.asarray(tri_rows, np.float32).reshape(-1, 3, 4)
    nt = rows.shape[0]
    out = np.zeros(segs.shape[0], bool)
    for i in range(segs.shape[0]):                                       # ray by ray: the oracle sees the candidates only
        seg = segs[i:i + 1]
        cand = np.nonzero(conditioning_matrix(seg, tri_rows)[0] >= WELL_CONDITIONED)[0]
        if table is not None:
            inside = in_interval(seg, (table[0][i:i + 1], table[1][i:i + 1]))[0]
            out[i] = inside[nt:].any() or inside[cand].any()
        else:
            out[i] = (spheres is not None and expected_occluded(orc, seg, rows[:0].reshape(-1, 4), spheres, contract)[0]) or \
                     expected_occluded(orc, seg, rows[cand].reshape(-1, 4), None, contract)[0]
    return out


def check_bvh_occluded(got, scan, segs, tri_rows, orc, spheres=None, contract=None, table=None, cap=None, label=""):
    """The any-hit BVH contract for every ray: BVH = 1 implies scan = 1; BVH = scan when scan = 0; BVH = scan when an
    in-interval occluder is well conditioned or a sphere.  The oracle is asked only about the rays that differ.  Returns (and
    prints) how many rays used the exclusion; cap: at most this fraction of the rays may."""
    got, scan = np.asarray(got).astype(bool).ravel(), np.asarray(scan).astype(bool).ravel()
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    assert got.shape == scan.shape == (segs.shape[0],)
    invented = np.nonzero(got & ~scan)[0]
    assert invented.size == 0, (label, "the BVH reports occluders the scan does not", invented[:5], segs[invented[:5]])
    lost = np.nonzero(scan & ~got)[0]
    if cap is not None:                                                  # (before the oracle is asked about each of them)
        assert lost.size <= cap * segs.shape[0], (label, lost.size)
    if lost.size:
        sub = None if table is None else (table[0][lost], table[1][lost])
        must = in_interval_conditioning(orc, segs[lost], tri_rows, spheres, contract, sub)
        assert not must.any(), (label, "a well-conditioned occluder was lost", lost[must][:5], segs[lost[must][:5]])
    print("%s: %d rays, %.1f %% occluded, %d excluded (every in-interval occluder below 2^-10)"
          % (label, segs.shape[0], 100.0 * scan.mean() if scan.size else 0.0, lost.size))
    return int(lost.size)


def interval_families(rays, seed):
    """Four intervals per ray, as {name: (n, 8) float32 segments}."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    hi = lo + rng.uniform(0.0, 1.5, n).astype(np.float32)
    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    fam = {"unit": (zero, one), "forward": (np.full(n, 1e-3, np.float32), np.full(n, INF)),
           "any": (np.full(n, -INF), np.full(n, INF)), "window": (lo, hi)}
    return {k: np.ascontiguousarray(np.c_[rays, a, b], np.float32) for k, (a, b) in fam.items()}


def with_interval(rays, tmin, tmax):
    """(n, 8) segments of (n, 6) rays and per-ray (or scalar) bounds."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    out = np.empty((rays.shape[0], 8), np.float32)
    out[:, :6], out[:, 6], out[:, 7] = rays, tmin, tmax
    return out


# ---- the any-hit traversal, restated -------------------------------------------------------------------------------------

def walk_tree_occluded(orc, nodes, recs, info, segs, rows, spheres=None, contract=None, rho=RHO, strict=True, stats=None,
                       kernel_order=False):
    """occluded_bvh_kernel in numpy: spheres, the always-tested list, then the tree with the fp32 box test of
    csrc/rt_occluded.hpp operation by operation -- a child is skipped when exit < enter, exit < tmin or enter > tmax, unless
    the ray has a non-finite component or a zero direction or the child's arithmetic holds a NaN -- and the oracle's
    HitTriangle on the leaves' triangles (absolute rows).  The order of the visits does not change an OR, so the children are
    entered as stored.  Returns ((n,) bool, triangle tests made).  strict=False (for tests of the tests) also skips a child whose
    exit EQUALS tmin or whose enter EQUALS tmax; stats: a dict that receives note_box_arithmetic's counters and
    note_high_water's marks -- the entries that WAIT: one of a node's children is entered at once and the others are stacked.
    "As stored" is the order of a walk that stacks all of a node's children slot by slot and pops one: the LAST stored slot is
    entered first, which tree_walk_expect.walk gives with the slot as the key.  kernel_order: the children are entered
    in the kernel's order -- the largest overlap of the child's span with the interval first, +inf where nothing is decided --
    which is what the marks of a device lane follow; the answer is the same OR."""
    contract = orc.FMA if contract is None else contract
    L = orc.lib()
    fp = C.POINTER(C.c_float)
    tris = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3])
    sph = np.ascontiguousarray(np.zeros((0, 4), np.float32) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4))
    segs = np.ascontiguousarray(np.asarray(segs, np.float32).reshape(-1, 8))
    n_leaf = recs.shape[0] - info["always_tested"]
    index = recs["index"].astype(np.int64)
    out = np.zeros(segs.shape[0], bool)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    f32 = np.float32
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(segs.shape[0]):
            ray = segs[i].ctypes.data_as(fp)
            o, d, tmin, tmax = segs[i, :3], segs[i, 3:6], segs[i, 6], segs[i, 7]

            def inside():
                tj = f32(t.value)
                return bool(tmin <= tj) and bool(tj <= tmax)

            def test(j):
                a, b, c = tris[j]
                return bool(L.orc_hit_triangle(ray, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp), contract, 0,
                                               C.byref(t), C.byref(u), C.byref(v))) and inside()

            done = any(L.orc_hit_sphere(ray, s.ctypes.data_as(fp), contract, C.byref(t)) and inside() for s in sph)
            for j in index[n_leaf:]:
                if done:
                    break
                tests += 1
                done = test(j)
            prunes = bool(np.isfinite(segs[i, :6]).all()) and bool((d != 0).any())
            inv = f32(1.0) / d
            omax = np.abs(o).max()
            seen = {}

            def leaf(k):
                nonlocal tests, done
                tests += 1
                done = test(index[k])
                return done

            def child(nd):
                enter, exit_, nan, t1, t2 = ray_slab(nd, o, inv, omax, rho)
                skip = (exit_ < enter) | (exit_ < tmin) | (enter > tmax)
                if not strict:
                    skip |= (exit_ == tmin) | (enter == tmax)
                note_box_arithmetic(stats, seen, t1, t2, nd["child"] != EMPTY)
                decided = prunes & ~nan
                if kernel_order:                                         # (equal overlaps are entered in slot order)
                    return keys_of(np.fmin(exit_, tmax) - np.fmax(enter, tmin), decided, skip)
                return [None if (decided[c] and skip[c]) else f32(c) for c in range(4)]      # the slot is the key: the last first

            mark, _ = walk(nodes, cap, not done, child, leaf)
            note_high_water(stats, mark)
            out[i] = done
    return out, tests
