"""Test side of the opt-in BVH of the ray queries (RT_QUERY_BVH): the contract's conditioning of a scan winner and the
exclusion rule built on it, the three ray populations of the device comparison, structural checks of a dumped tree, and a
numpy restatement of the traversal's fp32 box test that walks such a tree without a GPU."""
import ctypes as C

import numpy as np

from query_expect import FLT_MAX, HIT_DTYPE
from tree_walk_expect import EMPTY, LEAF, keys_of, leaf_span, note_box_arithmetic, note_high_water, ray_slab, walk  # noqa: F401  (re-exported)

RHO = np.float32(2.0 ** -8)            # RT_BVH_RHO (csrc/rt_kernels.hpp)
WELL_CONDITIONED = 2.0 ** -10          # the contract's bound on det / (|d| |e1| |e2|), include/rt_mi355x.h
EXCLUSION_CAP = 1e-3                   # at most this fraction of a population may use the exclusion


def records_of_rows(rows, edges=False):
    """(v0, e1, e2) as the kernel holds them: fp32 differences of absolute vertices, or the rows of the edge layout."""
    t = np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3]
    if edges:
        return t[:, 0], t[:, 1], t[:, 2]
    return t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]


def conditioning(rays, rows, prim, edges=False):
    """det / (|d| |e1| |e2|) in float64 of each ray with its winner `prim` (inf where the winner is no triangle)."""
    v0, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows, edges))
    prim = np.asarray(prim, np.int64)
    out = np.full(prim.shape, np.inf)
    m = (prim >= 0) & (prim < v0.shape[0])
    d = np.asarray(rays, np.float32).reshape(-1, 6)[m, 3:].astype(np.float64)
    a, b = e1[prim[m]], e2[prim[m]]
    with np.errstate(all="ignore"):
        det = np.einsum("ij,ij->i", a, np.cross(d, b))
        r = det / (np.linalg.norm(d, axis=1) * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    out[m] = np.where(np.isnan(r), -np.inf, r)          # a NaN ratio is not a well-conditioned one
    return out


def check_against_scan(got, scan, rays, rows, edges=False, label=""):
    """The exclusion rule: `got` (BVH) equals `scan` bit for bit, except for rays whose SCAN winner is not well conditioned,
    and those are at most EXCLUSION_CAP of the population.  Prints and returns how many rays used the exclusion."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    s = np.ascontiguousarray(scan).view(np.uint32).reshape(-1, 4)
    assert g.shape == s.shape
    differ = (g != s).any(axis=1)
    ratio = conditioning(rays, rows, scan["prim"], edges)
    bad = np.nonzero(differ & ~(ratio < WELL_CONDITIONED))[0]
    used = int((differ & (ratio < WELL_CONDITIONED)).sum())
    print("%s: %d rays, %d differ, %d excluded (scan winner below 2^-10), smallest winner ratio %.3g"
          % (label, g.shape[0], int(differ.sum()), used, float(np.min(ratio[np.isfinite(ratio)], initial=np.inf))))
    assert bad.size == 0, (label, bad[:5], got[bad[:5]], scan[bad[:5]], ratio[bad[:5]])
    assert used <= EXCLUSION_CAP * g.shape[0], (label, used)
    return used


def populations(rows, n, seed):
    """The three ray populations of the device comparison, n rays each, as {name: (n, 6) float32}: (i) origins uniform in
    [-2, 2]^3 aimed at triangle centroids + N(0, 0.05), directions times +1, -1 or 0.37; (ii) the same targets from origins
    1000 x farther out; (iii) rays from the world origin to the same targets."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3]
    org = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    tgt = (tris[rng.integers(0, tris.shape[0], n)].mean(axis=1) + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    scale = rng.choice(np.float32([1.0, -1.0, 0.37]), (n, 1)).astype(np.float32)
    far = org * np.float32(1000.0)
    zero = np.zeros_like(org)
    return {"near": np.ascontiguousarray(np.c_[org, (tgt - org) * scale], np.float32),
            "far": np.ascontiguousarray(np.c_[far, (tgt - far) * scale], np.float32),
            "origin": np.ascontiguousarray(np.c_[zero, tgt * scale], np.float32)}


# ---- the dumped tree ----------------------------------------------------------------------------------------------------

def check_tree(nodes, recs, info, rows, edges=False):
    """Every finite triangle in exactly one leaf with its upload index, the non-finite ones only in the always-tested list;
    every leaf box holds its records' corners (float64); every child box lies inside its parent's; depth within the bound."""
    v0, e1, e2 = records_of_rows(rows, edges)
    n = v0.shape[0]
    assert recs.shape[0] == n and sorted(recs["index"].tolist()) == list(range(n))
    idx = recs["index"].astype(np.int64)
    assert np.array_equal(recs["v0"].view(np.uint32), v0[idx].view(np.uint32))
    assert np.array_equal(recs["e1"].view(np.uint32), e1[idx].view(np.uint32))
    assert np.array_equal(recs["e2"].view(np.uint32), e2[idx].view(np.uint32))
    assert not recs["pad"].any()
    with np.errstate(all="ignore"):
        corners = np.stack([v0.astype(np.float64), v0.astype(np.float64) + e1, v0.astype(np.float64) + e2], 1)   # (n, 3, 3)
    rec_finite = np.isfinite(np.c_[v0, e1, e2]).all(axis=1) & (np.abs(corners).max(axis=(1, 2)) <= float(FLT_MAX))
    n_leaf = n - info["always_tested"]
    always = idx[n_leaf:]
    assert not rec_finite[always].any() and rec_finite[idx[:n_leaf]].all()
    assert np.array_equal(always, np.sort(always))
    assert info["nodes"] == nodes.shape[0] and (nodes.shape[0] > 0) == (n_leaf > 0)
    assert info["depth"] <= info["depth_bound"]
    seen = np.zeros(n_leaf, np.int32)
    leaves, depth = 0, 0
    todo = [(0, 1, None)] if nodes.shape[0] else []
    visited = 0
    while todo:
        ni, level, box = todo.pop()
        visited += 1
        depth = max(depth, level)
        nd = nodes[ni]
        for c in range(4):
            ref = int(nd["child"][c])
            lo, hi = nd["lo"][:, c].astype(np.float64), nd["hi"][:, c].astype(np.float64)
            if ref == EMPTY:
                assert (nd["lo"][:, c] == np.inf).all() and (nd["hi"][:, c] == -np.inf).all()
                continue
            assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
            assert nd["cmax"][c] == np.float32(max(np.abs(lo).max(), np.abs(hi).max()))
            if box is not None:
                assert (box[0] <= lo).all() and (hi <= box[1]).all()
            if ref & LEAF:
                first, count = leaf_span(ref)
                assert 1 <= count <= 4 and first + count <= n_leaf
                seen[first:first + count] += 1
                leaves += 1
                k = idx[first:first + count]
                assert (np.diff(k) > 0).all()
                assert (corners[k].min(axis=1) >= lo).all() and (corners[k].max(axis=1) <= hi).all()
            else:
                assert ref < nodes.shape[0]
                todo.append((ref, level + 1, (lo, hi)))
    assert (seen == 1).all() and visited == nodes.shape[0]
    assert leaves == info["leaves"] and depth == info["depth"]
    return depth


# ---- the traversal's box test, restated -----------------------------------------------------------------------------------

def walk_tree(orc, nodes, recs, info, rays, rows, contract=None, nearest=False, rho=RHO, tie_rule=True, strict=True, stats=None):
    """query_bvh_kernel in numpy: the fp32 box test of csrc/rt_bvh.hpp operation by operation, the order-free hit rule, the
    oracle's HitTriangle on the leaves' triangles (absolute rows).  Returns (HIT_DTYPE array, triangle tests made).
    Switches that break one rule each, for tests of the tests: tie_rule=False drops "equal t: the lower upload index wins" (the
    first visited keeps a tie); strict=False prunes and drops a child whose goodness EQUALS the best t.  stats: a dict that
    receives note_box_arithmetic's counters and note_high_water's marks."""
    contract = orc.FMA if contract is None else contract
    L = orc.lib()
    fp = C.POINTER(C.c_float)
    tris = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3])
    rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 6))
    n_leaf = recs.shape[0] - info["always_tested"]
    index = recs["index"].astype(np.int64)
    out = np.zeros(rays.shape[0], HIT_DTYPE)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    f32 = np.float32
    tests = 0
    cap = 3 * max(info["depth"], 1)
    with np.errstate(all="ignore"):
        for i in range(rays.shape[0]):
            ray = rays[i].ctypes.data_as(fp)
            o, d = rays[i, :3], rays[i, 3:]
            finite = bool(np.isfinite(rays[i]).all())
            inv = f32(1.0) / d
            omax = np.abs(o).max()
            state = {"t": FLT_MAX if nearest else -FLT_MAX, "i": -1, "u": f32(0), "v": f32(0)}

            def test(j):
                a, b, c = tris[j]
                if not L.orc_hit_triangle(ray, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp), contract, 0,
                                          C.byref(t), C.byref(u), C.byref(v)):
                    return
                tj = f32(t.value)
                better = (tj > 0 and tj < state["t"]) if nearest else (state["t"] < tj)
                if better or (tie_rule and tj == state["t"] and j < state["i"]):
                    state.update(t=tj, i=int(j), u=f32(u.value), v=f32(v.value))

            seen = {}

            def lim():
                return -state["t"] if nearest else state["t"]

            def stale(g):
                return (g < lim()) if strict else (g <= lim())

            def leaf(k):
                nonlocal tests
                tests += 1
                test(index[k])

            def child(nd):
                enter, exit_, nan, t1, t2 = ray_slab(nd, o, inv, omax, rho)
                good = -enter if nearest else exit_
                skip = (exit_ < enter) | stale(good) | (nearest & (exit_ <= 0))
                note_box_arithmetic(stats, seen, t1, t2, nd["child"] != EMPTY)
                return keys_of(good, finite & ~nan, skip)

            mark, _ = walk(nodes, cap, True, child, leaf, stale)
            note_high_water(stats, mark)
            for j in index[n_leaf:]:
                tests += 1
                test(j)
            out[i] = (state["t"], state["u"], state["v"], state["i"]) if state["i"] >= 0 else (0, 0, 0, -1)
    return out, tests
