"""The traversal every tree-walking query's restatement shares, stated once: rt_bvh_walk.hpp's bvh_walk(child, leaf, stale) in
plain Python over a dumped tree (nodes, recs, info of api.bvh_build / query_tree), one query (one lane) per call, with the two
fp32 child-box arithmetics of the kernels in numpy, operation by operation, and the helpers that note a walk's stats.  The
candidate rule, the list, the cursor, the spheres, the always-tested list and the count of records tested stay with each query's
own module (query_accel_expect, allhits_expect, occluded_expect, closest_expect, nearest_expect, tridistance_expect,
overlap_expect, spherecast_expect).  A helper, not a test.  Everything is deterministic and needs no device."""
import numpy as np

from query_expect import FLT_MAX

f32 = np.float32
EMPTY, LEAF = 0xFFFFFFFF, 0x80000000
DEFLATE = f32(1.0 - 2.0 ** -21)         # the factor on a box's squared gap (csrc/rt_closest.hpp)


def leaf_span(ref):
    return int(ref & 0x0FFFFFFF), int((ref >> 28) & 3) + 1


# ---- the walk --------------------------------------------------------------------------------------------------------------

def walk(nodes, cap, start, child, leaf, stale=None, enforce_cap=True):
    """One query's walk from the root (start; False: nothing is visited) -> (mark, overflow): the largest number of entries
    that waited on its stack, and whether a push found the stack full.
      child(nd)   -> per child slot None (skipped) or a key: +inf takes no pruning decision, anything else is clamped to
                  >= -FLT_MAX, the larger the earlier.  Empty references are ignored here, whatever their key.  The survivors
                  are ordered by a STABLE sort by descending key (equal keys stay in slot order), the first is entered and the
                  others wait, the better of them on top.
      leaf(k)     tests the record at position k of recs (the caller knows its upload index, recs["index"][k]); True ends the
                  walk (an any-hit query).
      stale(key)  makes the entries keyed: a popped entry for which it is true is dropped.  None: unkeyed entries.
    enforce_cap=True asserts that the stack never holds more than `cap` entries (3 x the tree's depth always suffice; the deep
    tests pass a smaller one and expect the AssertionError); False drops a push beyond cap and reports overflow, which is the
    region kernel's stack_cap behaviour."""
    stack, mark, overflow = [], 0, False
    cur = 0 if (nodes.shape[0] and start) else EMPTY
    while True:
        if cur == EMPTY:
            if not stack:
                break
            key, cur = stack.pop()
            if stale is not None and stale(key):
                cur = EMPTY
                continue
        if cur & LEAF:
            first, count = leaf_span(cur)
            for k in range(first, first + count):
                if leaf(k):
                    return mark, overflow
            cur = EMPTY
            continue
        nd = nodes[cur]
        keys = child(nd)
        kids = [(np.fmax(keys[c], -FLT_MAX), int(nd["child"][c])) for c in range(4)
                if int(nd["child"][c]) != EMPTY and keys[c] is not None]
        kids.sort(key=lambda k: -k[0])
        cur = kids[0][1] if kids else EMPTY
        for k in reversed(kids[1:]):
            if enforce_cap or len(stack) < cap:
                stack.append(k)
            else:
                overflow = True
        assert len(stack) <= cap
        mark = max(mark, len(stack))
    return mark, overflow


# ---- the two child-box arithmetics -----------------------------------------------------------------------------------------

def slab(nd, o, inv, pad):
    """bvh_slab for a node's four children at once: the line o + t / inv against each box grown by the caller's pad (4,).
    -> (enter, exit_, nan, t1, t2): (4,) enter and exit, (4,) bool "a NaN among the six products", and the products (3, 4)."""
    t1 = ((nd["lo"] - pad) - o[:, None]) * inv[:, None]               # (3, 4)
    t2 = ((nd["hi"] + pad) - o[:, None]) * inv[:, None]
    assert t1.dtype == np.float32 and pad.dtype == np.float32
    nan = (np.isnan(t1) | np.isnan(t2)).any(axis=0)
    enter = np.fmax.reduce(np.fmin(t1, t2), axis=0)
    exit_ = np.fmin.reduce(np.fmax(t1, t2), axis=0)
    return enter, exit_, nan, t1, t2


def ray_slab(nd, o, inv, omax, rho):
    """slab with the ray queries' pad = rho * (omax + cmax)."""
    return slab(nd, o, inv, rho * (omax + nd["cmax"]))


def box_gap_lb(nd, qmin, qmax, qabs, rho_c):
    """The lower bound (4,) on the squared distance from the query's bounding box [qmin, qmax] (qabs: its largest |coordinate|)
    to each child box: per axis the gap between the boxes less pad = rho_c * (qabs + cmax), not below 0; the sum of the squares
    times DEFLATE.  A point p is the box qmin = qmax = p with qabs = max|p|: the same operations on the same operands as the
    point kernels' form."""
    zero = f32(0)
    pad = rho_c * (qabs + nd["cmax"])                                                                        # (4,) float32
    gap = np.fmax(np.fmax(np.fmax(nd["lo"] - qmax[:, None], qmin[:, None] - nd["hi"]), zero) - pad, zero)    # (3, 4)
    lb = ((gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2]) * DEFLATE
    assert lb.dtype == f32 and pad.dtype == f32
    return lb


def keys_of(good, decided, skip):
    """child()'s answer from a node's four goodness values: None where a decided child is skipped, +inf where nothing is
    decided, the goodness elsewhere."""
    return [None if (decided[c] and skip[c]) else (good[c] if decided[c] else f32(np.inf)) for c in range(4)]


# ---- what a walk notes -----------------------------------------------------------------------------------------------------

def note_box_arithmetic(stats, seen, t1, t2, present):
    """Into the dict `stats` of a walk (if given): which branches of the box test this node's present children reach.  seen is
    the ray's own {"nan": bool, "inf": bool}; stats counts rays ("nan_rays", "inf_rays") and child boxes ("nan_boxes",
    "inf_boxes") whose t1, t2 hold a NaN (0 * inf: the ray runs inside a slab's plane) or an infinity (parallel, outside)."""
    if stats is None or (np.isfinite(t1).all() and np.isfinite(t2).all()):
        return
    for key, bad in (("nan", np.isnan(t1) | np.isnan(t2)), ("inf", np.isinf(t1) | np.isinf(t2))):
        boxes = int((bad.any(axis=0) & present).sum())
        stats[key + "_boxes"] = stats.get(key + "_boxes", 0) + boxes
        if boxes and not seen.get(key):
            seen[key] = True
            stats[key + "_rays"] = stats.get(key + "_rays", 0) + 1


def note_high_water(stats, mark):
    """Into the dict `stats` of a walk (if given): `mark`, the largest number of entries this ray's or point's stack held, is
    appended to stats["high_water_per"] (one per ray or point, in order; 0 for one that never walks), and stats["high_water"]
    is the largest of them.  A kernel lane whose capacity is below its mark takes the overflow path."""
    if stats is not None:
        stats.setdefault("high_water_per", []).append(int(mark))
        stats["high_water"] = max(stats.get("high_water", 0), int(mark))
