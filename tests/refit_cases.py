"""Scenes, moves and checks of the BVH refit tests (test_bvh_refit.py without a device, test_gpu_refit.py on one): the scenes
a tree is built for, the ways their vertices move between two uploads, the tightness of a refitted tree, and a numpy
restatement of rtb::refit that can leave out a step, for the tests of the tests.  Everything is deterministic."""
import numpy as np

import lattice_cases as lc
from query_accel_expect import EMPTY, LEAF, leaf_span, records_of_rows
from query_expect import adversarial_scene

DYADIC_SCALE = 2.0
DYADIC_SHIFT = np.float32([0.5, -0.25, 1.0])     # with the scale: no wall of the moved rooms() lies on a zero coordinate


def scenes():
    return {"rooms": lc.rooms(), "copies": lc.copies()[0], "adversarial37": adversarial_scene(37, 3),
            "adversarial1100": adversarial_scene(1100, 5)}


def dyadic(rows, scale=DYADIC_SCALE, shift=DYADIC_SHIFT):
    """x -> scale x + shift: exact in fp32 for the lattice scenes' coordinates."""
    r = np.array(rows, np.float32).reshape(-1, 4).copy()
    r[:, :3] = r[:, :3] * np.float32(scale) + np.asarray(shift, np.float32)
    return r


def dyadic_rays(rays, scale=DYADIC_SCALE, shift=DYADIC_SHIFT):
    """The rays that see the moved scene as `rays` see the original: o -> scale o + shift, d -> scale d; every t is kept."""
    r = np.array(rays, np.float32).reshape(-1, 6).copy()
    r[:, :3] = r[:, :3] * np.float32(scale) + np.asarray(shift, np.float32)
    r[:, 3:] = r[:, 3:] * np.float32(scale)
    return r


def jitter(rows, seed, amplitude=0.05):
    """Every vertex moved by its own uniform offset in [-amplitude, amplitude]^3."""
    r = np.array(rows, np.float32).reshape(-1, 4).copy()
    r[:, :3] += np.random.default_rng(seed).uniform(-amplitude, amplitude, (r.shape[0], 3)).astype(np.float32)
    return r


def collapse(rows, point=(0.25, -0.5, -3.0)):
    """Every vertex on one point: every triangle degenerate, every box a point."""
    r = np.array(rows, np.float32).reshape(-1, 4).copy()
    r[:, :3] = np.float32(point)
    return r


MOVES = {"dyadic": dyadic, "jitter": lambda rows: jitter(rows, 17), "collapse": collapse}


def swap_with_far(rows):
    """Half the triangles trade places with the triangle farthest from them in upload order's other half: the tree's leaves
    then hold triangles from opposite ends of the scene."""
    t = np.array(rows, np.float32).reshape(-1, 3, 4).copy()
    c = t[:, :, :3].mean(axis=1)
    order = np.argsort(c @ np.float32([1.0, 0.7, 0.4]))          # along one direction through the scene
    half = order.shape[0] // 4
    a, b = order[:half:2], order[-half::2][:order[:half:2].shape[0]]     # every second one of the two outer quarters
    t[np.r_[a, b]] = t[np.r_[b, a]]
    return t.reshape(-1, 4)


# ---- boxes as the builder computes them ---------------------------------------------------------------------------------------

def round_outward(lo, hi):
    """float64 bounds -> fp32, lo towards -inf and hi towards +inf (rtb::detail::round_down / round_up)."""
    with np.errstate(over="ignore"):
        l, h = lo.astype(np.float32), hi.astype(np.float32)
    l = np.where(l.astype(np.float64) > lo, np.nextafter(l, np.float32(-np.inf)), l)
    h = np.where(h.astype(np.float64) < hi, np.nextafter(h, np.float32(np.inf)), h)
    return l.astype(np.float32), h.astype(np.float32)


def triangle_boxes(rows, edges=False):
    """(lo (n, 3), hi (n, 3)) float32: the corners v0, v0 + e1, v0 + e2 of the records in float64, rounded outward."""
    v0, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows, edges))
    with np.errstate(all="ignore"):
        corners = np.stack([v0, v0 + e1, v0 + e2], 1)
    return round_outward(corners.min(axis=1), corners.max(axis=1))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_tight(nodes, recs, info, rows, edges=False):
    """Every leaf child's box is the union of its triangles' outward-rounded boxes and every inner child's box the union of the
    referenced node's four child boxes, bit for bit; cmax is the box's largest |coordinate|.  Returns the children checked."""
    lo, hi = triangle_boxes(rows, edges)
    idx = recs["index"].astype(np.int64)
    checked = 0
    for nd in nodes:
        for c in range(4):
            ref = int(nd["child"][c])
            if ref == EMPTY:
                continue
            if ref & LEAF:
                first, count = leaf_span(ref)
                k = idx[first:first + count]
                elo, ehi = lo[k].min(axis=0), hi[k].max(axis=0)
            else:
                elo, ehi = nodes[ref]["lo"].min(axis=1), nodes[ref]["hi"].max(axis=1)
            assert np.array_equal(_bits(nd["lo"][:, c]), _bits(elo)) and np.array_equal(_bits(nd["hi"][:, c]), _bits(ehi)), (ref, c)
            assert nd["cmax"][c] == np.float32(max(np.abs(elo).max(), np.abs(ehi).max()))
            checked += 1
    return checked


def node_levels(nodes):
    """The level of every node (root 0): children come behind their parents in the array."""
    level = np.zeros(nodes.shape[0], np.int64)
    for i, nd in enumerate(nodes):
        for ref in nd["child"]:
            if ref != EMPTY and not ref & LEAF:
                assert ref > i
                level[ref] = level[i] + 1
    return level


def restated_refit(nodes, recs, info, rows, edges=False, skip_deepest=False, skip_gather=False):
    """rtb::refit in numpy -> (nodes, recs): the gather of the new records by upload index, then the boxes from the deepest
    level up.  skip_deepest leaves the nodes of the last level as they were; skip_gather keeps the old records (the boxes are
    then computed from them)."""
    nodes, recs = nodes.copy(), recs.copy()
    v0, e1, e2 = records_of_rows(rows, edges)
    idx = recs["index"].astype(np.int64)
    if not skip_gather:
        recs["v0"], recs["e1"], recs["e2"] = v0[idx], e1[idx], e2[idx]
    with np.errstate(all="ignore"):
        a = recs["v0"].astype(np.float64)
        corners = np.stack([a, a + recs["e1"], a + recs["e2"]], 1)
    lo, hi = round_outward(corners.min(axis=1), corners.max(axis=1))         # per record slot
    level = node_levels(nodes)
    for i in range(nodes.shape[0] - 1, -1, -1):
        if skip_deepest and level[i] == level.max():
            continue
        for c in range(4):
            ref = int(nodes[i]["child"][c])
            if ref == EMPTY:
                continue
            if ref & LEAF:
                first, count = leaf_span(ref)
                blo, bhi = lo[first:first + count].min(axis=0), hi[first:first + count].max(axis=0)
            else:
                blo, bhi = nodes[ref]["lo"].min(axis=1), nodes[ref]["hi"].max(axis=1)
            nodes[i]["lo"][:, c], nodes[i]["hi"][:, c] = blo, bhi
            nodes[i]["cmax"][c] = max(np.abs(blo).max(), np.abs(bhi).max())
    return nodes, recs


def same_tree(a, b):
    """Two (nodes, records, ...) tuples hold the same bytes."""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
