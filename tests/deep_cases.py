"""Scenes and populations that drive the query BVH to its depth bound (test_bvh_deep.py without a device,
test_gpu_query_deep.py on one): a ladder of triangle clusters whose sizes and distances from the origin grow geometrically, so
that the binned SAH peels a few triangles off one end at every level and the builder's median rule has to finish the tree inside
kBvhMaxBinaryDepth; its moved versions for the refit; and rays, segments, points and exposure points whose walks hold a stack
as full as a tree of 16 levels allows.  A helper, not a test.  Everything is deterministic and needs no device."""
import numpy as np

import refit_cases as rc
from closest_expect import with_radius
from lattice_cases import ray_segments
from query_expect import edge_rows

f32 = np.float32
INF = f32(np.inf)
AXIS = np.array([1.0, 0.0, -5.0])              # cluster k sits around s AXIS, s = S0 ratio^k
# The smallest scale.  The ray queries' hit arithmetic is cubic in a record's size (t = e2 . ((o - v0) x e1) / det): beyond
# about 2^42 it overflows fp32, and the exact test then reports t = +inf for triangles BEHIND a ray -- answers that follow
# no geometry, so no box test can reproduce them (a ladder of 60 steps from 2^-12 reaches 2^47; test_bvh_deep.py shows both the
# overflow and the walk that disagrees with the scan there).  From 2^-28 the largest of 70 clusters sits at 2^41 and every
# product stays finite; the clusters below about 2^-14 are smaller than the hit rule's det < 1e-10 cull lets through, so rays
# pass through them while points still find them.  The scene is scale-invariant about the origin and the factor is a power of
# two, so a ladder's tree is the same tree at any such scale.
S0 = 2.0 ** -28
S0_OVERFLOWING = 2.0 ** -12
DEPTH_BOUND = 16                               # rtb::kBvhMaxDepth
# The scene the tests keep.  The SAH peels about one cluster per binary level off the large end, so the tree's depth grows with
# the ladder's span: 60 steps give 32 binary levels (16 of 4-wide nodes) by the SAH alone -- the bound is met, the builder's
# median rule never fires; with 70 steps the SAH alone goes on to 35 (seed 4; 33 to 35 over seeds 1..4), the rule fires, and
# the tree stops at 32 (test_bvh_deep.py builds both ways with the builder's own code).  The median splits the rule forces
# are balanced, every node on the deepest path then has four children, and every restated walk of the populations below
# holds a FULL stack, 48 of 48 entries, on the mirrored ladder; on the plain one every walk but the any-hit one does.
KEPT = dict(per=32, steps=70, ratio=2.0, seed=4, spread=0.05, s0=S0)


def scale_ladder(per, steps, ratio, seed, spread, mirror=False, s0=S0):
    """(3 per steps, 4) float32 upload rows: `steps` clusters of `per` triangles.  Cluster k has the scale s = s0 ratio^k:
    every triangle's centre is s AXIS + spread s U(-1, 1)^3 and its vertices are the centre + 0.2 s U(-1, 1)^3.  The scene is
    scale-invariant about the origin: sizes and distances run from s0 to s0 ratio^(steps - 1).
    mirror: the same scene reflected in the plane z = 0.  The builder cuts along z and puts the lower side first, so the
    subtree that goes on to the full depth -- the small clusters -- is a node's LAST child in the plain ladder and its FIRST in
    the mirrored one: a walk that takes no pruning decision enters the children as stored, and only in the mirrored tree does
    it enter the deep child while its three siblings wait."""
    rng = np.random.default_rng(seed)
    s = s0 * float(ratio) ** np.arange(steps)
    centre = AXIS[None, None, :] + spread * rng.uniform(-1.0, 1.0, (steps, per, 3))
    v = centre[:, :, None, :] + 0.2 * rng.uniform(-1.0, 1.0, (steps, per, 3, 3))
    v = v * s[:, None, None, None]
    if mirror:
        v[..., 2] = -v[..., 2]
    rows = np.zeros((steps * per, 3, 4), f32)
    rows[:, :, :3] = v.reshape(-1, 3, 3)
    return rows.reshape(-1, 4)


def scales(**kw):
    """The clusters' scales s of a ladder's parameters (KEPT by default)."""
    k = dict(KEPT, **kw)
    return k.get("s0", S0) * float(k["ratio"]) ** np.arange(k["steps"])


def _reflect(a, cols, kw):
    """The population of the mirrored ladder: the z of every origin, direction or normal (columns `cols`) negated."""
    if kw.get("mirror"):
        a[:, cols] = -a[:, cols]
    return np.ascontiguousarray(a, f32)


def deep_scene(edges=False, **kw):
    """The kept ladder (or one with some parameters replaced) in either upload layout."""
    rows = scale_ladder(**dict(KEPT, **kw))
    return edge_rows(rows) if edges else rows


def doubled(rows):
    """The scene times 2: exact in fp32 for every coordinate, so every bit of the refitted tree follows from the built one."""
    return rc.dyadic(rows, 2.0, f32([0.0, 0.0, 0.0]))


def doubled_boxes(nodes):
    """A tree's nodes with every box and cmax times 2: what a refit to doubled() must give, bit for bit."""
    out = nodes.copy()
    for k in ("lo", "hi", "cmax"):
        out[k] = out[k] * f32(2.0)                                        # (an absent child's +-inf stays)
    return out


def jittered(rows, seed=23):
    """refit_cases.jitter scaled to the ladder: every vertex moves by up to 5 % of its own distance from the origin (an absolute
    0.05 would bury the small clusters), so clusters overlap their neighbours and the refitted boxes are loose."""
    r = np.array(rows, f32).reshape(-1, 4).copy()
    amp = 0.05 * np.abs(r[:, :3]).max(axis=1, keepdims=True)
    r[:, :3] += (np.random.default_rng(seed).uniform(-1.0, 1.0, (r.shape[0], 3)) * amp).astype(f32)
    return r


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def rays(seed=31, **kw):
    """(m, 6) float32 rays of the kept ladder, a couple of hundred, unit directions unless said otherwise:
    along the axis from c s AXIS (c = 0.5, 2, -1) at several scales, towards and away from the origin, slightly tilted so that
    they cross triangles, and on the axis itself; from beside the world origin through the smallest cluster; from origins at
    about 2^44, whose pad swallows every small box, towards the clusters; from inside the smallest cluster in random
    directions; axis-parallel rays through cluster centres; rays of direction zero; rays with one NaN, +inf or -inf component
    (they take no pruning decision: every child is visited, in the order stored)."""
    rng = np.random.default_rng(seed)
    s = scales(**kw)
    a = _unit(AXIS)
    out = []
    pick = s[[0, 1, len(s) // 4, len(s) // 2, 3 * len(s) // 4, len(s) - 2, len(s) - 1]]
    for sk in pick:
        for c in (0.5, 2.0, -1.0):
            for sign in (1.0, -1.0):
                for _ in range(2):
                    d = _unit(sign * a + 0.02 * rng.uniform(-1, 1, 3))
                    out.append(np.r_[c * sk * AXIS, d])
    for o, sign in ((0.0, 1.0), (0.5 * s[0], 1.0), (-s[0], 1.0), (-s[-1], 1.0), (2.0 * s[-1], -1.0), (0.5 * s[0], -1.0),
                    (s[len(s) // 2], 1.0), (s[len(s) // 2], -1.0)):
        out.append(np.r_[o * AXIS, sign * a])                             # on the axis itself: no cluster's box is missed
    for k in range(48):                                                   # from beside the world origin through the smallest
        o = s[0] * ((0.0, 0.5, -1.0, -4.0)[k % 4] * AXIS + 0.01 * rng.uniform(-1, 1, 3))     # cluster and on through them all
        tgt = s[0] * (AXIS + 0.12 * rng.uniform(-1, 1, 3))
        out.append(np.r_[o, _unit(tgt - o)])
    far = 2.0 ** 44
    for k in range(24):
        o = far * _unit(rng.normal(0, 1, 3)) if k % 3 else far * a * (1 if k % 2 else -1)
        tgt = s[rng.integers(0, len(s))] * (AXIS + 0.05 * rng.uniform(-1, 1, 3))
        out.append(np.r_[o, _unit(tgt - o)])
    for _ in range(24):
        o = s[0] * (AXIS + 0.05 * rng.uniform(-1, 1, 3))
        out.append(np.r_[o, _unit(rng.normal(0, 1, 3))])
    for k in range(18):
        sk = s[rng.integers(0, len(s))]
        d = np.zeros(3)
        d[k % 3] = 1.0 if k % 2 else -1.0
        o = sk * (AXIS + 0.05 * rng.uniform(-1, 1, 3)) - 3.0 * sk * d
        out.append(np.r_[o, d])
    for k in range(8):
        o = s[(k * 7) % len(s)] * AXIS if k else np.zeros(3)
        out.append(np.r_[o, np.zeros(3)])
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            r = np.r_[0.5 * s[0] * AXIS, a]
            r[k] = bad
            out.append(r)
    return _reflect(np.asarray(out, f32), [2, 5], kw)


def segments(r=None, **kw):
    """The rays as (m, 8) segments with lattice_cases.ray_segments' intervals by turns, then the same rays inactive (tmin > tmax)
    for the first eight."""
    r = rays(**kw) if r is None else r
    segs = ray_segments(r)
    dead = segs[:8].copy()
    dead[:, 6], dead[:, 7] = 1.0, 0.5
    return np.ascontiguousarray(np.concatenate([segs, dead]), f32)


def points(seed=37, **kw):
    """(m, 4) float32 {x, y, z, d2max}: cluster centres at several scales, the origin, points beside the axis and points far
    outside (2^50, 2^55), each with d2max = inf and with a finite one (the squared distance of its scale: it accepts the
    clusters nearby); then one NaN and one negative radius, and six points with a NaN, +inf or -inf coordinate."""
    rng = np.random.default_rng(seed)
    s = scales(**kw)
    p, scale = [np.zeros(3)], [s[0]]
    for k in (0, 1, 2, len(s) // 4, len(s) // 2, 3 * len(s) // 4, len(s) - 2, len(s) - 1):
        for _ in range(3):
            p.append(s[k] * (AXIS + 0.05 * rng.uniform(-1, 1, 3)))
            scale.append(s[k])
        p.append(s[k] * (AXIS + np.array([0.0, 2.0, 0.0])))
        scale.append(s[k])
        p.append(-s[k] * AXIS)
        scale.append(s[k])
    for far in (2.0 ** 50, 2.0 ** 55):
        for _ in range(3):
            p.append(far * _unit(rng.normal(0, 1, 3)))
            scale.append(far)
    p, scale = np.asarray(p), np.asarray(scale)
    with np.errstate(over="ignore"):
        finite = f32(36.0) * scale.astype(f32) * scale.astype(f32)      # (6 s)^2: a point's own cluster and its neighbours
    bad = np.tile(s[0] * AXIS, (6, 1))                                    # a non-finite point takes no pruning decision
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        bad[k, k % 3] = v
    out = np.concatenate([with_radius(p, INF), with_radius(p, finite), with_radius(p[:1], np.nan), with_radius(p[1:2], -1.0),
                          with_radius(bad, INF)])
    return _reflect(out, [2], kw)


def exposure_points(seed=41, **kw):
    """(m, 8) float32 {origin, unit normal, tmin, tmax}: cluster centres at several scales with normals along and across the
    axis, tmin = 2^-10 of the scale and tmax = inf, or 4 times the scale; then seven points with one non-finite origin
    coordinate.  Every ray of those takes no pruning decision and hits nothing: all 64 lanes of the point's wave visit every
    node in the order stored, which on the mirrored ladder fills the stack of every lane (exposure_bvh_kernel's stride-256
    layout, four such waves to a block)."""
    rng = np.random.default_rng(seed)
    s = scales(**kw)
    out = []
    for k in (0, 1, len(s) // 3, len(s) // 2, len(s) - 2, len(s) - 1):
        for j in range(3):
            o = s[k] * (AXIS + 0.05 * rng.uniform(-1, 1, 3))
            n = _unit((-AXIS, AXIS, rng.normal(0, 1, 3))[j])
            out.append(np.r_[o, n, s[k] * 2.0 ** -10, np.inf if j != 1 else 4.0 * s[k]])
    for k, bad in enumerate((np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.inf)):
        o = s[len(s) // 2] * AXIS                                         # seven points that decide nothing in any direction
        o[k % 3] = bad
        out.append(np.r_[o, _unit(-AXIS), 0.0, np.inf])
    return _reflect(np.asarray(out, f32), [2, 5], kw)


# 5 directions for world=True, so that lanes >= 5 idle; the last is the zero direction, which decides nothing from any origin
SHORT_TABLE = f32([[0, 0, 1], [0.6, 0, 0.8], [-0.6, 0, 0.8], [0, 0.6, 0.8], [0, 0, 0]])
