"""Grazing rays at the conditioning bound of the ray queries' BVH contract (include/rt_mi355x.h): scenes and ray
populations whose targeted triangles are met at a conditioning det / (|d| |e1| |e2|) just above (2^-10 .. 2^-6, where the tree
still owes the scan's bits and the box pad rho * (max|o| + cmax) is all that keeps a leaf) or just below (2^-14 .. 2^-10, where
it may lose the hit) the bound -- from origins 2, 2^11 and 2^21 scene extents away, at interior points and within 2^-20 .. 2^-8
of an edge or a corner on either side of it, hit in front of the origin, behind it and at t = 1 / 0.37.  The segment and
point-plus-direction-table forms of the same rays, and the one-sided check of rows the contract lets differ.  A helper, not a
test.  Everything is deterministic and needs no device (`pairs` reads the tree of the host builder).

The geometry, for a triangle with the unit normal n and the sine s of the corner angle at v0: det = -(d . (e1 x e2)), so the
conditioning of a ray is -(d^ . n) s.  A ray of conditioning r therefore has d^ = -(r / s) n + sqrt(1 - (r / s)^2) p for a unit
vector p in the plane; it is drawn in float64, rounded to fp32 once, and judged on the rounded values.  At 2^21 extents the
24 bits of a direction move the line by about one scene unit at the target, so most rays of that class meet another triangle
or none; they stay in the population, and the classes record what was aimed at, not what is hit."""
import numpy as np

from occluded_expect import with_interval
from query_accel_expect import EMPTY, LEAF, WELL_CONDITIONED, conditioning, leaf_span, records_of_rows
from query_expect import adversarial_scene, tri_rows

INF = np.float32(np.inf)
ABOVE = (2.0 ** -10, 2.0 ** -6)                  # the band in which the contract still promises the scan's bits
BELOW = (2.0 ** -14, 2.0 ** -10)                 # the band in which it allows a loss
L_CLASSES = (2.0, 2.0 ** 11, 2.0 ** 21)          # the origin's distance from its target, in scene extents
SCALES = (1.0, -1.0, 0.37)                       # t of the targeted hit is 1 / scale: -1 is a hit behind the origin
TARGETS = ("interior", "edge", "corner")
NEAR = (-20.0, -8.0)                             # log2 of an edge or corner target's barycentric distance from it
TIE_STEPS = (1.0, 4.0, 16.0, 64.0)               # a wall's displacement along the ray, in expected t errors of its floor's hit
FINE_STEPS = (2.0 ** -8, 2.0 ** -6, 2.0 ** -4, 2.0 ** -2)    # and in fractions of it: the measured t errors are that much smaller
SMALL = 2.0 ** -6                                # the scale of the pairs' second bundle, about the world origin
MIN_SINE = 2.0 ** -5                             # a targeted triangle's corner sine: above the band, so every ratio is reachable


def extent(rows):
    """The scene's largest |coordinate|."""
    return float(np.abs(np.asarray(rows, np.float32).reshape(-1, 4)[:, :3]).max())


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def general(n, seed=31, size=1.2):
    """query_expect.adversarial_scene's triangles (a duplicate and a reversed copy among them), none behind the origin;
    size: the half width of a triangle's vertex cloud."""
    if size == 1.2:
        return adversarial_scene(n, seed, behind=False)
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-12, -3, n)], 1)
    v = c[:, None, :] + rng.uniform(-size, size, (n, 3, 3))
    v[n // 2] = v[1]
    v[n - 1] = v[n // 3][[0, 2, 1]]
    return tri_rows(v)


def flat(n, seed=32, size=0.7):
    """Every triangle in one of six planes -- x = -2 or 2, y = -2 or 2, z = -5 or -9 -- with the same fp32 value on that axis in
    its three vertices, so most leaves hold triangles of one plane: their boxes have lo == hi there and the pad is all that
    holds a grazing line."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-11, -3, n)], 1)
    v = c[:, None, :] + rng.uniform(-size, size, (n, 3, 3))
    axis = np.arange(n) % 3
    plane = np.array([[-2.0, 2.0], [-2.0, 2.0], [-5.0, -9.0]])[axis, (np.arange(n) // 3) % 2]
    v[np.arange(n), :, axis] = plane[:, None]
    return tri_rows(v)


def slivers(n, seed=33):
    """Needles like test_bvh_build._slivers in four planes z = const, long in x or in y: 2 long and 2^-5 .. 2^-3 high,
    so the sine of the corner angle at v0 -- a factor of the conditioning -- is that small while the ray need not graze."""
    rng = np.random.default_rng(seed)
    a = np.c_[rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.array([-4.0, -6.0, -8.0, -10.0])[(np.arange(n) // 4) % 4]]
    h = 2.0 ** rng.uniform(-4.9, -3.0, n)
    e1 = np.zeros((n, 3))
    e2 = np.zeros((n, 3))
    along = np.arange(n) % 2
    e1[np.arange(n), along] = 2.0
    e2[np.arange(n), along] = 1.0
    e2[np.arange(n), 1 - along] = h * np.where(np.arange(n) % 4 < 2, 1.0, -1.0)     # both windings
    return tri_rows(np.stack([a, a + e1, a + e2], 1))


SCENES = {"general": general, "flat": flat, "slivers": slivers}


# ---- rays ------------------------------------------------------------------------------------------------------------------

def _frames(rows):
    """Per triangle, in float64 from the records the kernel intersects: v0, e1, e2, the unit normal, the sine at v0."""
    v0, e1, e2 = (x.astype(np.float64) for x in records_of_rows(rows))
    n = np.cross(e1, e2)
    area2 = np.linalg.norm(n, axis=1)
    with np.errstate(all="ignore"):
        sine = area2 / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
        n = n / area2[:, None]
    return v0, e1, e2, n, np.where(np.isfinite(sine), sine, 0.0)


def _barycentric(rng, m, target):
    """(u, v) of m targets by class: interior points, points beside an edge, points beside a corner -- either side."""
    u, v = rng.uniform(0.05, 0.45, m), rng.uniform(0.05, 0.45, m)
    eps1 = rng.choice([-1.0, 1.0], m) * 2.0 ** rng.uniform(*NEAR, m)
    eps2 = rng.choice([-1.0, 1.0], m) * 2.0 ** rng.uniform(*NEAR, m)
    s = rng.uniform(0.1, 0.9, m)
    which = rng.integers(0, 3, m)
    edge, corner = target == 1, target == 2
    eu = np.choose(which, [eps1, s, s])
    ev = np.choose(which, [s, eps1, 1.0 - s - eps1])
    cu = np.choose(which, [eps1, 1.0 - eps1, eps1])
    cv = np.choose(which, [eps2, eps2, 1.0 - eps2])
    return np.where(edge, eu, np.where(corner, cu, u)), np.where(edge, ev, np.where(corner, cv, v))


def _aim(frames, prim, ratio, L, scale, uv, rng, ext, phi=None):
    """The rays (m, 6) float32 that meet triangle prim[i] at its point v0 + u e1 + v e2 with the conditioning ratio[i], and those
    target points (float64).  phi: the angle of the in-plane part of d from e1 (drawn uniformly when None)."""
    v0, e1, e2, n, sine = (x[prim] for x in frames)
    m = prim.shape[0]
    c = ratio / sine
    a1 = e1 / np.linalg.norm(e1, axis=1)[:, None]
    a2 = np.cross(n, a1)
    phi = rng.uniform(0.0, 2.0 * np.pi, m) if phi is None else phi
    p = np.cos(phi)[:, None] * a1 + np.sin(phi)[:, None] * a2
    unit = -c[:, None] * n + np.sqrt(1.0 - c * c)[:, None] * p
    u, v = uv
    P = v0 + u[:, None] * e1 + v[:, None] * e2
    d = (unit * (L * ext * np.abs(scale))[:, None]).astype(np.float32)
    o = (P - d.astype(np.float64) / scale[:, None]).astype(np.float32)
    return np.ascontiguousarray(np.c_[o, d], np.float32), P


def rays(rows, kind, n, seed, l_classes=L_CLASSES, prims=None):
    """A population of n grazing rays at the scene `rows`: kind "above" (every targeted triangle's conditioning log-uniform in
    ABOVE, and >= 2^-10 for the fp32 ray in float64) or "below" (in BELOW, and < 2^-10).  A ray whose rounded values leave its
    band is drawn again.  -> {"rays": (n, 6) float32, "prim": the targeted triangle, "ratio": its conditioning with the ray,
    "L", "scale", "target": the class indices into L_CLASSES (or l_classes), SCALES and TARGETS, "point": the target (float64)}."""
    lo, hi = ABOVE if kind == "above" else BELOW
    rng = np.random.default_rng(seed)
    frames = _frames(rows)
    cand = np.nonzero(frames[4] >= MIN_SINE)[0] if prims is None else np.asarray(prims, np.int64)
    assert cand.size
    ext = extent(rows)
    prim = cand[rng.integers(0, cand.size, n)]
    li = np.arange(n) % len(l_classes)                                    # every combination of the three classes occurs
    si = (np.arange(n) // len(l_classes)) % len(SCALES)
    ti = (np.arange(n) // (len(l_classes) * len(SCALES))) % len(TARGETS)
    out = np.zeros((n, 6), np.float32)
    point = np.zeros((n, 3))
    ratio = np.zeros(n)
    todo = np.arange(n)
    for _ in range(64):
        r = 2.0 ** rng.uniform(np.log2(lo), np.log2(hi), todo.size)
        got, P = _aim(frames, prim[todo], r, np.asarray(l_classes)[li[todo]], np.asarray(SCALES)[si[todo]],
                      _barycentric(rng, todo.size, ti[todo]), rng, ext)
        real = conditioning(got, rows, prim[todo])
        ok = (real >= lo) & (real < hi) if kind == "below" else (real >= lo)
        out[todo[ok]], point[todo[ok]], ratio[todo[ok]] = got[ok], P[ok], real[ok]
        todo = todo[~ok]
        if not todo.size:
            break
    assert not todo.size, (kind, todo.size)
    return {"rays": out, "prim": prim, "ratio": ratio, "L": li, "scale": si, "target": ti, "point": point}


# ---- pairs: a grazed floor and a wall met head-on at a near-tie of t -------------------------------------------------------------

def pairs(m, seed=34, l_classes=L_CLASSES[:2]):
    """m pairs -> (rows of 2 m triangles, the `rivals` population).  Floor i (triangle i) runs from a vertex at x = -9 to an edge
    in the plane x = 3, 0.5 .. 1 wide and turned about the x axis by its own angle; every third floor belongs to a bundle 2.5 x 2.5 across
    around z = -6, the others to the same bundle scaled by SMALL about the world origin, where a box's cmax is far below the
    scene's extent and max|o| is all of the pad.  The far edge lies in a face of every box that holds the floor.  Ray i runs
    along its floor (within 0.005 rad of the x axis in the floor's plane, towards the edge or away from it: so the fp32
    rounding of a far origin moves the hit by little) at a conditioning in ABOVE and meets it 2^-16 .. 2^-6 (barycentric)
    inside that edge: the line leaves or enters the floor's boxes right at the hit.  Wall i (triangle m + i) is a small triangle
    across the same ray, facing it, at the point where the fp32 ray meets the floor's plane displaced along the ray by
    +-{1, 4, 16, 64} times the floor hit's expected t error 2^-24 |o - v0| / ratio (as a length) -- and, because the t errors
    measured on these floors are some 50 times below that first-order figure, also by +-{2^-8, 2^-6, 2^-4, 2^-2} of it: the two t
    nearly tie, from both sides.  The floors' centres lie at x = -1 and the walls' about x = 3 (times the bundle's scale), farther
    apart than the bundle is wide, so the builder separates them (leaves_of says so).  Origins are 2 and 2^11 extents of the
    whole scene away, the small bundle's all 2^11: at 2^21 the expected t error exceeds the scene.  The population is one `rays` returns, with "wall": the
    wall's triangle, "step": its signed displacement in t errors, "t_err": that error in units of t, "small": the bundle."""
    rng = np.random.default_rng(seed)
    small = np.arange(m) % 3 != 0                                         # two pairs of three
    k = np.where(small, np.cumsum(small) - 1, np.cumsum(~small) - 1)      # the pair's number within its bundle
    sigma = np.where(small, SMALL, 1.0)
    side = np.where(small, np.ceil(np.sqrt(small.sum())), np.ceil(np.sqrt((~small).sum()))).astype(np.int64)
    y = ((k % side) / np.maximum(side - 1, 1) - 0.5) * 2.5
    z = ((k // side) / np.maximum(side - 1, 1) - 0.5) * 2.5
    w = rng.uniform(0.5, 1.0, m) / 2.0
    alpha = rng.uniform(0.0, np.pi, m)
    fl = np.zeros((m, 3, 3))
    fl[:, :, 1], fl[:, :, 2] = y[:, None], z[:, None]
    fl[:, 0, 0], fl[:, 1, 0], fl[:, 2, 0] = -9.0, 3.0, 3.0
    fl[:, 1, 1], fl[:, 1, 2] = fl[:, 1, 1] - w * np.cos(alpha), fl[:, 1, 2] - w * np.sin(alpha)
    fl[:, 2, 1], fl[:, 2, 2] = fl[:, 2, 1] + w * np.cos(alpha), fl[:, 2, 2] + w * np.sin(alpha)
    fl *= sigma[:, None, None]
    fl[small, :, 1:] += np.stack([y, z], 1)[small, None, :] * (0.1 - SMALL)   # (the small bundle 0.25 across: its walls are no smaller)
    fl[~small, :, 2] -= 6.0
    flip = k % 4 >= 2                                                     # both windings
    fl[flip] = fl[flip][:, [0, 2, 1]]
    floors = tri_rows(fl)
    frames = _frames(floors)
    assert (frames[4] >= MIN_SINE).all()
    ext = extent(floors)
    prim = np.arange(m)
    li, si = np.where(small, len(l_classes) - 1, k % len(l_classes)), (k // len(l_classes)) % len(SCALES)
    ti = np.ones(m, np.int64)                                             # every target lies beside the edge u + v = 1
    out, point, ratio = np.zeros((m, 6), np.float32), np.zeros((m, 3)), np.zeros(m)
    todo = prim.copy()
    for _ in range(64):
        r = 2.0 ** rng.uniform(np.log2(ABOVE[0]), np.log2(ABOVE[1]), todo.size)
        eps, s = 2.0 ** rng.uniform(-16.0, -6.0, todo.size), rng.uniform(0.3, 0.7, todo.size)
        # e1 points from v0 to one end of the far edge: the x axis in the floor's plane is e1 + e2
        axis = frames[1][todo] + frames[2][todo]
        a1 = frames[1][todo] / np.linalg.norm(frames[1][todo], axis=1)[:, None]
        a2 = np.cross(frames[3][todo], a1)
        phi = np.arctan2(np.einsum("ij,ij->i", axis, a2), np.einsum("ij,ij->i", axis, a1))
        phi = phi + rng.choice([0.0, np.pi], todo.size) + rng.normal(0.0, 0.005, todo.size)
        got, P = _aim(frames, todo, r, np.asarray(l_classes)[li[todo]], np.asarray(SCALES)[si[todo]],
                      (s * (1.0 - eps), (1.0 - s) * (1.0 - eps)), rng, ext, phi)
        real = conditioning(got, floors, todo)
        ok = real >= ABOVE[0]
        out[todo[ok]], point[todo[ok]], ratio[todo[ok]] = got[ok], P[ok], real[ok]
        todo = todo[~ok]
        if not todo.size:
            break
    assert not todo.size
    o, d = out[:, :3].astype(np.float64), out[:, 3:].astype(np.float64)
    dn = np.linalg.norm(d, axis=1)
    unit = d / dn[:, None]
    t_err = 2.0 ** -24 * np.linalg.norm(o - frames[0], axis=1) / ratio    # as a length along the ray
    steps = np.asarray(TIE_STEPS + FINE_STEPS)                            # (the small bundle: the first two fine ones, which stay  
    step = np.where(small, steps[4 + (k // 2) % 2], steps[(k // 2) % 8]) * np.where(k % 2 == 0, 1.0, -1.0)   #  beside its far edge)
    # where the fp32 ray really meets the floor's plane (the rounding of o moved it), then along the ray
    t_plane = np.einsum("ij,ij->i", frames[0] - o, frames[3]) / np.einsum("ij,ij->i", d, frames[3])
    centre = o + t_plane[:, None] * d + (step * t_err)[:, None] * unit
    a1 = np.cross(unit, np.where(np.abs(unit[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
    a1 /= np.linalg.norm(a1, axis=1)[:, None]
    a2 = np.cross(unit, a1)
    # a wall a far origin still meets: the fp32 difference o - v0 is rounded to an ulp of |o|
    s = np.maximum(0.04 * sigma, 6.0 * np.spacing(np.abs(out[:, :3]).max(axis=1)).astype(np.float64))[:, None]
    wl = np.stack([centre - s * a1 - s * a2, centre - s * a1 + 2.0 * s * a2, centre + 2.0 * s * a1 - s * a2], 1)   # faces the ray
    rows = np.concatenate([floors, tri_rows(wl)])
    return rows, {"rays": out, "prim": prim, "ratio": ratio, "L": li, "scale": si, "target": ti, "point": point,
                  "wall": prim + m, "step": step, "t_err": t_err / dn, "small": small}


def leaves_of(nodes, recs, info):
    """The leaf (its reference) that holds each upload index, -1 for the always-tested ones."""
    out = np.full(recs.shape[0], -1, np.int64)
    idx = recs["index"].astype(np.int64)
    for nd in nodes:
        for ref in nd["child"]:
            ref = int(ref)
            if ref != EMPTY and ref & LEAF:
                first, count = leaf_span(ref)
                out[idx[first:first + count]] = ref
    return out


# ---- the other queries' forms of a population --------------------------------------------------------------------------------

def segments(pop):
    """(n, 8) segments of a population's rays for Occluded / IntersectAll, a third each: the whole line; t from 0 on; a window of
    2^-6 of |t| about the targeted hit's t = 1 / scale (so that the interval prunes next to the hit)."""
    r = pop["rays"]
    n = r.shape[0]
    t = (1.0 / np.asarray(SCALES))[pop["scale"]]
    k = (np.arange(n) // (len(L_CLASSES) * len(SCALES) * len(TARGETS))) % 3
    lo = np.where(k == 0, -np.inf, np.where(k == 1, 0.0, t - np.abs(t) * 2.0 ** -6))
    hi = np.where(k == 2, t + np.abs(t) * 2.0 ** -6, np.inf)
    return with_interval(r, lo.astype(np.float32), hi.astype(np.float32))


def exposure_groups(pop, groups):
    """The first 64 * groups rays of a population as Exposure calls with a world-space table: per group (points (64, 8) {origin,
    a dummy normal, tmin = -inf, tmax = inf}, dirs (64, 4)) -- point i's direction i is its own grazing ray, the other 63 are its
    neighbours' directions from its origin."""
    out = []
    r = pop["rays"]
    for g in range(groups):
        part = r[64 * g:64 * g + 64]
        if part.shape[0] < 64:
            break
        pts = np.zeros((64, 8), np.float32)
        pts[:, :3], pts[:, 5], pts[:, 6], pts[:, 7] = part[:, :3], 1.0, -INF, INF
        dirs = np.zeros((64, 4), np.float32)
        dirs[:, :3] = part[:, 3:]
        out.append((pts, dirs))
    return out


# ---- rows that may differ -----------------------------------------------------------------------------------------------------

def check_one_sided(orc, got, scan, rays_, rows, contract=None, nearest=False, label=""):
    """The contract where it allows a loss: a row of `got` (the tree) that differs from `scan` has a scan winner below 2^-10, and
    reports no hit or a hit the oracle's HitTriangle gives for that ray and prim, bit for bit (nearest: with t > 0).  Prints and
    returns how many rows differ; no cap."""
    contract = orc.FMA if contract is None else contract
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    s = np.ascontiguousarray(scan).view(np.uint32).reshape(-1, 4)
    differ = np.nonzero((g != s).any(axis=1))[0]
    ratio = conditioning(rays_[differ], rows, scan["prim"][differ])
    assert (ratio < WELL_CONDITIONED).all(), (label, differ[~(ratio < WELL_CONDITIONED)][:5])
    tris = np.asarray(rows, np.float32).reshape(-1, 3, 4)[:, :, :3]
    none = 0
    for i in differ:
        p = int(got["prim"][i])
        if p < 0:
            assert g[i].tolist() == [0, 0, 0, 0xFFFFFFFF], (label, i, got[i])
            none += 1
            continue
        assert p < tris.shape[0], (label, i, got[i])
        hit, t, u, v = orc.hit_triangle(rays_[i], *tris[p], contract=contract)
        assert hit and (not nearest or t > 0), (label, i, got[i])
        assert np.array([t, u, v], np.float32).view(np.uint32).tolist() == g[i, :3].tolist(), (label, i, got[i], (t, u, v))
    print("%s: %d rays, %d differ from the scan (scan winner below 2^-10), %d of them report no hit" % (label, g.shape[0], differ.size, none))
    return int(differ.size)


def targeted_wins(pop, scan):
    """The rows whose scan winner is the triangle the ray was aimed at."""
    return np.asarray(scan["prim"]) == pop["prim"]
