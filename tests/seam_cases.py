"""Scenes and populations that put the decisive primitives of every scan-mode query on the seams between the LDS chunks of
kQueryChunk = 1024 triangle records (csrc/rt_scan.hpp; test_seam_cases.py without a device, test_gpu_query_seams.py on one):
the last record of a chunk, the first of the next, the last record of the scene, a chunk of exactly 1024 and one of a single
record.  A helper, not a test.  Everything is deterministic and needs no device.

The scene.  Filler triangles lie in x < -2; everything a test aims at lies in x > 3.  Around every seam S in {1024, 2048} eight
"petals" take the upload indices S - 4 .. S + 3, as far as the scene has them (at 1023 triangles 1020 .. 1022 exist): thin
triangles that all face +z, lie in eight parallel planes z = -8 + k / 4 (k = index - (S - 4)), all contain the point above the
seam's centre, and each stretch from there in one of eight directions 45 degrees apart.  So
  * a ray down the centre (the stack ray) hits all of them, t = 8 - k / 4: the depth order is the reverse of the upload order,
    and the four records of the second chunk sort before the four of the first;
  * a ray down through petal k's outer part (its `point`, 2.5 axis lengths from the centre) hits that petal and nothing else,
    and a point 1/16 above it has that petal as its one nearest primitive: every index S - 4 .. S + 3 and n_tris - 1 (which is one
    of them at every size of SIZES) is the unique answer of rays and points of its own.
Every coordinate is a small dyadic number and every petal's det a power of two, so for the rays along z the reference's t, u
and v are exact under both arithmetic contracts and a tie is a tie bit for bit.

Two layouts.  The issue asks for the records S - 1 and S to be isolated targets, members of a stack of eight distinct depths,
AND bit-identical twins; one scene cannot hold all three, so the scene comes in two layouts that differ in ONE record:
"stack" is the scene above; "tie" overwrites record S (where the scene has it) with a copy of record S - 1, vertex for vertex:
the last record of one chunk and the first of the next are the same triangle.  The populations are the same in both.

sweep_batch and triangle_batch (SphereCast, TriangleDistance) tag every targeted row with the primitive it must name on the stack
layout; sweep_table / triangle_table, sweep_winners / triangle_winners and lose_columns restate the answers from
spherecast_expect and tridistance_expect, with the same two ways to break them as `winners` has for the rays."""
import numpy as np

import closest_expect as ce
import spherecast_expect as spe
import tridistance_expect as tde
from trioverlap_expect import queries_of
from lattice_cases import ray_segments
from occluded_expect import with_interval
from query_expect import FLT_MAX, HIT_DTYPE, adversarial_rays, edge_rows  # noqa: F401  (edge_rows: for the tests)

f32 = np.float32
INF = f32(np.inf)
CHUNK = 1024                                   # rtk::kQueryChunk (csrc/rt_scan.hpp)
SEAMS = (1024, 2048)
SIZES = (1023, 1024, 1025, 2048, 2049)
AXES = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))     # petal k stretches along AXES[k]
CENTRE = {1024: (8.0, 0.0), 2048: (8.0, 16.0)}
Z0, DZ = -8.0, 0.25                            # petal k lies in z = Z0 + k DZ
ABOVE, BELOW = 0.0, -16.0                      # the z of the ray origins in front of the petals and behind them
N_RAYS, N_RAYS_LONG = 331, 1100                # batch lengths: 1100 = 4 x 256 + 76 = 2 x 512 + 76 = 1024 + 76
LATE = 1024                                    # the late-finisher batch: whole blocks for K = 1, 2 and 4


def layouts(n_tris):
    """The layouts that differ at this size: without a record S there is no twin."""
    return ("stack", "tie") if any(S < n_tris for S in SEAMS) else ("stack",)


def members(n_tris, S):
    """The upload indices of seam S's petals that the scene has."""
    return [i for i in range(S - 4, S + 4) if i < n_tris]


def placed_seams(n_tris):
    return [S for S in SEAMS if members(n_tris, S)]


def _k(i, S):
    return i - (S - 4)


def petal_z(i, S):
    return Z0 + DZ * _k(i, S)


def petal_point(i, S):
    """(x, y) inside petal i and inside no other: v0 + 3 a = centre + 2.5 a."""
    a, c = AXES[_k(i, S)], CENTRE[S]
    return (c[0] + 2.5 * a[0], c[1] + 2.5 * a[1])


def petal(i, S):
    """(3, 3) vertices: v0 = centre - a / 2, v1 = v0 + 4 a - p, v2 = v0 + 4 a + p with p = a turned by 90 degrees, all at the
    petal's z.  cross(e1, e2).z = 8 (a x p) = 8 or 16 > 0: it faces +z, and 1 / det is exact."""
    a, c, z = AXES[_k(i, S)], CENTRE[S], petal_z(i, S)
    p = (-a[1], a[0])
    v0 = np.array([c[0] - 0.5 * a[0], c[1] - 0.5 * a[1], z])
    v1 = v0 + [4 * a[0] - p[0], 4 * a[1] - p[1], 0.0]
    v2 = v0 + [4 * a[0] + p[0], 4 * a[1] + p[1], 0.0]
    return np.stack([v0, v1, v2])


def seam_scene(n_tris, layout="stack"):
    """-> (rows (3 n_tris, 4) float32 upload rows, info).  info: n_tris, layout, last = n_tris - 1, seams = {S: {centre,
    members (ascending indices), full (all eight exist), tie ((S - 1, S) in the tie layout where record S exists, else None),
    top / bottom (the highest and lowest z of the petals the layout keeps in place)}}, seam_of = {index: S} of every petal,
    applies = {tie, stack, cut, last}: does the layout have a twin pair; a stack of at least two depths; a stack of eight, four on
    either side of the seam; and is record n_tris - 1 an isolated target (not a twin)."""
    assert n_tris in SIZES and layout in ("stack", "tie")
    rng = np.random.default_rng(1000 + n_tris)
    centre = np.stack([rng.uniform(-9.0, -2.5, n_tris), rng.uniform(-4.0, 4.0, n_tris), rng.uniform(-4.0, 4.0, n_tris)], 1)
    tris = centre[:, None, :] + rng.uniform(-0.3, 0.3, (n_tris, 3, 3))
    seams, seam_of = {}, {}
    for S in placed_seams(n_tris):
        m = members(n_tris, S)
        for i in m:
            tris[i] = petal(i, S)
            seam_of[i] = S
        tie = (S - 1, S) if (layout == "tie" and S < n_tris) else None
        if tie:
            tris[S] = tris[S - 1]
        kept = [i for i in m if not (tie and i == S)]
        seams[S] = {"centre": CENTRE[S], "members": m, "full": len(m) == 8, "tie": tie,
                    "top": max(petal_z(i, S) for i in kept), "bottom": min(petal_z(i, S) for i in kept)}
    rows = np.zeros((n_tris, 3, 4), f32)
    rows[:, :, :3] = tris
    assert (rows[[i for i in range(n_tris) if i not in seam_of], :, 0] < -2.0).all()
    last = n_tris - 1
    twins = {t[1] for t in (s["tie"] for s in seams.values()) if t}
    info = {"n_tris": n_tris, "layout": layout, "last": last, "seams": seams, "seam_of": seam_of,
            "applies": {"tie": bool(twins), "stack": any(len(s["members"]) >= 2 for s in seams.values()),
                        "cut": any(s["full"] and not s["tie"] for s in seams.values()), "last": last not in twins}}
    return rows.reshape(-1, 4), info


SPHERES = f32([[8.0, 0.0, -4.0, 0.5], [8.0, 0.0, -4.0, 0.5], [10.5, 0.0, -3.0, 0.25], [-5.0, 0.0, 0.0, 1.5]])
"""Four spheres, the first two coincident on the stack ray of seam 1024 (in front of the stack), the third above petal 1020's
point, the fourth among the filler: prim = n_tris + si right behind a seam-sized n_tris."""


# ---- rays -----------------------------------------------------------------------------------------------------------------

def targeted_rays(n_tris):
    """-> (rays (m, 6) float32, tags): the rays aimed at the seams, the same in both layouts.  tags[j] = (kind, S, index):
    front / behind -- down through petal `index`'s point from z = 0 (t = -z > 0) and from z = -16 (t < 0, which the
    reference's farthest-hit rule accepts); centroid -- through its fp32 centroid with the direction (0, 0, -2);
    stack_front / stack_behind -- down the seam's centre, through every petal (index = -1)."""
    rays, tags = [], []
    for S in placed_seams(n_tris):
        for i in members(n_tris, S):
            x, y = petal_point(i, S)
            cen = petal(i, S).astype(f32).mean(axis=0, dtype=f32)
            for kind, ray in (("front", [x, y, ABOVE, 0, 0, -1]), ("behind", [x, y, BELOW, 0, 0, -1]),
                              ("centroid", [cen[0], cen[1], ABOVE, 0, 0, -2])):
                rays.append(ray)
                tags.append((kind, S, i))
        cx, cy = CENTRE[S]
        for kind, z in (("stack_front", ABOVE), ("stack_behind", BELOW)):
            rays.append([cx, cy, z, 0, 0, -1])
            tags.append((kind, S, -1))
    return np.ascontiguousarray(rays, f32), tags


def distinct_rays(n_tris, rows):
    """-> (rays, tags): the targeted rays, then 69 of query_expect.adversarial_rays of the whole scene (tag ("adversarial", 0,
    -1)): a NaN, +inf or -inf in every component, a zero direction, two rays with everything behind them, and random ones
    from around the origin towards random triangles.  The batches below repeat these; the oracle sees each once."""
    rays, tags = targeted_rays(n_tris)
    adv = adversarial_rays(rows, 48, 77 + n_tris)[-69:]
    return np.ascontiguousarray(np.concatenate([rays, adv]), f32), tags + [("adversarial", 0, -1)] * adv.shape[0]


def _spread(n, d, seed):
    """n indices into d distinct entries, every entry about n / d times, shuffled: targeted and adversarial entries share waves."""
    return np.random.default_rng(seed).permutation(np.arange(n) % d)


def ray_batch(n_tris, rows):
    """-> (rays (1100, 6), idx (1100,) into distinct_rays, distinct rays, tags).  The first 331 alone hold every distinct ray
    too: 331 and 1100 are no multiples of 64 and end in a partial block for K = 1, 2 and 4."""
    rays, tags = distinct_rays(n_tris, rows)
    d = rays.shape[0]
    assert 2 * d <= N_RAYS
    idx = np.concatenate([_spread(N_RAYS, d, 1), _spread(N_RAYS_LONG - N_RAYS, d, 2)])
    return np.ascontiguousarray(rays[idx]), idx, rays, tags


def find(tags, kind, S=None, index=None):
    """The positions in a tag list of the entries of one kind (and seam, and index)."""
    return [j for j, t in enumerate(tags) if t[0] == kind and (S is None or t[1] == S) and (index is None or t[2] == index)]


# ---- segments -------------------------------------------------------------------------------------------------------------

def segment_batch(n_tris, rows):
    """-> (segs (n, 8), idx (n,) into distinct_rays, tags).  The first 331 rays of ray_batch with lattice_cases.ray_segments'
    intervals by turns ([0, inf], every t, [0, 1]; tag ("turns", ...)), and the interval families of the seams, each twice:
      only_last   the stack ray of the seam that holds n_tris - 1, [t - 1/8, t + 1/8] around that petal's t: nothing else
      far_half    a stack ray with [t_(S-1) - 1/8, inf]: the petals below the seam, S - 4 .. S - 1 (the first chunk's; at 1023
                  triangles S - 1 is missing and 1022 stands in, here and in closed_tie)
      near_half   a stack ray with [0, t_S + 1/8]: the petals S .. S + 3 (the second chunk's)
      closed_tie  the front ray of petal S - 1 with tmin == tmax == its t (both twins in the tie layout), and the stack ray with
                  tmin == tmax == t_S
      dead        tmin > tmax on stack and front rays
    then shuffled; (kind, S, index) per segment, index = the petal an interval is built around."""
    rays, ridx, distinct, rtags = ray_batch(n_tris, rows)
    turns = ray_segments(rays[:N_RAYS])
    segs, idx, tags = [turns], [ridx[:N_RAYS]], [("turns",) + rtags[j][1:] for j in ridx[:N_RAYS]]
    extra = []
    last = n_tris - 1
    for S in placed_seams(n_tris):
        m = members(n_tris, S)
        stack = find(rtags, "stack_front", S)[0]
        t = {i: -petal_z(i, S) for i in m}                                # from z = 0 along (0, 0, -1)
        if last in m:
            extra.append((stack, t[last] - 0.125, t[last] + 0.125, ("only_last", S, last)))
        lo = max(i for i in m if i < S)                                   # S - 1, or the scene's last record below it
        extra.append((stack, t[lo] - 0.125, np.inf, ("far_half", S, lo)))
        extra.append((find(rtags, "front", S, lo)[0], t[lo], t[lo], ("closed_tie", S, lo)))
        if S in m:
            extra.append((stack, 0.0, t[S] + 0.125, ("near_half", S, S)))
            extra.append((stack, t[S], t[S], ("closed_tie", S, S)))
        extra.append((stack, 1.0, 0.5, ("dead", S, -1)))
        extra.append((find(rtags, "front", S, m[-1])[0], np.inf, -np.inf, ("dead", S, m[-1])))
    extra = extra + extra
    while (N_RAYS + len(extra)) % 64 == 0 or len(extra) % 2:
        extra.append(extra[0])
    segs.append(np.stack([np.r_[distinct[j], lo, hi] for j, lo, hi, _ in extra]).astype(f32))
    idx.append(np.array([e[0] for e in extra]))
    tags += [e[3] for e in extra]
    order = np.random.default_rng(3).permutation(len(tags))
    return (np.ascontiguousarray(np.concatenate(segs)[order], f32), np.concatenate(idx)[order], [tags[j] for j in order])


def late_finisher(n_tris, rows, position=None):
    """-> (segs (1024, 8), idx (1024,) into distinct_rays): the front rays of the petals 1020 .. 1023 other than n_tris - 1, by
    turns, over [0, inf] -- each is occluded by a record of the FIRST chunk and by nothing else -- and at `position` the front
    ray of petal n_tris - 1, which only the scene's last record occludes (the stack layout; in the tie layout at 1025 and 2049
    that petal is the twin's empty place).  position=None: no such segment, every ray of every block finishes in chunk 0."""
    distinct, tags = distinct_rays(n_tris, rows)
    early = [find(tags, "front", 1024, i)[0] for i in members(n_tris, 1024) if i < CHUNK and i != n_tris - 1]
    assert early
    idx = np.array([early[j % len(early)] for j in range(LATE)])
    if position is not None:
        last = n_tris - 1
        idx[position] = find(tags, "front", [S for S in placed_seams(n_tris) if last in members(n_tris, S)][0], last)[0]
    return with_interval(distinct[idx], 0.0, np.inf), idx


# ---- points ---------------------------------------------------------------------------------------------------------------

def point_batch(n_tris, rows):
    """-> (points (n, 4) float32 {x, y, z, d2max}, tags), n > 256 and no multiple of 64, shuffled.  rows: the STACK layout's
    (the radii are taken from it).  tags[j] = (kind, S, index):
      near        1/16 above petal `index`'s point, d2max = inf: that petal is the one nearest primitive
      under       1/16 below the point of petal S - 1: equidistant from both twins in the tie layout
      beside      above the highest and below the lowest petal on the stack's axis, and one off the axis, d2max = inf
      fourth      the same two axis points with d2max == the squared distance of the 4th petal from there (closed: it is
                  accepted, the 5th is not): from above the petals S + 3 .. S, from below S - 4 .. S - 1 -- the cut falls on
                  the seam (stacks of eight only; index = that 4th petal)
      nan / negative   closest_expect.radius_families' two bad radii on the near points
      general     closest_expect.points_for of the whole scene, d2max = inf, and 16 of them with d2max = 0"""
    pts, tags = [], []
    for S in placed_seams(n_tris):
        m = members(n_tris, S)
        cx, cy = CENTRE[S]
        top, bot = max(petal_z(i, S) for i in m) + 0.5, Z0 - 0.5
        for i in m:
            x, y = petal_point(i, S)
            pts.append([x, y, petal_z(i, S) + 0.0625, np.inf])
            tags.append(("near", S, i))
        if S - 1 in m:
            x, y = petal_point(S - 1, S)
            pts.append([x, y, petal_z(S - 1, S) - 0.0625, np.inf])
            tags.append(("under", S, S - 1))
        for p in ([cx, cy, top, np.inf], [cx, cy, bot, np.inf], [cx + 0.0625, cy + 0.03125, top, np.inf]):
            pts.append(p)
            tags.append(("beside", S, -1))
        if len(m) == 8:
            for z, fourth in ((top, S), (bot, S - 1)):
                t = ce.table(f32([[cx, cy, z]]), rows)[0][0, fourth]
                assert t == f32(z - petal_z(fourth, S)) ** 2
                pts.append([cx, cy, z, t])
                tags.append(("fourth", S, fourth))
    near = f32([p for p, t in zip(pts, tags) if t[0] == "near"])
    fam = ce.radius_families(near, rows)
    for kind in ("nan", "negative"):
        pts.extend(fam[kind].tolist())
        tags += [(kind, t[1], t[2]) for t in tags if t[0] == "near"]
    general = ce.with_radius(ce.points_for(rows, 260, 91 + n_tris), INF)
    pts.extend(general.tolist())
    pts.extend(ce.with_radius(general[:16], 0.0).tolist())
    tags += [("general", 0, -1)] * (general.shape[0] + 16)
    if len(pts) % 64 == 0:
        pts.append(pts[0])
        tags.append(tags[0])
    order = np.random.default_rng(4).permutation(len(pts))
    return np.ascontiguousarray(f32(pts)[order]), [tags[j] for j in order]


def tie_cursor(pts, tags, exp_closest):
    """The ClosestAll cursor of the seams: at every `near` and `under` point of a petal S - 1 the record ClosestPoint is
    expected to answer (the twin pair's first record in the tie layout), elsewhere none: the continuation starts behind it."""
    after = np.zeros(pts.shape[0], HIT_DTYPE)
    after["prim"] = -1
    for j, t in enumerate(tags):
        if t[0] in ("near", "under") and t[2] == t[1] - 1:
            after[j] = exp_closest[j]
    return after


# ---- sweeps ---------------------------------------------------------------------------------------------------------------

SWEEP_R = 1.0 / 32                             # the targeted sweeps' radius: a petal's neighbours are many radii away


def _pad(items, tags):
    """More than 256 items and no multiple of 64: the batch ends in a partial wave of a second block."""
    assert len(items) > 256
    if len(items) % 64 == 0:
        items.append(items[0])
        tags.append(tags[0])


def sweep_batch(n_tris, rows):
    """-> (sweeps (n, 8) float32 {origin, direction, radius, tmax}, tags), n > 256 and no multiple of 64, shuffled.  rows: the
    STACK layout's.  tags[j] = (kind, S, index), index = the primitive the sweep must name on the stack layout, -1 = none:
      down        from (petal_point(index), z = 0) along (0, 0, -1), r = 1/32, tmax = inf: that petal alone, on its face
      up          the same from z = -16 along (0, 0, +1): the petal again, from behind
      start       from 1/16 above the petal's point with r = 1/8: the sweep starts in overlap, t = 0 and that petal
      axis_down / axis_up   along the stack's axis from z = 0 and from z = -16: the highest member (a record of the SECOND chunk
                  where the seam has one) and the lowest
      cut         the axis_down sweep with tmax == the t of its contact (closed: index = that petal) and one ulp below it (-1)
      bad         the down sweeps with a negative radius, a NaN radius and tmax < 0 (-1)
      general     260 of spherecast_expect.batch of the whole scene (its fixed populations are some 2 500 sweeps, so the batch is
                  drawn at 3 000 and, being shuffled, cut at 260), index -1 without meaning
    Every coordinate of the targeted sweeps is dyadic: their t are exact and a tie is a tie bit for bit."""
    sw, tags = [], []
    r = SWEEP_R
    for S in placed_seams(n_tris):
        m = members(n_tris, S)
        cx, cy = CENTRE[S]
        for i in m:
            x, y = petal_point(i, S)
            down = [x, y, ABOVE, 0, 0, -1, r, np.inf]
            for kind, s in (("down", down), ("up", [x, y, BELOW, 0, 0, 1, r, np.inf]),
                            ("start", [x, y, petal_z(i, S) + 0.0625, 0, 0, -1, 0.125, np.inf])):
                sw.append(s)
                tags.append((kind, S, i))
            for slot, val in ((6, -r), (6, np.nan), (7, -1.0)):
                s = list(down)
                s[slot] = val
                sw.append(s)
                tags.append(("bad", S, -1))
        axis = [cx, cy, ABOVE, 0, 0, -1, r, np.inf]
        sw += [axis, [cx, cy, BELOW, 0, 0, 1, r, np.inf]]
        tags += [("axis_down", S, m[-1]), ("axis_up", S, m[0])]
        t = spe.table(f32([axis]), rows)[0][0, m[-1]]
        assert t == f32(ABOVE - petal_z(m[-1], S) - r)
        sw += [axis[:7] + [t], axis[:7] + [np.nextafter(t, f32(0))]]
        tags += [("cut", S, m[-1]), ("cut", S, -1)]
    general = spe.batch(rows, 3000, 51 + n_tris)[:260]
    sw.extend(general.tolist())
    tags += [("general", 0, -1)] * general.shape[0]
    _pad(sw, tags)
    order = np.random.default_rng(5).permutation(len(sw))
    return np.ascontiguousarray(f32(sw)[order]), [tags[j] for j in order]


def sweep_table(sweeps, rows, edges=False, spheres=None):
    """spherecast_expect.table, read-only."""
    tab = spe.table(sweeps, rows, edges, spheres)
    for x in tab:
        x.setflags(write=False)
    return tab


def sweep_winners(tab, sweeps, drop=(), tie_high=False):
    """spherecast_expect.winners' records.  For tests of the tests: drop -- primitives the scan leaves out; tie_high -- the
    LATER of two equal t wins."""
    tab = lose_columns(tab, drop, INF)
    if not tie_high:
        return spe.winners(tab, sweeps)[0]
    out = spe.winners(tuple(x[:, ::-1] for x in tab), sweeps)[0]
    out["prim"] = np.where(out["prim"] >= 0, tab[0].shape[1] - 1 - out["prim"], -1)
    return out


# ---- query triangles ------------------------------------------------------------------------------------------------------

def _corner_triangle(x, y, z, up):
    """A small dyadic triangle whose corner P0 = (x, y, z) is its lowest (up = 1) or highest (up = -1) point."""
    return [[x, y, z], [x + 0.03125, y, z + up * 0.0625], [x, y + 0.03125, z + up * 0.0625]]


def triangle_batch(n_tris, rows):
    """-> (queries (n, 12) float32 {P0 xyz, d2max, P1 xyz, -, P2 xyz, -}, tags), n > 256 and no multiple of 64, shuffled.  rows:
    the STACK layout's.  tags[j] = (kind, S, index), index = the primitive the query must name on the stack layout, -1 = none:
      near        a small triangle whose nearest corner is 1/16 above petal `index`'s point, d2max = inf: t = 2^-8, that petal
      under       the same 1/16 below the point of petal S - 1: equidistant from both twins in the tie layout
      beside      on the stack's axis, 1/2 above the highest petal and 1/2 below the lowest
      fourth      the beside triangles with d2max == the squared distance of the 4th petal from there (S from above, S - 1
                  from below; closed, so the bound cuts the stack on the seam; stacks of eight only)
      nan / negative   the near triangles with d2max NaN and -1 (-1)
      general     tridistance_expect.mixed_queries of the whole scene, 260 of them, index -1 without meaning"""
    tri, d2, tags = [], [], []
    for S in placed_seams(n_tris):
        m = members(n_tris, S)
        cx, cy = CENTRE[S]
        for i in m:
            x, y = petal_point(i, S)
            for kind, radius in (("near", np.inf), ("nan", np.nan), ("negative", -1.0)):
                tri.append(_corner_triangle(x, y, petal_z(i, S) + 0.0625, 1))
                d2.append(radius)
                tags.append((kind, S, i if kind == "near" else -1))
        if S - 1 in m:
            x, y = petal_point(S - 1, S)
            tri.append(_corner_triangle(x, y, petal_z(S - 1, S) - 0.0625, -1))
            d2.append(np.inf)
            tags.append(("under", S, S - 1))
        above = _corner_triangle(cx, cy, petal_z(m[-1], S) + 0.5, 1)
        below = _corner_triangle(cx, cy, Z0 - 0.5, -1)
        tri += [above, below]
        d2 += [np.inf, np.inf]
        tags += [("beside", S, m[-1]), ("beside", S, m[0])]
        if len(m) == 8:
            for q, fourth, winner in ((above, S, m[-1]), (below, S - 1, m[0])):
                t = tde.table(tde.with_radius(queries_of([q]), INF), rows)["t"][0, fourth]
                assert t == f32(q[0][2] - petal_z(fourth, S)) ** 2
                tri.append(q)
                d2.append(t)
                tags.append(("fourth", S, winner))
    q = tde.with_radius(queries_of(tri), f32(d2)) if tri else np.zeros((0, 12), f32)
    general = tde.mixed_queries(rows, 260, 61 + n_tris)
    q = q.tolist() + general.tolist()
    tags += [("general", 0, -1)] * general.shape[0]
    _pad(q, tags)
    order = np.random.default_rng(6).permutation(len(q))
    return np.ascontiguousarray(f32(q)[order]), [tags[j] for j in order]


def triangle_table(queries, rows, edges=False, spheres=None):
    """tridistance_expect.table as a tuple (t, u, v, where, x), read-only: tie_table and lose_columns take it as they take the
    others."""
    tab = tde.table(queries, rows, edges, spheres)
    out = tuple(tab[k] for k in ("t", "u", "v", "where", "x"))
    for x in out:
        x.setflags(write=False)
    return out


def triangle_winners(tab, d2max, drop=(), tie_high=False):
    """tridistance_expect.winners' (hits, witness) on triangle_table's tuple; drop and tie_high as sweep_winners'."""
    tab = lose_columns(tab, drop, f32(np.nan))
    if tie_high:
        tab = tuple(x[:, ::-1] for x in tab)
    hits, wit = tde.winners(dict(zip(("t", "u", "v", "where", "x"), tab)), d2max)
    if tie_high:
        hits["prim"] = np.where(hits["prim"] >= 0, tab[0].shape[1] - 1 - hits["prim"], -1)
    return hits, wit


def lose_columns(tab, drop, never):
    """A table (t first) whose primitives `drop` answer `never` (the t no query accepts): a scan that loses those records."""
    if not drop:
        return tab
    out = tuple(x.copy() for x in tab)
    out[0][:, list(drop)] = never
    return out


# ---- exposure points ------------------------------------------------------------------------------------------------------

def exposure_points(n_tris):
    """(5, 8) float32 {origin, normal, tmin, tmax}, tmin = 2^-10, tmax = inf, normals -z unless said: [0] and [4] 1/2 above
    the point of petal n_tris - 1 -- the directions about straight down are blocked by that record alone, the grazing ones
    are open; [1] 1/2 above petal 1020's point: its rays finish in the first chunk or never; [2] on the axis above the stack
    that holds n_tris - 1; [3] above the other stack when there is one (else the same), with a tilted normal.  Batches of
    1, 3, 4 and 5 are its prefixes: the first point's wave is then alone with three padding waves, with two that finish early,
    in a full block, and in a second block."""
    last = n_tris - 1
    S = [s for s in placed_seams(n_tris) if last in members(n_tris, s)][0]
    other = [s for s in placed_seams(n_tris) if s != S]
    S2 = other[0] if other else S
    tmin = 2.0 ** -10
    x, y = petal_point(last, S)
    ex, ey = petal_point(1020, 1024)
    p0 = [x, y, petal_z(last, S) + 0.5, 0, 0, -1, tmin, np.inf]
    p1 = [ex, ey, petal_z(1020, 1024) + 0.5, 0, 0, -1, tmin, np.inf]
    p2 = [CENTRE[S][0], CENTRE[S][1], max(petal_z(i, S) for i in members(n_tris, S)) + 0.5, 0, 0, -1, tmin, np.inf]
    p3 = [CENTRE[S2][0], CENTRE[S2][1], max(petal_z(i, S2) for i in members(n_tris, S2)) + 0.5, 0.6, 0, -0.8, tmin, np.inf]
    return np.ascontiguousarray([p0, p1, p2, p3, p0], f32)


# ---- the reference's winners from a hit table -------------------------------------------------------------------------------

def tie_table(table, info):
    """The hit table of the TIE layout from the stack layout's, for the same rays: column S is column S - 1's (the same
    function on the same operands gives the same bits); every other record is the same triangle in both layouts."""
    out = tuple(x.copy() for x in table)
    for S in (s for s in SEAMS if s < info["n_tris"]):
        for x in out:
            x[:, S] = x[:, S - 1]
    return out


def winners(table, nearest=False, drop=(), tie_high=False):
    """query_expect.expected_hits folded over a hit table with u and v (allhits_expect.hit_table_uv; triangles, then spheres): the
    primitives in order, strict comparisons, the first scanned keeps a tie.  For tests of the tests: drop -- primitives the
    scan leaves out (a kernel that loses a record); tie_high -- the LATER of two equal t wins (<= in place of <)."""
    hit, t, u, v = table
    n, P = hit.shape
    best_t = np.full(n, FLT_MAX if nearest else -FLT_MAX, f32)
    best = np.full(n, -1, np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(P):
            if j in drop:
                continue
            tj = t[:, j]
            if nearest:
                better = (tj > 0) & ((tj <= best_t) if tie_high else (tj < best_t))
            else:
                better = (best_t <= tj) if tie_high else (best_t < tj)
            better &= hit[:, j]
            best_t = np.where(better, tj, best_t)
            best = np.where(better, j, best)
    out = np.zeros(n, HIT_DTYPE)
    out["prim"] = -1
    r = np.nonzero(best >= 0)[0]
    out["t"][r], out["u"][r], out["v"][r], out["prim"][r] = best_t[r], u[r, best[r]], v[r, best[r]], best[r]
    return out


def drop_columns(table, drop):
    """A hit table whose primitives `drop` hit nothing: what every table-based expectation sees when a record is lost."""
    out = tuple(x.copy() for x in table)
    out[0][:, list(drop)] = False
    return out
