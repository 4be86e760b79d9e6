"""Scenes and ray populations of the lattice tests (test_lattice_expect.py without a device, test_gpu_query_lattice.py on
one): the geometry the ray queries are for and the other query tests do not contain -- axis-aligned walls, whose child boxes
are flat; rays that run inside a wall's plane or parallel to an axis; origins on a surface with tmin = 0; and exact ties on t
between triangles of different leaves.  Every coordinate is a small dyadic number, so the reference's triangle test is exact for
the lattice rays under both arithmetic modes and a tie is a tie bit for bit.  Everything is deterministic."""
import ctypes as C

import numpy as np

from occluded_expect import with_interval
from query_accel_expect import EMPTY, RHO, populations
from query_expect import HIT_DTYPE, expected_hits, tri_rows as _rows

INF = np.float32(np.inf)
SHIFT = 1.75                                   # the walls lie on k - SHIFT: the world origin is a quarter point of a cell
EPS20 = np.float32(2.0 ** -20)

AXES = [tuple(float(s) if k == a else 0.0 for k in range(3)) for a in range(3) for s in (1, -1)]
FACE_DIAGONALS = [tuple(float(v) for v in (x, y, z)) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)
                  if abs(x) + abs(y) + abs(z) == 2]
SPACE_DIAGONALS = [(float(x), float(y), float(z)) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
DIRECTIONS = np.float32(AXES + FACE_DIAGONALS + SPACE_DIAGONALS)               # 6 + 12 + 8, each with its opposite


# ---- the scenes ---------------------------------------------------------------------------------------------------------

def rooms(n=4, seed=7):
    """The walls of an n x n x n lattice of unit cells: one quad per cell face on the planes x, y, z = k - SHIFT (k = 0..n), two
    triangles per quad, the diagonal alternating with the parity of the quad's position and the winding with another parity, in
    an upload order shuffled by a fixed permutation.  3 (n + 1) n^2 quads: 240 quads, 480 triangles for n = 4.
    (3N, 4) float32 upload rows."""
    tris = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in range(n + 1):
            for i in range(n):
                for j in range(n):
                    p = np.zeros((4, 3))
                    p[:, a] = k
                    p[:, b] = [i, i + 1, i + 1, i]
                    p[:, c] = [j, j, j + 1, j + 1]
                    p -= SHIFT
                    pair = ((0, 1, 2), (0, 2, 3)) if (i + j + k) % 2 == 0 else ((1, 2, 3), (1, 3, 0))
                    flip = (i + 2 * j + 3 * k + a) % 4 in (1, 2)
                    for t in pair:
                        t = (t[0], t[2], t[1]) if flip else t
                        tris.append(p[list(t)])
    tris = np.asarray(tris)
    return _rows(tris[np.random.default_rng(seed).permutation(tris.shape[0])])


def copies(k=33, others=64, seed=9):
    """One triangle uploaded k times, and two coplanar ones that overlap it (to its right and to its left) uploaded 9 times each,
    at scattered upload indices among `others` triangles in general position.  The builder keeps equal centres in upload order,
    so a tie among copies of ONE triangle is met lowest index first by any traversal; a tie between two of the triangles is met
    in the order of their leaves' boxes, which depends on the ray and on the hit rule.  The lowest upload index of all belongs to
    the second triangle, the next one to the first, and every copy of the third comes after that: whichever of two groups a
    traversal enters first, one of the two overlaps has its winner in the other.
    Returns (rows, first, second, third): the ascending upload indices of the copies."""
    rng = np.random.default_rng(seed)
    first = np.array([[-1.0, -1.0, -6.0], [1.0, -1.0, -6.0], [0.0, 1.0, -6.0]])
    second = np.array([[-0.5, -0.5, -6.0], [1.5, -0.5, -6.0], [0.5, 1.5, -6.0]])
    third = np.array([[-1.5, -0.5, -6.0], [0.5, -0.5, -6.0], [-0.5, 1.5, -6.0]])
    c = np.stack([rng.uniform(-3, 3, others), rng.uniform(-3, 3, others), rng.uniform(-12, -3, others)], 1)
    general = c[:, None, :] + rng.uniform(-1.2, 1.2, (others, 3, 3))
    total = k + 18 + others
    perm = rng.permutation(total)
    low = np.sort(perm[:k + 18])[:2]                                      # the two lowest indices of all the copies
    rest = perm[:k + 18][~np.isin(perm[:k + 18], low)]
    i1, i2, i3 = np.r_[low[1], rest[:k - 1]], np.r_[low[0], rest[k - 1:k + 7]], rest[k + 7:]
    tris = np.zeros((total, 3, 3))
    tris[i1], tris[i2], tris[i3] = first, second, third
    tris[perm[k + 18:]] = general
    return _rows(tris), np.sort(i1), np.sort(i2), np.sort(i3)


# ---- ray populations of rooms() -------------------------------------------------------------------------------------------

def _centres(n=4):
    """Cell centres spread over the lattice (a fixed choice: corners, middle and edge cells)."""
    cells = [(0, 0, 0), (2, 1, 2), (3, 3, 3), (1, 1, 1), (0, 3, 1), (2, 2, 0), (1, 0, 3), (3, 1, 2)]
    return np.float32([[i + 0.5 - SHIFT, j + 0.5 - SHIFT, k + 0.5 - SHIFT] for i, j, k in cells if max(i, j, k) < n])


def _rays(o, d):
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[o, d], np.float32)


def axis_rays(n=4):
    """From cell centres and quarter points along +-e_k times 1, 0.37 and 4; each direction twice, with +0.0 and with -0.0 in
    its two zero components (1 / -0.0 = -inf swaps the two planes of a slab)."""
    org = np.concatenate([_centres(n)[:3], _centres(n)[:2] + np.float32([0.25, -0.25, 0.25]), np.zeros((1, 3), np.float32)])
    out = []
    for o in org:
        for e in np.float32(AXES):
            for s in np.float32([1.0, 0.37, 4.0]):
                d = e * s
                for zero in np.float32([0.0, -0.0]):
                    out.append(np.r_[o, np.where(e != 0, d, zero)])
    return np.ascontiguousarray(out, np.float32)


def in_plane_rays(n=4):
    """Origins exactly on a wall plane -- in the interior of a face, on a lattice line and on a lattice vertex -- with the eight
    directions inside that plane (two axes, four face diagonals, with their opposites).  A ray along a lattice line lies in two
    planes and runs through the shared edges of four quads.  The zero of the normal component is -0.0 for every second ray."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in ((0, 2, n) if a == 0 else (2,)):                          # an outer wall on either side, and inner ones
            for ob, oc in ((1.25, 2.5), (1.0, 2.25), (2.0, 1.0)):          # face interior, lattice line, lattice vertex
                o = np.zeros(3, np.float32)
                o[a], o[b], o[c] = k - SHIFT, ob - SHIFT, oc - SHIFT
                for d in DIRECTIONS:
                    if d[a] == 0 and (d != 0).sum() <= 2:
                        d = d.copy()
                        d[a] = -0.0 if len(out) % 2 else 0.0
                        out.append(np.r_[o, d])
    return np.ascontiguousarray(out, np.float32)


def padded_plane_rays(nodes, rho=RHO, count=12):
    """Rays inside a PADDED slab plane of a flat child box of a dumped tree.  The box test pads every box by rho (max|o| + cmax)
    before it subtracts the origin, so an origin on the wall itself never gives (lo - pad) - o = 0; one at lo - pad (or hi +
    pad), which these dyadic coordinates hold exactly, does, and with a zero direction component on that axis the product is
    0 * inf: the NaN for which the traversal takes no pruning decision.  The other two coordinates are the box's centre;
    directions: the axes and face diagonals inside the plane, the zero given as +0.0 and as -0.0."""
    out, boxes = [], 0
    for nd in nodes:
        for c in range(4):
            if nd["child"][c] == EMPTY or boxes >= count:
                continue
            lo, hi = nd["lo"][:, c], nd["hi"][:, c]
            flat = np.nonzero(lo == hi)[0]
            if flat.size != 1:
                continue
            a = int(flat[0])
            o = ((lo + hi) * np.float32(0.5)).astype(np.float32)
            omax = np.abs(np.delete(o, a)).max()
            pad = np.float32(rho) * (omax + nd["cmax"][c])
            o[a] = (lo[a] - pad) if boxes % 2 else (hi[a] + pad)
            edge = (lo[a] - pad) if boxes % 2 else (hi[a] + pad)
            if np.abs(o).max() != omax or np.float32(edge - o[a]) != 0:
                continue
            boxes += 1
            for d in DIRECTIONS[(DIRECTIONS[:, a] == 0) & ((DIRECTIONS != 0).sum(axis=1) <= 2)][boxes % 2::2]:
                d = d.copy()
                d[a] = -0.0 if len(out) % 2 else 0.0
                out.append(np.r_[o, d])
    return np.ascontiguousarray(out, np.float32).reshape(-1, 6)


def vertex_rays(n=4):
    """From cell centres along the space diagonals (+-1, +-1, +-1) / 2 and the face diagonals: the hits lie exactly on lattice
    vertices and edge midpoints, where the triangles of several quads tie on t."""
    d = np.float32(FACE_DIAGONALS + SPACE_DIAGONALS) * np.float32(0.5)
    return np.concatenate([_rays(np.repeat(o[None], d.shape[0], 0), d) for o in _centres(n)])


def surface_points(orc, rows, rays, count=12, contract=None):
    """`count` distinct points o + t d (fp32) of the oracle's nearest hits of `rays`, spread over them."""
    near = expected_hits(orc, rays, rows, None, contract, nearest=True)
    m = near["prim"] >= 0
    pts = (rays[m, :3] + near["t"][m, None] * rays[m, 3:]).astype(np.float32)
    _, first = np.unique(pts.view(np.uint32), axis=0, return_index=True)
    pts = pts[np.sort(first)]
    return np.ascontiguousarray(pts[np.linspace(0, pts.shape[0] - 1, min(count, pts.shape[0])).astype(np.int64)])


def on_surface_rays(points):
    """Every point relaunched in each of the 26 axis, face-diagonal and space-diagonal directions: into the room, out of it and
    along the wall the point sits on."""
    return np.concatenate([_rays(np.repeat(p[None], DIRECTIONS.shape[0], 0), DIRECTIONS) for p in points])


def pair_points(points, n=4):
    """(a, b) for Visible: from every surface point to the points 1 and 3 cells on in each of the 26 directions, where that is
    still inside the lattice -- on the same wall (a direction inside it), on the opposite wall of one cell, on walls several
    cells apart -- and to itself."""
    lo, hi = np.float32(-SHIFT), np.float32(n - SHIFT)
    a, b = [], []
    for p in points:
        for m in np.float32([1.0, 3.0]):
            for d in DIRECTIONS:
                q = (p + m * d).astype(np.float32)
                if (q >= lo).all() and (q <= hi).all():
                    a.append(p)
                    b.append(q)
        a.append(p)
        b.append(p.copy())
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def pair_rays(a, b):
    """The rays Visible makes of the pairs: o = a, d = b - a in fp32."""
    return _rays(a, b - a)


PAIR_FAMILIES = ("unit", "short_of_b", "past_a", "at_a_hit", "empty")


def pair_segments(rays, table):
    """The interval families of the pairs as {name: (n, 8)}: [0, 1], [0, 1 - 2^-20], [2^-20, 1], [t, t] for a t the oracle lists
    for the ray (the middle one of its hits; [1, 1] for a ray without a hit) and tmin > tmax.  table: a hit table of the rays."""
    hit, t = table[0], table[1]
    n = rays.shape[0]
    at = np.ones(n, np.float32)
    for i in range(n):
        ts = np.sort(t[i][hit[i]])
        if ts.size:
            at[i] = ts[ts.size // 2]
    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    fam = {"unit": (zero, one), "short_of_b": (zero, one - EPS20), "past_a": (zero + EPS20, one), "at_a_hit": (at, at),
           "empty": (one, zero)}
    return {k: with_interval(rays, lo, hi) for k, (lo, hi) in fam.items()}


def hits_from_table(table, nearest=False):
    """The scan's winners from a hit table with u and v (allhits_expect.hit_table_uv), for finite rays: the largest t (nearest:
    the smallest t > 0) of each row, equal t to the lowest upload index -- what first-scanned-wins gives in upload order."""
    hit, t, u, v = table
    out = np.zeros(hit.shape[0], HIT_DTYPE)
    out["prim"] = -1
    ok = hit & (t > 0) if nearest else hit
    key = np.where(ok, t, INF if nearest else -INF)
    best = key.min(axis=1) if nearest else key.max(axis=1)
    win = np.argmax(ok & (key == best[:, None]), axis=1)                 # the first index at the best t
    m = ok.any(axis=1)
    r = np.nonzero(m)[0]
    out["t"][r], out["u"][r], out["v"][r], out["prim"][r] = t[r, win[r]], u[r, win[r]], v[r, win[r]], win[r]
    return out


def ray_segments(rays):
    """Intervals for a population of rays, by turns: [0, inf] (a shadow or continuation ray), every t, and [0, 1]."""
    n = rays.shape[0]
    lo = np.where(np.arange(n) % 3 == 1, -INF, np.float32(0)).astype(np.float32)
    hi = np.where(np.arange(n) % 3 == 2, np.float32(1), INF).astype(np.float32)
    return with_interval(rays, lo, hi)


def control_rays(rows, n=24, seed=21):
    """n rays of each population of query_accel_expect.populations, in one array: general directions, the ordinary rule."""
    return np.concatenate(list(populations(rows, n, seed).values()))


def rooms_populations(orc, rows, nodes, contract=None, n=4):
    """({name: (m, 6) rays} of rooms(): the lattice populations, then `control`; (a, b) of the pairs).  nodes: the scene's
    dumped tree, for the part of in_plane that lies in padded planes."""
    pops = {"axis": axis_rays(n), "in_plane": np.concatenate([in_plane_rays(n), padded_plane_rays(nodes)]), "vertex": vertex_rays(n)}
    pts = surface_points(orc, rows, np.concatenate([pops["axis"], pops["vertex"]]), contract=contract)
    pops["on_surface"] = on_surface_rays(pts[:8])
    ab = pair_points(pts[1::2][:5], n)
    pops["pairs"] = pair_rays(*ab)
    pops["control"] = control_rays(rows)
    return pops, ab


def cornell_populations(orc, rows, contract=None, W=65, H=49):
    """{name: rays} of cornell32: the pinhole rays of an odd-sized frame (a centre column and row), relaunches from the points
    their nearest hits lie at, and `control`.  The boxes are rotated: every population is under the ordinary rule."""
    frame = pinhole_rays(orc, W, H, orc.FMA if contract is None else contract)
    pts = surface_points(orc, rows, frame, contract=contract)
    return {"frame": frame, "on_surface": on_surface_rays(pts), "control": control_rays(rows)}


def segments(name, rays, table):
    """(segments (m, 8), table row of each) of a population: the pairs under every family of pair_segments, any other by
    ray_segments."""
    if name != "pairs":
        return ray_segments(rays), np.arange(rays.shape[0])
    fams = pair_segments(rays, table)
    return np.concatenate([fams[k] for k in PAIR_FAMILIES]), np.tile(np.arange(rays.shape[0]), len(PAIR_FAMILIES))


LATTICE = ("axis", "in_plane", "vertex", "on_surface", "pairs")        # bit-exact populations of rooms(); "copies" of copies()


# ---- copies() and cornell32 ---------------------------------------------------------------------------------------------

def copies_rays():
    """Through the copied triangle's interior, edge midpoints and vertices, and the overlap with the second one, from both
    sides: from points of the plane z = 0 straight down, from the world origin, and from behind the plane z = -6."""
    targets = np.float32([[0, -0.25, -6], [0.25, 0, -6], [-0.25, -0.5, -6], [0.5, 0.5, -6],      # interior (the last three in both)
                          [0, -1, -6], [0.5, 0, -6], [-0.5, 0, -6],                             # edge midpoints
                          [-1, -1, -6], [1, -1, -6], [0, 1, -6],                                # vertices
                          [-0.5, -0.5, -6], [0.75, -0.5, -6], [1.25, 0, -6], [-0.75, 0, -6],   # the second one's; outside the first
                          [-0.5, 0, -6], [-0.25, 0.25, -6], [-1.25, -0.25, -6], [0, 0.5, -6]]) # in the third one
    out = []
    for p in targets:
        out.append(np.r_[p[0], p[1], 0, 0, 0, -1])
        out.append(np.r_[p[0], p[1], 0, 0, 0, -4])
        out.append(np.r_[p[0], p[1], 0, -0.0, -0.0, -0.5])
        out.append(np.r_[0, 0, 0, p])
        out.append(np.r_[0.5, -0.25, -2, p - np.float32([0.5, -0.25, -2])])
        out.append(np.r_[p[0], p[1], -12, 0, 0, 1])                      # from behind: culled, or seen with t < 0 going away
        out.append(np.r_[p[0], p[1], -12, 0, 0, -1])
        out.append(np.r_[p, 0, 0, -1])                                   # from the triangle itself: t = 0
    return np.ascontiguousarray(out, np.float32)


def pinhole_rays(orc, W, H, contract, fov=70.0, focal=3.0, aperture=0.05):
    """The pinhole rays of a W x H frame from the world origin, as RayTracer.Pick makes them (row by row)."""
    cam = orc.camera((0.0, 0.0), fov, focal, aperture)
    out = np.zeros((W * H, 6), np.float32)
    fp = C.POINTER(C.c_float)
    for y in range(H):
        for x in range(W):
            orc.lib().orc_camera_pinhole(C.byref(cam), x, y, W, H, contract, out[y * W + x].ctypes.data_as(fp))
    return out


def frame_pixels(W, H):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
    return np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], 1))
