"""Test side of the signed point queries (rt_tracer_signed_distance, rt_tracer_closest_sides; csrc/rt_features_host.hpp,
csrc/rt_sides.hpp): an independent numpy float64 construction of the feature table; the side arithmetic of
include/rt_mi355x.h in float32, operation by operation, on top of closest_expect.closest_triangle (which reports the region);
small closed meshes with an analytic inside test each, and one open mesh.  A helper, not a test.  Everything is deterministic and
needs no device."""
import numpy as np

import closest_expect as ce
from query_accel_expect import records_of_rows
from query_expect import dot3 as _dot, tri_rows as _rows

f32 = np.float32
SIDE_DTYPE = np.dtype([("s", np.float32), ("feature", np.int32)])
FEATURE_NONE, FEATURE_SPHERE = -1, 7
# closest_triangle's region 1..7 -> the feature: 0 the face, 1-3 the vertices A, B, C, 4-6 the edges AB, AC, BC
FEATURE_OF_REGION = np.array([-1, 1, 2, 4, 3, 5, 6, 0])
TABLE_TOL = 2.0 ** -22          # components are <= 1 and rounded once (2^-24); the margin is a last-bit atan2 difference


# ---- the table, float64, written independently ----------------------------------------------------------------------------

def corners(rows, edges=False):
    """(T, 3, 3) float32 corners A, B, C as the table welds them: the uploaded vertices, or fp32 v0, v0 + e1, v0 + e2."""
    r = np.ascontiguousarray(rows, f32).reshape(-1, 3, 4)[:, :, :3]
    if not edges:
        return r.copy()
    with np.errstate(all="ignore"):
        return np.stack([r[:, 0], r[:, 0] + r[:, 1], r[:, 0] + r[:, 2]], 1).astype(f32)


def _key(v):
    return (v + f32(0.0)).tobytes() if not np.isnan(v).any() else v.tobytes()      # (-0 + 0 = +0: welds with +0)


def feature_table64(rows, edges=False):
    """(T, 7, 4) float32: face, vertex (angle-weighted) and edge (plain sum) unit pseudonormals, float64 throughout, rounded
    once.  Dictionaries keyed by the vertices' bits; triangles are visited in ascending index, so the sums are."""
    P32 = corners(rows, edges)
    P = P32.astype(np.float64)
    T = P.shape[0]
    out = np.zeros((T, 7, 4), f32)

    def unit(v):
        with np.errstate(all="ignore"):
            l = np.sqrt((v * v).sum())
            return v / l if (l > 0 and np.isfinite(l)) else np.zeros(3)

    with np.errstate(all="ignore"):
        face = np.array([unit(np.cross(P[i, 1] - P[i, 0], P[i, 2] - P[i, 0])) for i in range(T)]).reshape(T, 3)
    good = np.isfinite(face).all(axis=1) & (face != 0).any(axis=1)
    face[~good] = 0.0
    keys = [[_key(P32[i, c]) for c in range(3)] for i in range(T)]
    vsum, esum = {}, {}
    pairs = ((0, 1), (0, 2), (1, 2))
    for i in np.nonzero(good)[0]:
        for c in range(3):
            a, b = P[i, (c + 1) % 3] - P[i, c], P[i, (c + 2) % 3] - P[i, c]
            ang = np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)
            vsum[keys[i][c]] = vsum.get(keys[i][c], 0.0) + ang * face[i]
        for x, y in pairs:
            k = frozenset((keys[i][x], keys[i][y]))
            esum[k] = esum.get(k, 0.0) + face[i]
    zero = np.zeros(3)
    for i in range(T):
        out[i, 0, :3] = face[i]
        for c in range(3):
            out[i, 1 + c, :3] = unit(np.asarray(vsum.get(keys[i][c], zero)))
        for e, (x, y) in enumerate(pairs):
            out[i, 4 + e, :3] = unit(np.asarray(esum.get(frozenset((keys[i][x], keys[i][y])), zero)))
    return out


# ---- the side arithmetic, float32 ---------------------------------------------------------------------------------------------

def sides_of(pts, prim, rows, table, edges=False, spheres=None, normal_of=None):
    """rt_side of (point i, primitive prim[i]): pts (n, >=3), prim (n,) int -> SIDE_DTYPE (n,).  The triangle rule of
    closest_expect.closest_triangle gives u, v and the region; r = (ap - u*e1) - v*e2 and s = (r.x*N.x + r.y*N.y) + r.z*N.z in
    float32.  normal_of(prim, feature) -> (m, 3) replaces the table look-up (the tests' wrong pipelines)."""
    p = np.asarray(pts, f32).reshape(-1, np.shape(pts)[-1])[:, :3]
    prim = np.asarray(prim, np.int64).reshape(-1)
    n_tris = 0 if rows is None else len(rows) // 3
    n_sph = 0 if spheres is None else len(spheres)
    out = np.zeros(p.shape[0], SIDE_DTYPE)
    out["feature"] = FEATURE_NONE
    tri = np.nonzero((prim >= 0) & (prim < n_tris))[0]
    with np.errstate(all="ignore"):
        if tri.size:
            v0, e1, e2 = records_of_rows(rows, edges)
            tab = np.asarray(table, f32).reshape(-1, 7, 4)
            for c0 in range(0, tri.size, 256):                               # (P, T) tables of 256 points at a time
                idx = tri[c0:c0 + 256]
                uniq, inv = np.unique(prim[idx], return_inverse=True)
                _, u, v, reg = ce.closest_triangle(p[idx], v0[uniq], e1[uniq], e2[uniq])
                k = np.arange(idx.size)
                u, v, feat = u[k, inv], v[k, inv], FEATURE_OF_REGION[reg[k, inv]]
                V0, E1, E2 = v0[prim[idx]], e1[prim[idx]], e2[prim[idx]]
                r = [((p[idx, a] - V0[:, a]) - u * E1[:, a]) - v * E2[:, a] for a in range(3)]
                N = tab[prim[idx], feat, :3] if normal_of is None else np.asarray(normal_of(prim[idx], feat), f32)
                s = _dot(r, [N[:, 0], N[:, 1], N[:, 2]])
                assert s.dtype == f32
                out["s"][idx], out["feature"][idx] = s, feat
        sph = np.nonzero((prim >= n_tris) & (prim < n_tris + n_sph))[0]
        if sph.size:
            S = np.asarray(spheres, f32).reshape(-1, 4)[prim[sph] - n_tris]
            w = [p[sph, a] - S[:, a] for a in range(3)]
            s = np.sqrt(_dot(w, w)) - S[:, 3]
            assert s.dtype == f32
            out["s"][sph], out["feature"][sph] = s, FEATURE_SPHERE
    return out


def expected_sides(pts, hits, rows, table, edges=False, spheres=None):
    """The sides of records the point queries returned: hits HIT_DTYPE (n,) or (n, k) -> SIDE_DTYPE of that shape."""
    h = np.asarray(hits)
    p = np.asarray(pts, f32).reshape(-1, np.shape(pts)[-1])[:, :3]
    per = 1 if h.ndim == 1 else h.shape[1]
    return sides_of(np.repeat(p, per, axis=0), h["prim"].reshape(-1), rows, table, edges, spheres).reshape(h.shape)


def same_sides(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def face_normal_of(table):
    """normal_of for sides_of: the winner's face normal whatever the feature -- the pipeline the table exists to replace."""
    tab = np.asarray(table, f32).reshape(-1, 7, 4)
    return lambda prim, feat: tab[prim, 0, :3]


# ---- meshes -------------------------------------------------------------------------------------------------------------------

def _prism(poly, cap_tris, z0, z1):
    """A closed prism over a counter-clockwise polygon, wound outward: caps from cap_tris (index triples, counter-clockwise),
    two triangles per side."""
    lo = [np.r_[p, z0] for p in poly]
    hi = [np.r_[p, z1] for p in poly]
    tris = []
    for a, b, c in cap_tris:
        tris.append([hi[a], hi[b], hi[c]])
        tris.append([lo[a], lo[c], lo[b]])
    m = len(poly)
    for a in range(m):
        b = (a + 1) % m
        tris.append([lo[a], lo[b], hi[b]])
        tris.append([lo[a], hi[b], hi[a]])
    return np.asarray(tris, np.float64)


CUBE_LO, CUBE_HI = np.array([-0.3, 0.1, -0.7]), np.array([0.7, 1.1, 0.3])


def cube():
    """A unit cube, 12 triangles wound outward, at coordinates that are no dyadic numbers."""
    x0, y0 = CUBE_LO[:2]
    x1, y1 = CUBE_HI[:2]
    return _rows(_prism([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [(0, 1, 2), (0, 2, 3)], CUBE_LO[2], CUBE_HI[2]))


def cube_inside(p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return ((p > CUBE_LO) & (p < CUBE_HI)).all(axis=1)


# The L: its notch at (1, 1) is ACUTE (about 59 degrees between the walls that meet there), so the outward normals of those two
# walls are obtuse to each other and a point inside the solid next to the concave edge lies in front of one wall's plane.
L_POLY = [(0.0, 0.0), (2.0, 0.0), (2.0, 1.0), (1.0, 1.0), (1.6, 2.0), (0.0, 2.0)]
L_CAPS = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]
L_Z = (-0.25, 0.75)


def l_prism():
    """An L-shaped prism (20 triangles, wound outward) with one concave edge and two concave vertices."""
    return _rows(_prism(L_POLY, L_CAPS, *L_Z))


def _in_polygon(x, y, poly):
    """Crossing number, float64."""
    inside = np.zeros(x.shape, bool)
    m = len(poly)
    for a in range(m):
        (xa, ya), (xb, yb) = poly[a], poly[(a + 1) % m]
        if ya == yb:
            continue
        cross = ((ya > y) != (yb > y)) & (x < (xb - xa) * (y - ya) / (yb - ya) + xa)
        inside ^= cross
    return inside


def l_prism_inside(p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return _in_polygon(p[:, 0], p[:, 1], L_POLY) & (p[:, 2] > L_Z[0]) & (p[:, 2] < L_Z[1])


SPIKE = np.array([[0.05, 0.0, 0.0], [-0.025, 0.0433, 0.0], [-0.025, -0.0433, 0.0], [0.01, -0.005, 2.0]])


def spike():
    """A thin tetrahedron (base radius 0.05, height 2, wound outward): at the apex the three long faces' normals are mutually
    obtuse (about 120 degrees apart), so next to the apex, outside, a point is behind the plane of at least one of them."""
    a, b, c, d = SPIKE
    return _rows(np.asarray([[a, c, b], [a, b, d], [b, c, d], [c, a, d]]))


def spike_inside(p):
    """Inside all four planes, float64."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    t = corners(spike()).astype(np.float64)
    inside = np.ones(p.shape[0], bool)
    for tri in t:
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        inside &= ((p - tri[0]) @ n) < 0
    return inside


def square():
    """An open mesh: a two-triangle square in the plane z = 0.5, normal +z; its four outer edges are boundary edges."""
    q = np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [1.0, 1.0, 0.5], [0.0, 1.0, 0.5]])
    return _rows(np.asarray([[q[0], q[1], q[2]], [q[0], q[2], q[3]]]))


def closed_meshes():
    """{name: (rows, inside test)}."""
    return {"cube": (cube(), cube_inside), "l_prism": (l_prism(), l_prism_inside), "spike": (spike(), spike_inside)}


def probe_points(rows, n_random=3000, seed=61, eps=(3e-3, 3e-2)):
    """(m, 3) float32: n_random points uniform in the mesh's box grown by a quarter of its size, plus, for every vertex and every
    edge midpoint of the mesh, points eps away in 26 general directions, each with its opposite (towards the inside and the outside alike)."""
    P = corners(rows).astype(np.float64)
    lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    pad = 0.25 * (hi - lo).max()
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(lo - pad, hi + pad, (n_random, 3))]
    verts = np.unique(P.reshape(-1, 3), axis=0)
    mids = np.unique(np.concatenate([(P[:, a] + P[:, b]) / 2 for a, b in ((0, 1), (0, 2), (1, 2))]), axis=0)
    dirs = rng.normal(0, 1, (13, 3))                             # general directions (an axis direction would run inside a wall)
    dirs = np.concatenate([dirs, -dirs])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    for base in (verts, mids):
        for e in eps:
            pts.append((base[:, None, :] + e * dirs[None, :, :]).reshape(-1, 3))
    return np.ascontiguousarray(np.concatenate(pts), f32)


def far_enough(pts, rows, least=1e-4):
    """(m,) bool: the point is more than `least` from the surface (float64 distance): its side is decided."""
    return ce.distance64(np.asarray(pts, f32)[:, :3], rows).min(axis=1) > least
