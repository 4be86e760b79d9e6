"""Test side of the ray queries (RayTracer.Intersect / Pick / FocusAt): what every query must return, computed as a
scan in upload order with the oracle's HitTriangle and ray-sphere test, and the adversarial rays the GPU tests use."""
import ctypes as C

import numpy as np

HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("prim", np.int32)])
FLT_MAX = np.float32(np.finfo(np.float32).max)


def tri_rows(tris):
    """(n, 3, 3) triangles as (3n, 4) float32 upload rows."""
    r = np.zeros((len(tris), 3, 4), np.float32)
    r[:, :, :3] = tris
    return r.reshape(-1, 4)


def dot3(a, b):
    """a . b of two triples of broadcastable arrays, as the kernels round it: (a0 b0 + a1 b1) + a2 b2."""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    """a x b of two triples of broadcastable arrays, each component two separately rounded products and a difference."""
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def expected_hits(orc, rays, tri_rows, spheres=None, contract=None, nearest=False):
    """The farthest-hit (or nearest t > 0) scan of Kernels.cuh:73-92 for rays (n, 6) against absolute triangle rows
    (3N, 4) then spheres (M, 4): triangles in order, then spheres, strict comparisons (first scanned wins ties).
    Returns a HIT_DTYPE array: prim = triangle index, N + sphere index or -1; t/u/v of the winner, 0 without a hit.
    contract: the oracle's arithmetic (orc.FMA, the default, or orc.STRICT)."""
    contract = orc.FMA if contract is None else contract
    L = orc.lib()
    f3 = C.c_float * 3
    tris = np.ascontiguousarray(np.asarray(tri_rows, np.float32).reshape(-1, 3, 4)[:, :, :3])
    sph = np.ascontiguousarray(np.zeros((0, 4), np.float32) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 4))
    verts = [[f3(*map(float, tris[j, k])) for k in range(3)] for j in range(tris.shape[0])]
    sphs = [(C.c_float * 4)(*map(float, s)) for s in sph]
    rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 6))
    out = np.zeros(rays.shape[0], HIT_DTYPE)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    fp = C.POINTER(C.c_float)
    for i in range(rays.shape[0]):
        ray = rays[i].ctypes.data_as(fp)
        best_t, best, bu, bv = (FLT_MAX if nearest else -FLT_MAX), -1, np.float32(0), np.float32(0)
        for j, (a, b, c) in enumerate(verts):
            if not L.orc_hit_triangle(ray, a, b, c, contract, 0, C.byref(t), C.byref(u), C.byref(v)):
                continue
            tj = np.float32(t.value)
            if (tj > 0 and tj < best_t) if nearest else (best_t < tj):
                best_t, best, bu, bv = tj, j, np.float32(u.value), np.float32(v.value)
        for s, sp in enumerate(sphs):
            if not L.orc_hit_sphere(ray, sp, contract, C.byref(t)):
                continue
            ts = np.float32(t.value)
            if (ts > 0 and ts < best_t) if nearest else (best_t < ts):
                best_t, best, bu, bv = ts, tris.shape[0] + s, np.float32(0), np.float32(0)
        if best >= 0:
            out[i] = (best_t, bu, bv, best)
        else:
            out[i] = (0, 0, 0, -1)
    return out


def same_hits(a, b):
    """Bit-exact equality of two HIT_DTYPE arrays (t, u, v compared as bit patterns, NaN included)."""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(b).view(np.uint32).reshape(-1, 4)
    return a.shape == b.shape and np.array_equal(a, b)


def edge_rows(tri_rows):
    """The same triangles as (v0, e0 = v1 - v0, e1 = v2 - v0) rows, differences in fp32 (rt_tracer_upload_scene_edges)."""
    t = np.asarray(tri_rows, np.float32).reshape(-1, 3, 4).copy()
    e0 = t[:, 1, :3] - t[:, 0, :3]
    e1 = t[:, 2, :3] - t[:, 0, :3]
    t[:, 1, :3], t[:, 2, :3] = e0, e1
    t[:, :, 3] = 0.0
    return t.reshape(-1, 4)


def adversarial_scene(n_tris, seed, behind=True):
    """n_tris triangles in front of the origin (some duplicated), and optionally a few behind it (z > 0), both windings."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-3, 3, n_tris), rng.uniform(-3, 3, n_tris), rng.uniform(-12, -3, n_tris)], 1)
    v = c[:, None, :] + rng.uniform(-1.2, 1.2, (n_tris, 3, 3))
    if n_tris >= 4:
        v[n_tris // 2] = v[1]                        # a duplicated triangle: the lower index wins under both rules
        v[n_tris - 1] = v[n_tris // 3][[0, 2, 1]]    # the other winding of another one
    if behind and n_tris >= 8:
        for j in range(n_tris - 4, n_tris - 1):      # behind the origin: hits with t < 0 only
            v[j, :, 2] = -v[j, :, 2]
    rows = np.zeros((n_tris, 3, 4), np.float32)
    rows[:, :, :3] = v
    return rows.reshape(-1, 4)


def adversarial_rays(tri_rows, n_random, seed):
    """Rays through vertices and edge midpoints, with det near 1e-10, huge and tiny magnitudes, NaN / inf components, a
    zero direction, rays that only hit behind their origin, and random rays, as (n, 6) float32."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tri_rows, np.float32).reshape(-1, 3, 4)[:, :, :3]
    out = []
    o = np.zeros(3, np.float32)
    for j in range(min(tris.shape[0], 24)):
        a, b, c = tris[j]
        for target in (a, b, c, (a + b) / 2, (b + c) / 2, (a + c) / 2, (a + b + c) / 3):
            d = np.float32(target) - o
            out.append(np.r_[o, d])
            out.append(np.r_[o, d * np.float32(1e30)])
            out.append(np.r_[o, d * np.float32(1e-30)])
            out.append(np.r_[target - d * np.float32(0.5), -d])       # the same point, seen from beyond it
        e1, e2 = b - a, c - a
        n = np.cross(e1, e2)
        for eps in (1e-12, 1e-10, 1.0001e-10, 1e-9, 0.0):              # nearly in the triangle's plane: det ~ eps
            d = e1 + np.float32(eps) * n / max(np.float32(np.dot(n, n)), np.float32(1e-30))
            out.append(np.r_[a - d * np.float32(0.3) + np.float32(1e-3) * e2, d])
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            r = np.r_[o, np.float32([0.1, 0.2, -1.0])]
            r[k] = bad
            out.append(r)
    out.append(np.r_[o, np.zeros(3, np.float32)])                      # zero direction
    out.append(np.r_[np.float32([0, 0, -30]), np.float32([0, 0, -1])]) # everything behind the origin
    out.append(np.r_[np.float32([0, 0, -30]), np.float32([0, 0, 1])])
    org = rng.uniform(-2, 2, (n_random, 3)).astype(np.float32)
    tgt = tris[rng.integers(0, tris.shape[0], n_random)].mean(axis=1) + rng.normal(0, 0.6, (n_random, 3)).astype(np.float32)
    dirs = (tgt - org) * rng.choice(np.float32([1.0, -1.0, 0.37]), (n_random, 1)).astype(np.float32)
    out.extend(np.c_[org, dirs])
    return np.ascontiguousarray(np.asarray(out, np.float32))
