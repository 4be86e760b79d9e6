"""Test side of the exposure query (RayTracer.Exposure / rt_tracer_exposure): the frame of include/rt_mi355x.h restated in numpy
float32 operation for operation, the segments the query traces, the packing of per-direction answers into masks, and an open-top
unit box with the analytic rule of which directions leave it."""
import numpy as np

from query_expect import tri_rows as _rows

F32 = np.float32
ONE = F32(1.0)


def frame(normals, swap=False):
    """(T, B) of (m, 3) float32 normals, each (m, 3) float32: the header's arithmetic, every operation a float32 numpy operation.
    swap (for tests of the tests): T and B exchanged, a left-handed frame."""
    n = np.asarray(normals, F32).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = np.copysign(ONE, z)
        a = F32(-1.0) / (s + z)
        b = (x * y) * a
        T = np.stack([ONE + s * ((x * x) * a), s * b, -(s * x)], axis=1)
        B = np.stack([b, s + (y * y) * a, -y], axis=1)
    assert T.dtype == F32 and B.dtype == F32
    return (B, T) if swap else (T, B)


def as_dirs4(dirs):
    """(k, 4) float32 {x, y, z, w} of (k, 3) or (k, 4) directions (w = 0 when absent)."""
    d = np.asarray(dirs, F32)
    out = np.zeros((d.shape[0], 4), F32)
    out[:, :d.shape[1]] = d
    return out


def exposure_segments(points, dirs, world=False, swap=False):
    """The (n * k, 8) float32 segments {origin, d_ij, tmin_i, tmax_i}, point-major, of (n, 8) points {origin, normal, tmin, tmax}
    and (k, 3 | 4) directions: d = ((l.x * T + l.y * B) + l.z * n) per component in float32, or l itself in world mode."""
    p = np.asarray(points, F32).reshape(-1, 8)
    l = as_dirs4(dirs)
    n, k = p.shape[0], l.shape[0]
    out = np.empty((n, k, 8), F32)
    out[:, :, :3] = p[:, None, :3]
    out[:, :, 6:] = p[:, None, 6:]
    if world:
        out[:, :, 3:6] = l[None, :, :3]
    else:
        nrm = p[:, 3:6]
        T, B = frame(nrm, swap)
        lx, ly, lz = l[None, :, 0:1], l[None, :, 1:2], l[None, :, 2:3]
        with np.errstate(all="ignore"):
            d = (lx * T[:, None, :] + ly * B[:, None, :]) + lz * nrm[:, None, :]
        assert d.dtype == F32
        out[:, :, 3:6] = d
    return out.reshape(n * k, 8)


def pack_masks(open_bool):
    """(n, k <= 64) bool -> (n,) uint64, bit j = column j."""
    o = np.asarray(open_bool, bool)
    assert o.ndim == 2 and o.shape[1] <= 64
    w = (np.uint64(1) << np.arange(o.shape[1], dtype=np.uint64))
    return (o.astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)


def unpack_masks(masks, k=64):
    """(n,) uint64 -> (n, k) bool."""
    m = np.asarray(masks, np.uint64)
    return ((m[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def popcount(masks):
    return np.unpackbits(np.ascontiguousarray(masks, np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def open_box(double_sided=True):
    """The unit box [0, 1]^3 without its lid z = 1: floor and four walls, each quad as two triangles, in both windings (the hit
    test culls back faces) -- 20 triangles.  double_sided=False: the 10 that face outward only, as the mesh of a solid is wound,
    which nothing inside the box can hit.  (3N, 4) float32 upload rows."""
    quads = [  # corners counter-clockwise seen from inside the box
        [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)],                      # floor, normal +z
        [(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1)],                      # x = 0, normal +x
        [(1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)],                      # x = 1, normal -x
        [(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)],                      # y = 0, normal +y
        [(0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)],                      # y = 1, normal -y
    ]
    tris = []
    for q in quads:
        for t in ((0, 1, 2), (0, 2, 3)):
            tris.append([q[t[0]], q[t[2]], q[t[1]]])
            if double_sided:
                tris.append([q[t[0]], q[t[1]], q[t[2]]])
    return _rows(np.asarray(tris, np.float64))


def open_box_rule(segs, rim=1e-4, flat=1e-6):
    """(open, excluded) of (m, 8) segments whose origins lie in the box: in float64, a direction is open exactly when d.z > 0 and
    the ray meets z = 1 strictly inside the unit square.  excluded: it meets the lid plane within `rim` of the square's rim, or
    |d.z| < `flat`."""
    s = np.asarray(segs, F32).reshape(-1, 8).astype(np.float64)
    o, d = s[:, :3], s[:, 3:6]
    with np.errstate(all="ignore"):
        t = (1.0 - o[:, 2]) / d[:, 2]
        x, y = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
        up = d[:, 2] > 0
        inside = up & (x > 0) & (x < 1) & (y > 0) & (y < 1)
        edge = np.minimum(np.minimum(np.abs(x), np.abs(x - 1)), np.minimum(np.abs(y), np.abs(y - 1)))
        near = up & (edge < rim) & (x > -rim) & (x < 1 + rim) & (y > -rim) & (y < 1 + rim)
    return inside, near | (np.abs(d[:, 2]) < flat)


def open_box_points(seed=5, tmin=1e-3, tmax=np.inf):
    """40 points of the open box as (40, 8) {origin, unit normal, tmin, tmax}: 20 on the floor with the normal +z, 10 inside with
    the normal +z, 10 inside with random unit normals."""
    rng = np.random.default_rng(seed)
    p = np.zeros((40, 8), F32)
    p[:, :3] = rng.uniform(0.05, 0.95, (40, 3))
    p[:20, 2] = 0.0
    p[:, 3:6] = [0.0, 0.0, 1.0]
    p[30:, 3:6] = unit_normals(10, seed + 1)
    p[:, 6], p[:, 7] = tmin, tmax
    return p


def unit_normals(m, seed):
    """m random unit vectors: normalised in float64, rounded to float32 once."""
    v = np.random.default_rng(seed).normal(0.0, 1.0, (m, 3))
    return (v / np.sqrt((v * v).sum(axis=1))[:, None]).astype(F32)


def special_normals():
    """+-x, +-y, +-z, a normal with z = -0, the zero vector and a NaN normal."""
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, -0.0], [0, 0, 0],
                     [np.nan, 0.6, 0.8]], F32)
