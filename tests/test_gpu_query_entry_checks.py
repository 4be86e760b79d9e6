"""The query entry points' argument handling through the C ABI, one table row per entry point: the 13 host / _device pairs and
rt_tracer_pick, 27 rows.  Per row, on a scene of two triangles and batches of 8: every required array refused when null; the
query's own check refused with its text, and ahead of the null-array check; n = 0 accepted with null (and, for a _device
form, misaligned) pointers; every pointer of a _device form moved off its alignment in turn and refused with the full text;
null optional pointers accepted; the outputs untouched by every refusal; and per pair the two forms' outputs byte for byte
the same on the same inputs.  Every device buffer is one row longer than a call needs, so no pointer this file passes leaves
its allocation, whatever a check does with it."""
import collections
import ctypes

import numpy as np
import pytest

import hexoverlap_expect as he

pytestmark = pytest.mark.gpu

N = 8
MAX_HITS, MAX_DIRS = 16, 64                                              # RT_MAX_HITS, RT_MAX_DIRS of include/rt_mi355x.h
SENTINEL = 0xA5
NULL_ARRAY = "query: null array"

# One array of a call: output or input, bytes per query (fixed: the bytes of the whole array, whatever n is) from the call's
# scalars, the alignment its _device form demands (1: none) and whether the caller may pass NULL under these scalars.
A = collections.namedtuple("A", "out bytes align optional fixed", defaults=(lambda s: False, False))
# One pair: the host form's name, the C arguments in order (array names, "n", scalar names), the arrays, the scalars of a
# well-formed call, the query's own checks as (scalars that break it, text after "<entry point>: ") and the _device form's
# alignment text after "<entry point>_device: ".
Q = collections.namedtuple("Q", "name args arrays scalars checks misaligned")


def _rows(k):
    return lambda s: k * s["max_hits"]


ROW_CHECKS = [({"max_hits": 0}, "max_hits = 0 (1 to 16)"), ({"max_hits": MAX_HITS + 1}, "max_hits = 17 (1 to 16)")]
REGION_CHECKS = [({"max_hits": MAX_HITS + 1}, "max_hits = 17 (0 to 16)")]


def _region(name, array, floats):
    return Q(name, (array, "after", "n", "max_hits", "prims", "counts"),
             {array: A(False, lambda s: 4 * floats, 16), "after": A(False, lambda s: 4, 4, lambda s: True),
              "prims": A(True, _rows(4), 4, lambda s: s["max_hits"] == 0), "counts": A(True, lambda s: 4, 4)},
             {"max_hits": 4}, REGION_CHECKS, "%s must be 16-byte aligned, after, prims and counts 4-byte aligned" % array)


PAIRS = [
    Q("rt_tracer_intersect", ("rays", "n", "hits"), {"rays": A(False, lambda s: 24, 4), "hits": A(True, lambda s: 16, 16)},
      {}, [], "hits must be 16-byte aligned, rays 4-byte aligned"),
    Q("rt_tracer_occluded", ("segs", "n", "occluded"), {"segs": A(False, lambda s: 32, 16), "occluded": A(True, lambda s: 1, 1)},
      {}, [], "segs must be 16-byte aligned"),
    Q("rt_tracer_exposure", ("points", "n", "dirs", "n_dirs", "flags", "masks"),
      {"points": A(False, lambda s: 32, 16), "dirs": A(False, lambda s: 16 * s["n_dirs"], 16, fixed=True), "masks": A(True, lambda s: 8, 8)},
      {"n_dirs": 4, "flags": 0},
      [({"n_dirs": 0}, "n_dirs = 0 (1 to 64)"), ({"n_dirs": MAX_DIRS + 1}, "n_dirs = 65 (1 to 64)"), ({"flags": 0x80000000}, "unknown flags 0x80000000")],
      "points and dirs must be 16-byte aligned, masks 8-byte aligned"),
    Q("rt_tracer_intersect_all", ("segs", "n", "max_hits", "hits", "counts"),
      {"segs": A(False, lambda s: 32, 16), "hits": A(True, _rows(16), 16), "counts": A(True, lambda s: 4, 4)},
      {"max_hits": 4}, ROW_CHECKS, "segs and hits must be 16-byte aligned, counts 4-byte aligned"),
    Q("rt_tracer_closest_point", ("pts", "n", "out"), {"pts": A(False, lambda s: 16, 16), "out": A(True, lambda s: 16, 16)},
      {}, [], "pts and out must be 16-byte aligned"),
    Q("rt_tracer_closest_all", ("pts", "after", "n", "max_hits", "hits", "counts"),
      {"pts": A(False, lambda s: 16, 16), "after": A(False, lambda s: 16, 16, lambda s: True), "hits": A(True, _rows(16), 16),
       "counts": A(True, lambda s: 4, 4)},
      {"max_hits": 4}, ROW_CHECKS, "pts, after and hits must be 16-byte aligned, counts 4-byte aligned"),
    Q("rt_tracer_signed_distance", ("pts", "n", "hits", "sides"),
      {"pts": A(False, lambda s: 16, 16), "hits": A(True, lambda s: 16, 16), "sides": A(True, lambda s: 8, 8)},
      {}, [], "pts and hits must be 16-byte aligned, sides 8-byte aligned"),
    Q("rt_tracer_closest_sides", ("pts", "records", "n", "per_point", "sides"),
      {"pts": A(False, lambda s: 16, 16), "records": A(False, lambda s: 16 * s["per_point"], 16), "sides": A(True, lambda s: 8 * s["per_point"], 8)},
      {"per_point": 2}, [({"per_point": 0}, "per_point = 0 (1 to 16)"), ({"per_point": MAX_HITS + 1}, "per_point = 17 (1 to 16)")],
      "pts and hits must be 16-byte aligned, sides 8-byte aligned"),
    _region("rt_tracer_overlap", "boxes", 8),
    _region("rt_tracer_overlap_triangles", "tris", 12),
    _region("rt_tracer_overlap_hexahedra", "hexa", 32),
    Q("rt_tracer_sphere_cast", ("sweeps", "n", "hits"), {"sweeps": A(False, lambda s: 32, 16), "hits": A(True, lambda s: 16, 16)},
      {}, [], "sweeps and hits must be 16-byte aligned"),
    Q("rt_tracer_triangle_distance", ("tris", "n", "hits", "witness"),
      {"tris": A(False, lambda s: 48, 16), "hits": A(True, lambda s: 16, 16), "witness": A(True, lambda s: 16, 16)},
      {}, [], "tris, hits and witness must be 16-byte aligned"),
]
PICK = Q("rt_tracer_pick", ("pixels", "n", "hits", "rays"),
         {"pixels": A(False, lambda s: 8, 1), "hits": A(True, lambda s: 16, 1), "rays": A(True, lambda s: 24, 1, lambda s: True)}, {}, [], None)
# (pair, _device form?): the 27 entry points
ROWS = [(q, dev) for q in PAIRS for dev in (False, True)] + [(PICK, False)]
IDS = [q.name + ("_device" if dev else "") for q, dev in ROWS]


def test_the_table_has_a_row_for_each_of_the_27_entry_points():
    import raytracertest_amd as R
    L = R.api.load_library()
    assert len(ROWS) == 27 and len(set(IDS)) == 27
    for name in IDS:
        assert hasattr(L, name), name


def _inputs():
    """The 8 queries of every input array, as float32 / uint32 / int32 rows (the records of rt_tracer_closest_sides are made
    by the tracer: _state)."""
    rng = np.random.default_rng(27)
    f32, inf = np.float32, np.float32(np.inf)
    z = np.zeros((N, 1), f32)
    o = rng.uniform(-0.5, 0.5, (N, 3)).astype(f32)
    d = np.c_[rng.uniform(-0.3, 0.3, (N, 2)), -np.ones(N)].astype(f32)
    c = np.c_[rng.uniform(-1.2, 1.2, (N, 2)), rng.uniform(-3.5, -2.5, N)].astype(f32)     # about the quad at z = -3
    half = rng.uniform(0.1, 0.6, (N, 3)).astype(f32)
    tris = np.zeros((N, 3, 4), f32)
    tris[:, :, :3] = c[:, None, :] + rng.uniform(-0.6, 0.6, (N, 3, 3)).astype(f32)
    near = tris.copy()
    near[:, 0, 3] = inf                                                  # rt_tracer_triangle_distance: no search radius
    hexa = np.zeros((N, 8, 4), f32)
    hexa[:, :, :3] = he.aligned_boxes(c, 5, 2.0)
    dirs = np.array([[0, 0, 1, 0], [0.6, 0, 0.8, 0], [0, 0.6, 0.8, 0], [-0.6, 0, 0.8, 0]], f32)
    surface = np.c_[c[:, :2], np.full(N, -3.0), np.zeros((N, 2)), np.ones(N), np.full(N, 1e-3), np.full(N, inf)].astype(f32)
    return {"rays": np.c_[o, d], "segs": np.c_[o, d, z, z + inf], "points": surface, "dirs": dirs, "pts": np.c_[c, z + inf],
            "boxes": np.c_[c - half, z, c + half, z], "tris": tris, "near_tris": near, "hexa": hexa,
            "sweeps": np.c_[o, d, z + f32(0.1), z + inf], "pixels": np.array([[8 * i + 3, 5 * i + 2] for i in range(N)], np.uint32)}


@pytest.fixture(scope="module")
def state():
    """(library, tracer, input bytes by array name): the quad (-1.5, -1.5, -3) .. (1.5, 1.5, -3) as two triangles."""
    import raytracertest_amd as R
    L = R.api.load_library()
    g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1)
    quad = np.zeros((6, 4), np.float32)
    quad[:, :3] = [[-1.5, -1.5, -3], [1.5, -1.5, -3], [1.5, 1.5, -3], [-1.5, -1.5, -3], [1.5, 1.5, -3], [-1.5, 1.5, -3]]
    assert g.UploadScene(quad)
    data = {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in _inputs().items()}
    records, counts = np.zeros(N * 2 * 16, np.uint8), np.zeros(N, np.uint32)   # both triangles of every point, nearest first
    assert L.rt_tracer_closest_all(g._h, data["pts"].ctypes.data, None, N, 2, records.ctypes.data, counts.ctypes.data) == 0
    assert (counts == 2).all()
    data["records"] = records
    data["after"] = np.full(N * 16, 0xFF, np.uint8)                      # prim -1 in an rt_hit's last word, and -1 as int32: no cursor
    yield L, g, data
    g.close()


def _scalars(q, n, over=None):
    return dict(q.scalars, n=n, **(over or {}))


def _bytes(q, name, s, n=N):
    a = q.arrays[name]
    return a.bytes(s) * (1 if a.fixed else n)


def _source(q, name, data):
    return data["near_tris" if (q.name, name) == ("rt_tracer_triangle_distance", "tris") else name]


class Buffers:
    """The arrays of one call of q with scalars s, on the host (numpy) or the device (torch), each one row longer than the call
    reads or writes: the inputs hold data's bytes, the outputs SENTINEL."""

    def __init__(self, q, dev, s, data):
        import torch
        self.q, self.dev, self.arr = q, dev, {}
        for name, a in q.arrays.items():
            used = _bytes(q, name, s)
            host = np.full(used + max(a.bytes(s), a.align, 16), SENTINEL, np.uint8)
            if not a.out:
                src = _source(q, name, data)
                assert src.size >= used, name
                host[:used] = src[:used]
            self.arr[name] = torch.from_numpy(host).to("cuda:0") if dev else host

    def ptr(self, name):
        x = self.arr[name]
        return x.data_ptr() if self.dev else x.ctypes.data

    def outputs(self):
        import torch
        if self.dev:
            torch.cuda.synchronize()
        return {k: (x.cpu().numpy() if self.dev else x).copy() for k, x in self.arr.items() if self.q.arrays[k].out}

    def untouched(self):
        return all((x == SENTINEL).all() for x in self.outputs().values())


def _call(L, g, q, dev, s, ptrs):
    """-> (return code, the tracer's error text); ptrs: a pointer or None per array name."""
    args = [s[a] if a in s else ptrs[a] for a in q.args]
    rc = getattr(L, q.name + ("_device" if dev else ""))(g._h, *args, *([None] if dev else []))
    return rc, g.LastError()


def _pointers(q, b, s, null=(), moved=None):
    """Every array's pointer; the optional ones of `null` as None; `moved` off its alignment: 4 bytes off a demand of 16 or 8,
    an odd address for one of 4."""
    p = {name: None if name in null else b.ptr(name) for name in q.arrays}
    if moved:
        p[moved] += 4 if q.arrays[moved].align > 4 else 1
    return p


def _required(q, s):
    return [name for name, a in q.arrays.items() if not a.optional(s)]


@pytest.mark.parametrize("q,dev", ROWS, ids=IDS)
def test_refusals_leave_the_outputs_alone_and_well_formed_calls_are_accepted(state, q, dev):
    L, g, data = state
    who = q.name + ("_device" if dev else "")
    s = _scalars(q, N)
    b = Buffers(q, dev, s, data)
    assert b.untouched()
    for name in _required(q, s):                                         # each required array, null
        ptrs = dict(_pointers(q, b, s), **{name: None})
        assert _call(L, g, q, dev, s, ptrs) == (1, NULL_ARRAY), (who, name)
    for over, text in q.checks:                                          # the query's own check: its text, and before the null-array check
        bad = _scalars(q, N, over)
        for null in ([], _required(q, s)[:1]):
            ptrs = dict(_pointers(q, b, s), **{k: None for k in null})
            assert _call(L, g, q, dev, bad, ptrs) == (1, "%s: %s" % (who, text)), (who, over, null)
    nothing = {name: None for name in q.arrays}
    assert _call(L, g, q, dev, _scalars(q, 0), nothing)[0] == 0, who      # n = 0: nothing is looked at
    if dev:
        aligned = [name for name, a in q.arrays.items() if a.align > 1]
        off = _pointers(q, b, s)
        for name in aligned:
            off[name] += 4 if q.arrays[name].align > 4 else 1
        assert _call(L, g, q, dev, _scalars(q, 0), off)[0] == 0, who
        for name in aligned:                                             # each pointer in turn off its alignment: the full text
            assert _call(L, g, q, dev, s, _pointers(q, b, s, moved=name)) == (1, "%s: %s" % (who, q.misaligned)), (who, name)
    if q is PICK:                                                        # its check between the lock and the launch: a pixel outside the image
        outside = Buffers(q, dev, s, dict(data, pixels=np.array([[3, 2]] * (N - 1) + [[64, 2]], np.uint32).view(np.uint8).reshape(-1)))
        assert _call(L, g, q, dev, s, _pointers(q, outside, s)) == (1, "Pick: pixel (64, 2) is outside the 64 x 48 image")
        assert outside.untouched()
    assert b.untouched(), who                                            # no refusal wrote anything
    optional = [name for name, a in q.arrays.items() if a.optional(s)]
    assert _call(L, g, q, dev, s, _pointers(q, b, s, null=optional))[0] == 0, (who, g.LastError())
    assert not b.untouched()
    if "max_hits" in s and q.checks is REGION_CHECKS:                    # counts only: prims may be null, and is not written when given
        s0 = _scalars(q, N, {"max_hits": 0})
        for null in (("after", "prims"), ("after",)):
            b0 = Buffers(q, dev, s0, data)
            assert _call(L, g, q, dev, s0, _pointers(q, b0, s0, null=null))[0] == 0, (who, null, g.LastError())
            out = b0.outputs()
            assert (out["prims"] == SENTINEL).all() and not (out["counts"][:4 * N] == SENTINEL).all(), (who, null)


def _variants(q):
    """The well-formed calls of a pair: (scalars, optional arrays left out)."""
    s = _scalars(q, N)
    optional = tuple(name for name, a in q.arrays.items() if a.optional(s))
    out = [(s, ())] + ([(s, optional)] if optional else [])
    if q.checks is REGION_CHECKS:
        out.append((_scalars(q, N, {"max_hits": 0}), ("after", "prims")))
    return out


def _accepted(L, g, q, dev, s, null, data):
    """The outputs of one well-formed call: written where an array was given, and nothing past the call's bytes."""
    b = Buffers(q, dev, s, data)
    assert _call(L, g, q, dev, s, _pointers(q, b, s, null=null))[0] == 0, (q.name, dev, null, g.LastError())
    out = b.outputs()
    for name, x in out.items():
        used = 0 if name in null else _bytes(q, name, s)
        assert (x[used:] == SENTINEL).all() and (used == 0 or name == "prims" or not (x[:used] == SENTINEL).all()), (q.name, dev, name)
    return out


@pytest.mark.parametrize("q", PAIRS, ids=[q.name for q in PAIRS])
def test_both_forms_of_a_pair_give_the_same_bytes(state, q):
    L, g, data = state
    for s, null in _variants(q):
        host, device = (_accepted(L, g, q, dev, s, null, data) for dev in (False, True))
        for name in host:
            assert host[name].tobytes() == device[name].tobytes(), (q.name, name, null)


def test_pick_gives_the_same_hits_with_and_without_the_rays(state):
    L, g, data = state
    s = _scalars(PICK, N)
    with_rays, without = (_accepted(L, g, PICK, False, s, null, data) for null in ((), ("rays",)))
    assert with_rays["hits"].tobytes() == without["hits"].tobytes()
