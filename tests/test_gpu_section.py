"""The section queries on the device (RayTracer.Section / SectionAll / SectionSegments / Slice): the scan and the BVH walk against
the numpy restatement of section_expect, rows and counts exactly, for both upload layouts, both arithmetic modes (which must not
change a byte), with and without spheres, max_hits on both sides of the list-capacity switches and the continuation cursor; the
batch and chunk seams with invalid planes in every wave and one wave of nothing else; the walk against the scan byte for byte on
the lattice with planes in the walls, with any slack, a shortened stack, a refitted tree and non-finite records; the cut records
bit for bit; an axis-aligned slab against Overlap, a cut against IntersectAll; a running Trace left alone, the other queries in
between, the _device forms, the torch path, multi-device forwarding, n = 0 and argument errors."""
import functools
import hashlib

import numpy as np
import pytest

import lattice_cases as lc
import overlap_expect as oe
import section_expect as se
from query_accel_expect import conditioning
from query_expect import edge_rows
from test_gpu_overlap import COUNTS, SPHERES, _assert_rows, _tracer, assert_block_edges
from test_section_expect import _bad_records, lattice_planes

pytestmark = pytest.mark.gpu

f32 = np.float32
KS = (0, 1, 4, 5, 16)                                                    # 0: no list; 4 | 5: the list of 4 slots gives way to the one of 16


@pytest.fixture(scope="module", autouse=True)
def library_has_the_query():
    """The populations below are the query's: without rt_tracer_section there is nothing to aim them at."""
    from raytracertest_amd import api
    assert hasattr(api.load_library(), "rt_tracer_section") and hasattr(api.RayTracer, "SectionSegments")


def _assert_cuts(got, exp, label):
    """Bit for bit, a NaN for a NaN (0 / 0 of a zero normal has no prescribed payload)."""
    assert got.dtype == se.CUT_DTYPE and got.shape == exp.shape, label
    for name in ("kind", "features"):
        assert np.array_equal(got[name], exp[name]), (label, name, np.nonzero(got[name] != exp[name])[0][:5])
    for name in ("p0", "p1"):
        a, b = got[name], exp[name]
        ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        bad = np.nonzero(~ok.all(axis=-1))
        assert ok.all(), (label, name, [x[:3] for x in bad], a[bad][:3], b[bad][:3])


def mixed_planes(rows, n, seed):
    """Planes and thin and thick slabs through the scene, half-spaces, a slab that holds everything, n = 0, and -- in every run of
    sixteen -- an invalid plane; NaNs in the pads of every third."""
    planes = np.concatenate([se.random_planes(rows, n - n // 2, seed), se.random_planes(rows, n // 4, seed + 1, thick=0.02),
                             se.random_planes(rows, n // 2 - n // 4, seed + 2, thick=0.5)])
    planes = planes[np.random.default_rng(seed + 3).permutation(n)]
    planes[5] = se.planes_of((0.3, -1, 0.2), -se.INF, se.INF)[0]
    planes[6] = se.planes_of((0, 0, 0), -1.0, 1.0)[0]
    planes[8], planes[9] = se.planes_of((1, 1, 1), [-se.INF, 0.5], [0.25, se.INF])
    bad = se.bad_planes(planes[0])
    planes[7::16] = bad[np.arange(len(planes[7::16])) % len(bad)]
    planes[2::3] = se.nan_pads(planes[2::3])
    return planes


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, the mixed planes and the verdict table with SPHERES' columns: one table for all."""
    rows = se.random_scene(n_tris, seed=300 + n_tris, span=3.0, edge=0.6)
    planes = mixed_planes(rows, 257 if n_tris >= 1000 else 300, 400 + n_tris)
    planes[:4] = se.planes_of([(0, 0, 1), (0, 0, 1), (2, 0, 0), (0, 1, 0)], [-1.0, -1.85, 1.0, -29.0], [-1.0, -1.75, 2.6, -29.0])
    acc = se.table(planes, rows, spheres=SPHERES)
    for x in (rows, planes, acc):
        x.setflags(write=False)
    return rows, planes, acc


def test_the_populations_reach_what_they_are_for():
    _, planes, acc = _reference(1100)
    counts = acc[:, :1100].sum(axis=1)
    assert (counts == 0).any() and (counts > 4).any() and (counts > 16).any() and counts[5] == 1100
    small = _reference(37)[2][:, :37].sum(axis=1)
    assert all((small == c).any() for c in range(6))
    # the twin spheres' centre plane, a slab about their rim, a slab across them, the far one's tangent plane
    assert acc[0, 1100] and acc[0, 1101] and acc[1, 1100] and acc[2, 1100] and not acc[2, 1102] and acc[3, 1102] and not acc[3, 1100]
    assert np.array_equal(acc[:, 1100], acc[:, 1101])
    assert not se.valid(planes).all() and np.isnan(planes[:, 5:]).any() and not acc[~se.valid(planes)].any()


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_max_hits_and_count(n_tris, spheres):
    rows, planes, acc = _reference(n_tris)
    acc = acc if spheres else acc[:, :n_tris]
    exp = {k: se.rows_of_table(acc, k) for k in KS}
    cursor = exp[4][0][:, 3].copy()                                      # a row's last prim where it is full, else none
    exp_after = {k: se.rows_of_table(acc, k, after=cursor) for k in (1, 16)}
    digests = {}
    for edges in (False, True):
        if edges:                                                        # the edge layout's records are the uploaded rows themselves
            assert np.array_equal(se.table(planes, edge_rows(rows), edges=True, spheres=SPHERES if spheres else None), acc)
        for mm in (0, 1):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            if spheres:
                g.UploadSpheres(SPHERES)
            blob = hashlib.sha256()
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in KS:
                    label = "n_tris=%d spheres=%d edges=%d mm=%d accel=%d k=%d" % (n_tris, spheres, edges, mm, accel, k)
                    got = g.Section(planes, k)
                    _assert_rows(got, exp[k], label)
                    blob.update(got[0].tobytes())
                    blob.update(got[1].tobytes())
                    for n in COUNTS:
                        _assert_rows(g.Section(planes[:n], k), (exp[k][0][:n], exp[k][1][:n]), label + " n=%d" % n)
                for k in (1, 16):
                    _assert_rows(g.Section(planes, k, after=cursor), exp_after[k], "cursor accel=%d k=%d" % (accel, k))
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


def test_batch_and_chunk_seams_with_invalid_planes_in_every_wave_and_one_wave_of_nothing_else():
    rows = se.random_scene(1025, seed=81, span=3.0, edge=0.6)            # one triangle past a chunk, one sphere
    planes = mixed_planes(rows, 257, 82)                                 # a block and one; [:65]: a wave and one
    far = se.planes_of((0, 0, 1), [50.0, -50.0], [60.0, -49.0])
    planes[20], planes[200] = far
    bad = se.bad_planes(planes[0])
    planes[128:192] = bad[np.arange(64) % len(bad)]                      # the third wave holds invalid planes only: the idle-wave skip
    ok = se.valid(planes)
    assert not ok[128:192].any() and all((~ok[w:w + 64]).any() and (ok[w:w + 64].any() or w == 128) for w in (0, 64, 128, 192)) and ok[256]
    acc = se.table(planes, rows, spheres=SPHERES[:1])
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES[:1])
    assert_block_edges(g, g.Section, planes, acc, se.rows_of_table)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        _assert_rows(g.Section(planes, 16), se.rows_of_table(acc, 16), "257 planes accel=%d" % accel)
        _assert_rows(g.Section(planes[128:192], 4), se.rows_of_table(acc[128:192], 4), "the idle wave alone accel=%d" % accel)
        assert g.Section(planes[5:6], 16)[1][0] == 1026                  # the last record of the second chunk and the sphere counted
        last = g.Section(planes[5:6], 16, after=np.int32([1009]))
        assert last[1][0] == 16 and last[0][0].tolist() == list(range(1010, 1026))
    g.close()


def test_section_all_enumerates_once_and_the_cursor_edges():
    rows = np.zeros((111, 4), f32)
    rows[0::3, :3], rows[1::3, :3], rows[2::3, :3] = [-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]          # 37 coincident triangles
    spheres = f32([[0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.5, 0.5], [0.0, -0.25, 2.0, 0.25]])
    planes = np.concatenate([se.planes_of((0, 1, 0), [-0.25]), se.random_planes(rows, 30, 5, thick=0.2)])
    acc = se.table(planes, rows, spheres=spheres)
    assert acc[0].all() and acc.shape[1] == 40
    sets = oe.accepted_sets(acc)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(spheres)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 5, 1):
            prims, offsets = g.SectionAll(planes if k > 1 else planes[:1], k)
            assert prims.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == prims.shape[0]
            assert np.array_equal(prims[offsets[0]:offsets[1]], np.arange(40))      # 0 .. 39, once each, in order
            for i in range(offsets.shape[0] - 1):
                assert np.array_equal(prims[offsets[i]:offsets[i + 1]], sets[i])
        for after, count in ((39, 0), (-1, 40), (5000, 0), (2 ** 31 - 1, 0), (38, 1), (0, 39), (-2, 40), (-2 ** 31, 40)):
            p, c = g.Section(planes[:1], 4, after=np.int32([after]))
            assert c[0] == count, (after, c)
            first = max(after + 1, 0) if after != -1 else 0
            assert p[0].tolist() == [first + s if s < count else -1 for s in range(4)], (after, p)
    g.close()


def test_bvh_equals_scan_byte_for_byte_on_the_lattice_whatever_the_slack():
    rows = lc.rooms()
    planes = np.concatenate([lattice_planes(), mixed_planes(rows, 2048, 11)])
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.Section(planes, k) for k in (0, 4, 16)}
    assert (scan[16][1] == 0).any() and (scan[16][1] > 16).any()
    _assert_rows(tuple(x[:300] for x in scan[16]), se.expected(planes[:300], rows, 16), "the scan against the helper")
    g.SetQueryAcceleration(True)
    for slack in (1000, 0):
        g.DebugQueryAccelSlack(slack)
        for k in (0, 4, 16):
            got = g.Section(planes, k)
            assert got[0].tobytes() == scan[k][0].tobytes() and got[1].tobytes() == scan[k][1].tobytes(), (slack, k)
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_a_shortened_stack_restarts_list_and_count():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    s = dc.scales()
    rng = np.random.default_rng(3)
    pick = rng.integers(0, 70, 180)
    planes = np.concatenate([se.planes_of((0, 0, 1), -se.INF, se.INF), se.planes_of((1, 2, -1), -se.INF, se.INF),
                             se.planes_of((1.0, 0.0, 5.0), 26.0 * s[pick] * rng.uniform(0.98, 1.02, 180)),
                             se.planes_of((0, 0, -1), -5.2 * s[pick[:74]], -4.8 * s[pick[:74]])])
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.Section(planes, k) for k in (0, 3, 16)}
    total = scan[0][1]
    assert (total > 16).any() and (total < 16).any() and total[0] == rows.shape[0] // 3
    _assert_rows(tuple(x[:64] for x in scan[16]), se.expected(planes[:64], rows, 16), "deep scan against the helper")
    g.SetQueryAcceleration(True)
    g.Section(planes[:1], 0)                                             # builds the tree
    depth = g.QueryAccelInfo()["depth"]
    assert depth == dc.DEPTH_BOUND
    try:
        for cap in (None, 3 * depth, 3 * depth - 1, 0):
            g.DebugQueryStackCap(cap)
            for k in scan:
                _assert_rows(g.Section(planes, k), scan[k], "deep cap=%r k=%d" % (cap, k))
            cursor = scan[3][0][:, 2].copy()
            g.SetQueryAcceleration(False)
            want = g.Section(planes, 16, after=cursor)
            g.SetQueryAcceleration(True)
            _assert_rows(g.Section(planes, 16, after=cursor), want, "deep cap=%r cursor" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                    # (inf - inf and overflow are what the scene is made of)
def test_non_finite_records_a_refitted_tree_empty_scenes_spheres_alone_and_n_0():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = _bad_records(se.random_scene(1100, 21, span=3.0, edge=0.6))   # three records in the always-tested list
    planes = mixed_planes(rows, 300, 9)
    for edges in (False, True):
        r = edge_rows(rows) if edges else rows
        acc = se.table(planes, r, edges=edges, spheres=SPHERES)
        g = _tracer()
        assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
        g.UploadSpheres(SPHERES)
        for accel in (False, True):
            g.SetQueryAcceleration(accel)
            for k in (0, 4, 16):
                _assert_rows(g.Section(planes, k), se.rows_of_table(acc, k), "non-finite edges=%d accel=%d k=%d" % (edges, accel, k))
        assert g.QueryAccelInfo()["always_tested"] >= 2 and not acc[:, 5].any()
        g.close()
    base = rc.scenes()["adversarial1100"]
    moved = rc.jitter(base, 5)
    planes = mixed_planes(moved, 2048, 10)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(base)
    first = g.Section(planes, 16)
    assert g.UploadScene(moved)
    got = {k: g.Section(planes, k) for k in (16, 4, 0)}                  # the first of them refits
    u = g.QueryAccelUpdateInfo()
    assert u["refits"] == 1 and u["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    for k in (16, 4, 0):
        _assert_rows(got[k], g.Section(planes, k), "after the refit k=%d" % k)
    assert (first[0] != got[16][0]).any()                                # the scene did move
    _assert_rows(tuple(x[:128] for x in got[16]), se.expected(planes[:128], moved, 16), "the moved scene against the helper")
    g.close()
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        prims, counts = g.Section(planes[:300], 5)                       # no scene: nothing to cut
        assert prims.shape == (300, 5) and not counts.any() and (prims == -1).all()
        cuts = g.SectionSegments(planes[:300], prims)
        assert cuts.shape == (300, 5) and not cuts.view(np.uint8).any()
        prims, counts = g.Section(np.zeros((0, 8), f32), 3)              # n = 0
        assert prims.shape == (0, 3) and counts.shape == (0,) and g.SectionSegments(np.zeros((0, 8), f32), prims).shape == (0, 3)
        assert g.SectionAll(np.zeros((0, 8), f32))[1].tolist() == [0] and g.Slice((0, 0, 1), [])[1].tolist() == [0]
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        q = np.concatenate([_reference(37)[1][:4], planes[:100]])
        acc = se.table(q, None, spheres=SPHERES)
        assert acc[0, :2].all() and acc[3, 2]
        for k in KS:
            _assert_rows(g.Section(q, k), se.rows_of_table(acc, k), "spheres only accel=%d k=%d" % (accel, k))
        g.close()


# ---- the cut ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edges", [False, True])
def test_section_segments_are_the_restated_records_bit_for_bit(edges):
    rows, planes, acc = _reference(1100)
    r = edge_rows(rows) if edges else rows
    zero = se.planes_of((0, 0, 0), 0.0)[0]
    g = _tracer(1 if edges else 0)
    assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
    g.UploadSpheres(SPHERES)
    seen = set()
    for k in (1, 4, 16):
        q = np.array(planes)
        q[11] = zero                                                     # n = 0, d = 0: every corner is on the plane, every sphere 0 / 0
        prims = g.Section(q, k)[0].copy()
        assert (prims == -1).any() and (prims >= 1100).any()             # RT_PRIM_NONE padding and sphere prims are among them
        prims[12, -1], prims[13, 0], prims[14, -1], prims[15, 0] = 1103, 5000, -7, 2 ** 31 - 1      # beyond the scene
        prims[11, -1] = 1100                                             # a sphere against n = 0: a circle whose centre is 0 / 0
        for side in (0, 1):
            got = g.SectionSegments(q, prims if k > 1 else prims[:, 0], side)
            want = se.cuts(q, prims if k > 1 else prims[:, 0], r, edges=edges, spheres=SPHERES, side=side)
            _assert_cuts(got, want, "edges=%d k=%d side=%d" % (edges, k, side))
            seen |= set(np.unique(got["kind"]).tolist())
            flat = got.reshape(-1) if k > 1 else got
            assert not flat[(prims.reshape(-1) if k > 1 else prims[:, 0]) == -1].view(np.uint8).any()
    assert seen >= {se.CUT_NONE, se.CUT_SEGMENT, se.CUT_COPLANAR, se.CUT_CIRCLE}
    # a block and one: 257 records, and the kinds a random scene does not hold
    cube = se.cube()
    assert g.UploadScene(cube)
    pl = se.planes_of([(0, 0, 1)] * 3 + [(1, 1, 1)], [2.0, 1.0, 0.0, 0.0])
    q = np.tile(pl, (65, 1))[:257]
    prims = ((np.arange(257) // 4) % 12).astype(np.int32)             # every plane against every triangle
    got = g.SectionSegments(q, prims)
    _assert_cuts(got, se.cuts(q, prims, cube, spheres=SPHERES), "257 records on the cube")
    assert set(np.unique(got["kind"]).tolist()) == {se.CUT_NONE, se.CUT_SEGMENT, se.CUT_TOUCH, se.CUT_COPLANAR}
    g.close()


def test_the_cube_loop_comes_out_closed_and_counter_clockwise_and_slice_is_the_restated_slice():
    cube = se.cube()
    g = _tracer()
    assert g.UploadScene(cube)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for normal, d in (((0, 0, 1), 1.0), ((0, 0, -1), -1.0), ((0, 2, 0), 2.0)):
            cuts, off = g.Slice(normal, [d])
            assert cuts.shape[0] == 8 and off.tolist() == [0, 8]
            loop = se.loops(cuts)
            assert loop is not None and len(loop) == 1 and len(loop[0]) == 8
            assert se.loop_area(cuts, loop[0], normal) == 4.0            # counter-clockwise from the tip of n
        offsets = [0.5, 1.0, 1.5, 3.0, 2.0, 0.0]
        cuts, off = g.Slice((0, 0, 1), offsets)
        want, woff = se.slice_expected((0, 0, 1), offsets, cube)
        assert off.tolist() == woff.tolist() == [0, 8, 16, 24, 24, 24, 24]
        _assert_cuts(cuts, want, "Slice accel=%d" % accel)
    rows, _, _ = _reference(1100)
    assert g.UploadScene(rows)
    cuts, off = g.Slice((0.2, -0.1, 1.0), np.linspace(-3, 3, 33))
    want, woff = se.slice_expected((0.2, -0.1, 1.0), np.linspace(-3, 3, 33), rows)
    assert off.tolist() == woff.tolist() and off[-1] > 500
    _assert_cuts(cuts, want, "Slice of the random scene")
    g.close()


# ---- against the existing queries ----------------------------------------------------------------------------------------------

def test_an_axis_aligned_slab_on_the_eighth_lattice_answers_as_an_unbounded_box():
    rows = np.clip(oe.random_scene(400, 5, edge=1.0, span=1.5, snap=0.125), -2, 2)
    rng = np.random.default_rng(6)
    z0 = np.round(rng.uniform(-2, 1.5, 600) * 8) / 8
    z1 = np.minimum(z0 + np.round(rng.uniform(0, 1.0, 600) * 8) / 8, 2.0)
    planes = se.planes_of((0, 0, 1), z0, z1)
    boxes = np.repeat(oe.unbounded_boxes(np.zeros(8, f32))[:1], 600, axis=0)          # all of space ...
    boxes[:, 2], boxes[:, 6] = z0, z1                                    # ... between two heights
    g = _tracer()
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (0, 4, 16):
            want = g.Overlap(boxes, k)
            assert want[1].sum() > 5000 and (z0 == z1).sum() > 10
            _assert_rows(g.Section(planes, k), want, "lattice accel=%d k=%d" % (accel, k))
    g.close()


def test_a_cut_against_intersect_all():
    """Coarse.  The issue's form -- Occluded ALONG the segment lengthened by 2^-10 of its length at both ends, only for records
    that are well conditioned as the BVH contract defines it (|det| / (|d| |e1| |e2|) >= 2^-10) -- is kept as stated; a ray along
    a record's own cut lies in the record's plane, its conditioning is rounding noise (at most 7.1e-4 here), and the clause lets
    none of the 3 387 records through: that count is asserted, so (i) is known to cover nothing.  What does test the cut: a ray THROUGH the segment's midpoint along the record's normal, both ways
    (the ray queries cull back faces), finds the record at the midpoint."""
    rows, _, _ = _reference(1100)
    planes = se.random_planes(rows, 64, 71)
    g = _tracer()
    assert g.UploadScene(rows)
    prims, off = g.SectionAll(planes)
    owner = np.repeat(np.arange(64), np.diff(off))
    cuts = g.SectionSegments(planes[owner], prims)
    seg = cuts["kind"] == se.CUT_SEGMENT
    cuts, prims = cuts[seg], prims[seg]
    assert cuts.shape[0] > 2000
    p0, p1 = cuts["p0"].astype(np.float64), cuts["p1"].astype(np.float64)
    length = np.linalg.norm(p1 - p0, axis=1)
    # (i) along the segment
    o, d = p0 - 2.0 ** -10 * (p1 - p0), (1 + 2.0 ** -9) * (p1 - p0)
    rays = np.c_[o, d].astype(f32)
    with np.errstate(all="ignore"):
        well = np.abs(conditioning(rays, rows, prims)) >= 2.0 ** -10
    found = np.zeros(len(prims), bool)
    for sign in (1, -1):
        r = rays.copy()
        if sign < 0:
            r[:, :3], r[:, 3:] = rays[:, :3] + rays[:, 3:], -rays[:, 3:]
        hits, counts = g.IntersectAll(np.c_[r, np.zeros(len(r), f32), np.ones(len(r), f32)].astype(f32), 16)
        found |= ((hits["prim"] == prims[:, None]) & (np.arange(16)[None, :] < counts[:, None])).any(axis=1)
    print("along the segment: %d of %d records are well conditioned, %d of those found, %d found in all" % (well.sum(), len(prims), (found & well).sum(), found.sum()))
    assert found[well].all()
    assert well.sum() == 0                                               # the clause admits NONE of these (largest conditioning 7.1e-4 < 2^-10): (ii) is the test
    # (ii) through the midpoint
    A, B, C = (x[prims].astype(np.float64) for x in se.corners(rows))
    nrm = np.cross(B - A, C - A)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mid, h = (p0 + p1) / 2, 0.05
    inside = length > 0.02                                               # (a midpoint well inside the record, off its edges)
    got = np.zeros(len(prims), bool)
    for sign in (1, -1):
        r = np.c_[mid - sign * h * nrm, sign * nrm].astype(f32)
        hits, counts = g.IntersectAll(np.c_[r, np.zeros(len(r), f32), np.full(len(r), 2 * h, f32)].astype(f32), 16)
        mine = (hits["prim"] == prims[:, None]) & (np.arange(16)[None, :] < counts[:, None])
        got |= (mine & (np.abs(hits["t"] - h) < 1e-4)).any(axis=1)
    assert inside.sum() > 2000 and got[inside].all(), np.nonzero(inside & ~got)[0][:5]
    g.close()


# ---- around the call --------------------------------------------------------------------------------------------------------------

def test_section_between_the_other_queries_on_one_tracer_and_a_running_trace_left_alone():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    planes = mixed_planes(rows, 2048, 7)
    rng = np.random.default_rng(8)
    rays = np.c_[rng.uniform(-0.05, 0.05, (300, 3)), rng.uniform(-0.6, 0.6, (300, 2)), -np.ones(300)].astype(f32)
    pts = rng.uniform(-1, 1, (300, 3)).astype(f32)
    boxes = oe.random_boxes(rows, 300, 9)

    def run(calls, trace=True):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Section(planes, 16)
        idle_cuts = g.SectionSegments(planes, idle[0])
        others = (g.Intersect(rays), g.ClosestPoint(pts), g.Overlap(boxes, 4))
        got = []
        if trace:
            g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            n = (2048, 70, 5, 300)[i % 4]                                # a smaller batch behind a larger one: the staging buffers hold other bytes
            k = 16 if i % 4 < 2 else 4
            between = (g.Intersect(rays[:n]), g.ClosestPoint(pts[:n]), g.Overlap(boxes[:n], 4))[i % 3]
            sec = g.Section(planes[:n], k)
            got.append((n, k, sec, g.SectionSegments(planes[:n], sec[0], side=i % 2), between, i))
        if trace:
            assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, idle_cuts, others, got, out

    idle, idle_cuts, others, got, out = run(8)
    assert len(got) == 8 and idle[1].any()
    _assert_rows(tuple(x[:64] for x in idle), se.expected(planes[:64], rows, 16), "the idle answer against the helper")
    for n, k, (p, c), cuts, between, i in got:
        assert np.array_equal(p, idle[0][:n, :k]) and np.array_equal(c, idle[1][:n])
        _assert_cuts(cuts, se.cuts(planes[:n], p, rows, side=i % 2), "cuts of call %d" % i)
        want = others[i % 3]
        if i % 3 == 2:
            assert np.array_equal(between[0], want[0][:n]) and np.array_equal(between[1], want[1][:n])
        elif i % 2 == 0:                                                 # (the scan: the ray and point walks have their own contract with it)
            assert between.tobytes() == want[:n].tobytes()
    _assert_cuts(idle_cuts, se.cuts(planes, idle[0], rows), "the idle cuts")
    ref = run(0)[4]
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_torch_path_device_forms_on_a_side_stream_and_argument_errors():
    import torch
    import raytracertest_amd as R
    rows, planes, acc = _reference(1100)
    n = planes.shape[0]
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(planes)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 4, 0):
            want = se.rows_of_table(acc, k)
            tp, tc = g.Section(t, k)
            assert tp.dtype == torch.int32 and tp.shape == (n, k) and tc.dtype == torch.int32 and tc.shape == (n,)
            assert tp.cpu().numpy().tobytes() == want[0].tobytes() and tc.cpu().numpy().tobytes() == want[1].tobytes()
            if k:
                after = tp[:, k - 1].contiguous()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):                               # on the caller's current stream
                    tp2, tc2 = g.Section(t, k)
                    np_, nc = g.Section(t, k, after=after)
                    tcuts = g.SectionSegments(t, tp2, side=1)
                    tcuts1 = g.SectionSegments(t, tp2[:, 0].contiguous())
                s.synchronize()
                assert torch.equal(tp2, tp) and torch.equal(tc2, tc)
                page2 = se.rows_of_table(acc, k, after=want[0][:, k - 1])
                assert np_.cpu().numpy().tobytes() == page2[0].tobytes() and nc.cpu().numpy().tobytes() == page2[1].tobytes()
                assert tcuts.shape == (n, k, 8) and tcuts.dtype == torch.float32 and tcuts1.shape == (n, 8)
                _assert_cuts(np.ascontiguousarray(tcuts.cpu().numpy()).view(se.CUT_DTYPE)[..., 0], se.cuts(planes, want[0], rows, spheres=SPHERES, side=1),
                             "torch cuts k=%d" % k)
                _assert_cuts(np.ascontiguousarray(tcuts1.cpu().numpy()).view(se.CUT_DTYPE)[..., 0], se.cuts(planes, want[0][:, 0], rows, spheres=SPHERES),
                             "torch cuts of the first column")
            tp0, tc0 = g.Section(t[:0], k)
            assert tp0.shape == (0, k) and tc0.shape == (0,)
    for bad in (t.cpu(), t.double(), t[:, :5].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.Section(bad, 4)
    cur = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    for bad_after in (cur.cpu(), cur[:-1].contiguous(), cur.float(), np.full(n, -1, np.int32)):
        with pytest.raises(ValueError):
            g.Section(t, 4, after=bad_after)
    for bad_prims in (cur.cpu(), cur[:-1].contiguous(), cur.float(), torch.zeros((n, 17), dtype=torch.int32, device="cuda:0")):
        with pytest.raises(ValueError):
            g.SectionSegments(t, bad_prims)
    flat = t.reshape(-1)
    out = torch.full((8 * 4,), 77, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((8,), 99, dtype=torch.int32, device="cuda:0")
    cut = torch.full((8 * 4 * 8 + 4,), 5.0, dtype=torch.float32, device="cuda:0")
    P, O, Cn, A, X = flat.data_ptr(), out.data_ptr(), cnt.data_ptr(), cur.data_ptr(), cut.data_ptr()
    for args in ((P + 4, None, 8, 4, O, Cn), (P + 8, A, 8, 4, O, Cn)):   # misaligned planes
        assert L.rt_tracer_section_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, None, 8, 4, O, Cn), (P, None, 8, 4, None, Cn), (P, None, 8, 4, O, None), (P, None, 8, 17, O, Cn)):
        assert L.rt_tracer_section_device(g._h, *args, None) == 1
    for args in ((P + 4, O, 8, 4, 0, X), (P, O, 8, 4, 0, X + 4)):       # misaligned planes, misaligned cuts
        assert L.rt_tracer_section_segments_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((P, O, 8, 0, 0, X), (P, O, 8, 17, 0, X), (P, O, 8, 4, 2, X), (None, O, 8, 4, 0, X), (P, None, 8, 4, 0, X), (P, O, 8, 4, 0, None)):
        assert L.rt_tracer_section_segments_device(g._h, *args, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (cnt == 99).all() and (cut == 5.0).all()       # the outputs are untouched
    assert L.rt_tracer_section_device(g._h, None, None, 0, 4, None, None, None) == 0
    assert L.rt_tracer_section_segments_device(g._h, None, None, 0, 4, 0, None, None) == 0
    assert L.rt_tracer_section_device(g._h, P, A, 8, 4, O, Cn, None) == 0
    assert L.rt_tracer_section_segments_device(g._h, P, O, 8, 4, 0, X, None) == 0
    torch.cuda.synchronize()
    want = se.rows_of_table(acc[:8], 4)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and cnt.cpu().numpy().tobytes() == want[1].tobytes()
    _assert_cuts(cut[:256].cpu().numpy().view(se.CUT_DTYPE).reshape(8, 4), se.cuts(planes[:8], want[0], rows, spheres=SPHERES), "device form")
    assert (cut[256:] == 5.0).all()
    # the host forms' errors
    q = np.ascontiguousarray(planes[:70])
    prims = np.full((70, 4), 77, np.int32)
    cnt = np.full(70, 99, np.uint32)
    cuts = np.zeros((70, 4), se.CUT_DTYPE)
    assert L.rt_tracer_section(g._h, None, None, 70, 4, prims.ctypes.data, cnt.ctypes.data) == 1 and "null" in g.LastError()
    assert L.rt_tracer_section(g._h, q.ctypes.data, None, 70, 4, None, cnt.ctypes.data) == 1
    assert L.rt_tracer_section(g._h, q.ctypes.data, None, 70, 17, prims.ctypes.data, cnt.ctypes.data) == 1 and "max_hits" in g.LastError()
    assert (prims == 77).all() and (cnt == 99).all()
    assert L.rt_tracer_section(g._h, q.ctypes.data, None, 70, 0, None, cnt.ctypes.data) == 0            # counts only: prims may be NULL
    assert np.array_equal(cnt, acc[:70].sum(axis=1))
    for per, side, word in ((0, 0, "per_plane"), (17, 0, "per_plane"), (4, 2, "side")):
        assert L.rt_tracer_section_segments(g._h, q.ctypes.data, prims.ctypes.data, 70, per, side, cuts.ctypes.data) == 1 and word in g.LastError()
    assert L.rt_tracer_section_segments(g._h, q.ctypes.data, None, 70, 4, 0, cuts.ctypes.data) == 1 and "null" in g.LastError()
    assert not cuts.view(np.uint8).any()
    with pytest.raises(ValueError):
        g.Section(q, 17)
    for bad in (np.zeros((4, 6), f32), f32(1.0), np.zeros((4, 3), f32)):
        with pytest.raises(ValueError):
            g.Section(bad)
    with pytest.raises(ValueError):
        g.Section(q, 4, after=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        g.SectionSegments(q, np.zeros((69, 4), np.int32))
    with pytest.raises(ValueError):
        g.SectionSegments(q, np.zeros((70, 17), np.int32))
    want = g.Section(q, 16)
    for form in (q[:, :5], se.nan_pads(q)):
        _assert_rows(g.Section(form), want, "plane forms")
    planes4 = q[q[:, 3] == q[:, 4]]
    _assert_rows(g.Section(planes4[:, :4]), tuple(x[q[:, 3] == q[:, 4]] for x in want), "(n, 4) planes")
    assert np.array_equal(R.RayTracer.plane_rows(q[:, :3], q[:, 3], q[:, 4]), np.where(np.arange(8) < 5, q, 0).astype(f32), equal_nan=True)
    g.close()


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    planes = mixed_planes(rows, 500, 3)
    acc = se.table(planes, rows)
    exp = se.rows_of_table(acc, 4)
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_rows(m.Section(planes, 4), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_rows(m.Section(planes, 4), exp, "two bands, bvh")
    _assert_rows(m.Section(planes, 4, after=exp[0][:, 3]), se.rows_of_table(acc, 4, after=exp[0][:, 3]), "two bands, the cursor")
    _assert_cuts(m.SectionSegments(planes, exp[0], side=1), se.cuts(planes, exp[0], rows, side=1), "two bands, the cuts")
    assert m.QueryAccelInfo()["valid"] == 1
    with pytest.raises(R.RtError):
        m._check(R.api.load_library().rt_tracer_section_segments(m._h, planes.ctypes.data, exp[0].ctypes.data, 500, 4, 2, None))
    assert "side" in m.LastError()
    m.close()
