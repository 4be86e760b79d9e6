"""The triangle-shaped region query on the device (RayTracer.OverlapTriangles / OverlapTrianglesAll / SelfIntersections): the
scan and the BVH walk against the numpy restatement of trioverlap_expect, rows and counts exactly, for both upload layouts, both
arithmetic modes (which must not change a byte), with and without spheres, max_hits on both sides of the list-capacity switches
and batches that end in partial waves and blocks; the LDS chunk seams; the continuation cursor; the BVH walk against the scan
kernel byte for byte on 65 536 queries, with any slack; the overflow path; non-finite records and empty scenes; a refitted tree,
a running Trace left alone, multi-device forwarding, the torch path, argument errors; and the self-intersections of a cube."""
import functools
import hashlib

import numpy as np
import pytest

import lattice_cases as lc
import seam_cases as sc
import trioverlap_expect as te
from query_expect import edge_rows
from test_gpu_overlap import COUNTS, KS, SPHERES, _assert_rows, _tracer, assert_block_edges

pytestmark = pytest.mark.gpu

f32 = np.float32


def queries_around(rows, n, seed, grow=2.0, edges=False):
    """n query triangles, each with its corners anywhere in the bounds of a random finite triangle grown on every side by up to
    `grow` times its largest extent (scale free: the deep ladder's clusters span 2^-28 .. 2^41)."""
    rng = np.random.default_rng(seed)
    A, B, C = te.corners(rows, edges)
    fin = np.nonzero(np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1))[0]
    j = fin[rng.integers(0, fin.size, n)]
    mn, mx = np.minimum(np.minimum(A, B), C)[j].astype(np.float64), np.maximum(np.maximum(A, B), C)[j].astype(np.float64)
    ext = (mx - mn).max(axis=1, keepdims=True)
    g = rng.uniform(0.0, grow, (n, 1)) * ext
    return te.queries_of((mn - g)[:, None, :] + rng.uniform(0.0, 1.0, (n, 3, 3)) * (mx - mn + 2 * g)[:, None, :])


def test_query_counts_at_the_wave_and_block_edges():
    rows = te.random_scene(1025, seed=78, span=3.0, edge=0.6)            # one triangle past a chunk, one sphere
    queries = np.concatenate([te.queries_near(rows, 250, 5, edge=5.0), te.bad_queries(te.queries_near(rows, 1, 6)[0])])[:257]
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES[:1])
    assert_block_edges(g, g.OverlapTriangles, queries, te.table(queries, rows, spheres=SPHERES[:1]), te.rows_of_table)
    g.close()


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, 4097 queries of every population, and the verdict table with SPHERES' columns: one table for all."""
    rows = te.random_scene(n_tris, seed=100 + n_tris, span=3.0, edge=0.6)
    queries = te.mixed_queries(rows, 4097, 200 + n_tris)
    queries[:3] = te.queries_of([[[0.5, 0.3, -1.9], [1.4, 0.3, -1.0], [0.5, 1.2, -1.0]],       # cuts the twin spheres
                                 [[0.5, 0.3, -1.0], [0.6, 0.3, -1.0], [0.5, 0.4, -0.9]],       # inside them: touches neither
                                 [[40.0, -35.0, 20.0], [50.0, -35.0, 20.0], [40.0, -20.0, 20.0]]])   # from the far one's centre out
    acc = te.table(queries, rows, spheres=SPHERES)
    for x in (rows, queries, acc):
        x.setflags(write=False)
    return rows, queries, acc


def test_the_populations_reach_what_they_are_for():
    _, queries, acc = _reference(1100)
    counts = acc[:, :1100].sum(axis=1)
    for k in (1, 4):
        assert (counts == 0).any() and (counts == 1).any() and (counts == k).any() and (counts > k).any(), k
    assert (counts > 16).any()
    assert acc[0, 1100] and acc[0, 1101] and not acc[1, 1100:].any() and acc[2, 1102]
    assert np.array_equal(acc[:, 1100], acc[:, 1101])
    assert not np.isfinite(te.corners_of(queries)).all(axis=(1, 2)).all() and np.isnan(queries[:, [3, 7, 11]]).any()


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_max_hits_and_count(n_tris, spheres):
    rows, queries, acc = _reference(n_tris)
    acc = acc if spheres else acc[:, :n_tris]
    exp = {k: te.rows_of_table(acc, k) for k in KS}
    cursor = exp[4][0][:, 3].copy()                                      # a row's last prim where it is full, else none
    exp_after = {k: te.rows_of_table(acc, k, after=cursor) for k in (1, 16)}
    digests = {}
    for edges in (False, True):
        if edges:                                                        # the edge layout's records are the uploaded rows themselves
            assert np.array_equal(te.table(queries, edge_rows(rows), edges=True, spheres=SPHERES if spheres else None), acc)
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
                    got = g.OverlapTriangles(queries, k)
                    _assert_rows(got, exp[k], label)
                    blob.update(got[0].tobytes())
                    blob.update(got[1].tobytes())
                    for n in COUNTS:
                        _assert_rows(g.OverlapTriangles(queries[:n], k), (exp[k][0][:n], exp[k][1][:n]), label + " n=%d" % n)
                for k in (1, 16):
                    _assert_rows(g.OverlapTriangles(queries, k, after=cursor), exp_after[k], "cursor accel=%d k=%d" % (accel, k))
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


def test_the_pinned_zero_area_cases_and_shared_corners():
    for name, rows, query, want in te.degenerate_cases():
        g = _tracer()
        assert g.UploadScene(rows)
        for accel in (False, True):
            g.SetQueryAcceleration(accel)
            assert g.OverlapTriangles(query, 0)[1].tolist() == [int(want)], (name, accel)
        g.close()
    rows = te.random_scene(300, 31)
    for edges in (False, True):
        r = edge_rows(rows) if edges else rows
        g = _tracer()
        assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
        q, tags = te.shared_corner_queries(r, range(300), 32, edges=edges)   # bit-equal to the corners of THIS layout's records
        assert q.shape == (2700, 12)
        for accel in (False, True):
            g.SetQueryAcceleration(accel)
            prims, offsets = g.OverlapTrianglesAll(q)
            for i, (j, s, c) in enumerate(tags):
                assert j in prims[offsets[i]:offsets[i + 1]], (edges, accel, j, s, c)
        g.close()


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_chunk_seams(n_tris):
    """A small upright triangle through each petal's own point touches that petal alone (in the twin layout both twins, the lower
    prim first); a sliver down the stack touches every petal of the seam: the last record of a chunk, the first of the next, the
    last of the scene."""
    h = 1.0 / 16
    for layout in sc.layouts(n_tris):
        rows, info = sc.seam_scene(n_tris, layout)
        tris, want = [], []
        for S, seam in info["seams"].items():
            tie = seam["tie"]
            for i in seam["members"]:
                if tie and i == tie[1]:
                    continue                                             # record S is the twin of S - 1 here: it has no place of its own
                x, y, z = sc.petal_point(i, S) + (sc.petal_z(i, S),)
                tris.append([[x - h, y, z - h], [x + h, y, z - h], [x, y, z + h]])
                want.append([i, tie[1]] if tie and i == tie[0] else [i])
            cx, cy = seam["centre"]
            tris.append([[cx - h, cy, sc.Z0 - h], [cx + h, cy, sc.Z0 - h], [cx, cy, sc.Z0 + 8 * sc.DZ]])
            want.append(list(seam["members"]))
        cx, cy, cz, r = (float(v) for v in sc.SPHERES[0])                # the coincident spheres: prims n_tris and n_tris + 1
        ball = [[[cx + r / 8, cy, cz], [cx, cy + r / 8, cz], [cx, cy, cz + r / 8]],                 # inside the ball: nothing
                [[cx + 1.5 * r, cy, cz], [cx, cy + 1.5 * r, cz], [cx, cy, cz + 1.5 * r]],           # corners outside, the face cuts it
                [[cx + 4 * r, cy, cz], [cx + 5 * r, cy, cz], [cx + 4 * r, cy + r, cz]]]             # beyond
        touched = [False, True, False]
        queries = te.queries_of(tris + ball)
        want += [[]] * 3
        acc = te.table(queries, rows, spheres=sc.SPHERES)
        for row, w in zip(acc, want):
            assert np.nonzero(row[:n_tris])[0].tolist() == w             # the helper says what the scene was made for
        assert acc[-3:, n_tris].tolist() == touched and acc[-3:, n_tris + 1].tolist() == touched and not acc[:, n_tris + 2:].any()
        assert any(n_tris - 1 in w for w in want) and (n_tris < 1024 or any(1023 in w for w in want)) and (n_tris < 1025 or any(1024 in w for w in want))
        for edges in (False, True):
            g = _tracer()
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            g.UploadSpheres(sc.SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 1, 4, 16):
                    _assert_rows(g.OverlapTriangles(queries, k), te.rows_of_table(acc, k), "%d %s edges=%d accel=%d k=%d" % (n_tris, layout, edges, accel, k))
                first = te.rows_of_table(acc, 1)[0][:, 0]
                _assert_rows(g.OverlapTriangles(queries, 4, after=first), te.rows_of_table(acc, 4, after=first), "behind the first prim")
            g.close()


def test_overlap_triangles_all_enumerates_a_stack_once_and_the_cursor_edges():
    z = np.arange(37, dtype=f32)[:, None] / f32(32)                      # 37 parallel triangles and a blade through all of them
    rows = te.queries_of(np.stack([np.c_[-1 + 0 * z, -1 + 0 * z, z], np.c_[1 + 0 * z, -1 + 0 * z, z], np.c_[0 * z, 1 + 0 * z, z]], axis=1)).reshape(-1, 4)
    spheres = f32([[0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.5], [0.0, -0.25, 2.0, 0.25]])
    blade = te.queries_of([[[0, -0.5, -1], [0, 0, 3], [0.125, -0.25, 3]]])
    queries = np.concatenate([blade, te.queries_near(rows, 30, 5, edge=1.0)])
    acc = te.table(queries, rows, spheres=spheres)
    assert acc[0].all() and acc.shape[1] == 40
    sets = te.accepted_sets(acc)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(spheres)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 5, 1):
            prims, offsets = g.OverlapTrianglesAll(queries if k > 1 else queries[:1], k)
            assert prims.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == prims.shape[0]
            assert np.array_equal(prims[offsets[0]:offsets[1]], np.arange(40))      # 0 .. 39, once each, in order
            for i in range(offsets.shape[0] - 1):
                assert np.array_equal(prims[offsets[i]:offsets[i + 1]], sets[i])
        for after, count in ((39, 0), (-1, 40), (5000, 0), (2 ** 31 - 1, 0), (38, 1), (0, 39), (-2, 40), (-2 ** 31, 40)):
            p, c = g.OverlapTriangles(blade, 4, after=np.int32([after]))
            assert c[0] == count, (after, c)
            first = max(after + 1, 0) if after != -1 else 0
            assert p[0].tolist() == [first + s if s < count else -1 for s in range(4)], (after, p)
    g.close()


@pytest.mark.parametrize("scene", ["random10000", "rooms"])
def test_bvh_equals_scan_byte_for_byte_whatever_the_slack(scene):
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "random10000" else lc.rooms()
    second = te.random_queries(25536, 2, edge=1.0, span=2.0, snap=0.25) if scene == "rooms" else queries_around(rows, 25536, 2, grow=10.0)
    queries = np.concatenate([queries_around(rows, 40000, 1), second])
    assert queries.shape[0] == 65536
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.OverlapTriangles(queries, k) for k in (0, 4, 16)}
    assert (scan[16][1] == 0).any() and (scan[16][1] > 16).any()
    _assert_rows(tuple(x[:256] for x in scan[16]), te.expected(queries[:256], rows, 16), "the scan against the helper")
    g.SetQueryAcceleration(True)
    for slack in (1000, 0, 1000000):
        g.DebugQueryAccelSlack(slack)
        for k in (0, 4, 16):
            got = g.OverlapTriangles(queries, k)
            assert got[0].tobytes() == scan[k][0].tobytes() and got[1].tobytes() == scan[k][1].tobytes(), (scene, slack, k)
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_a_shortened_stack_restarts_list_and_count():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    n_tris = rows.shape[0] // 3
    queries = np.concatenate([queries_around(rows, 800, 3), queries_around(rows, 200, 4, grow=40.0)])
    acc = te.table(queries, rows)
    total = acc.sum(axis=1)
    print("deep scene: %d triangles, the most touched by one query: %d" % (n_tris, total.max()))
    assert (total > 16).any() and (total < 16).any() and (total < 3).any()
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.OverlapTriangles(queries, k) for k in (0, 3, 16)}
    for k in scan:
        _assert_rows(scan[k], te.rows_of_table(acc, k), "deep scan k=%d" % k)
    g.SetQueryAcceleration(True)
    try:
        for cap in (None, 0, 1, 3):
            g.DebugQueryStackCap(cap)
            for k in scan:
                _assert_rows(g.OverlapTriangles(queries, k), scan[k], "deep cap=%r k=%d" % (cap, k))
            cursor = scan[3][0][:, 2].copy()
            _assert_rows(g.OverlapTriangles(queries, 16, after=cursor), te.rows_of_table(acc, 16, after=cursor), "deep cap=%r cursor" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                    # (inf - inf and overflow are what the scene is made of)
def test_non_finite_records_empty_scenes_and_spheres_alone():
    rows = te.random_scene(37, 3, span=3.0, edge=0.6).reshape(-1, 3, 4).copy()
    rows[5, 1, 0] = np.nan
    rows[11, 0, 1] = -np.inf
    rows[20, 0, :3], rows[20, 1, :3] = 3.0e38, -3.0e38                   # finite vertices whose edge overflows
    rows[30, 2] = rows[30, 1] = rows[30, 0]                              # a point: a finite record like any other
    rows = rows.reshape(-1, 4)
    p30 = rows[90, :3]
    huge = te.queries_of([[[-3.0e38, -3.0e38, -3.0e38], [3.0e38, 3.0e38, -3.0e38], [0, 3.0e38, 3.0e38]],
                          [[-9, -9, -9], [9, 9, -9], [0, 0, 40]], [p30, p30, p30]])
    queries = np.concatenate([huge, queries_around(rows, 200, 4), te.queries_near(rows, 50, 6, edge=6.0)])
    nothing = np.full_like(rows, np.nan)
    for scene, always in ((rows, 2), (nothing, 37)):
        for edges in (False, True):
            r = edge_rows(scene) if edges else scene
            acc = te.table(queries, r, edges=edges, spheres=SPHERES)
            g = _tracer()
            assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
            g.UploadSpheres(SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 4, 16):
                    _assert_rows(g.OverlapTriangles(queries, k), te.rows_of_table(acc, k), "non-finite edges=%d accel=%d k=%d" % (edges, accel, k))
            info = g.QueryAccelInfo()
            assert info["always_tested"] >= always and (scene is rows or info["nodes"] == 0)
            if scene is rows:
                assert acc[:, :37].any() and not acc[:, 5].any() and not acc[:, 11].any() and acc[2, 30]
            else:
                assert not acc[:, :37].any() and acc[:, 37:39].any()
            g.close()
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        prims, counts = g.OverlapTriangles(queries, 5)                   # no scene: nothing to touch
        assert prims.shape == (queries.shape[0], 5) and not counts.any() and (prims == -1).all()
        prims, counts = g.OverlapTriangles(np.zeros((0, 12), f32), 3)
        assert prims.shape == (0, 3) and counts.shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        acc = te.table(queries, None, spheres=SPHERES)
        assert acc.any()
        for k in KS:
            _assert_rows(g.OverlapTriangles(queries, k), te.rows_of_table(acc, k), "spheres only accel=%d k=%d" % (accel, k))
        g.close()


def test_argument_errors_leave_the_outputs_untouched_and_triangle_forms_agree():
    import raytracertest_amd as R
    rows, queries, acc = _reference(37)
    L = R.api.load_library()
    g = _tracer()
    assert g.UploadScene(rows)
    q = np.ascontiguousarray(queries[:70])
    prims = np.full((70, 4), 77, np.int32)
    cnt = np.full(70, 99, np.uint32)
    assert L.rt_tracer_overlap_triangles(g._h, None, None, 70, 4, prims.ctypes.data, cnt.ctypes.data) == 1 and "null" in g.LastError()
    assert L.rt_tracer_overlap_triangles(g._h, q.ctypes.data, None, 70, 4, None, cnt.ctypes.data) == 1
    assert L.rt_tracer_overlap_triangles(g._h, q.ctypes.data, None, 70, 4, prims.ctypes.data, None) == 1
    assert L.rt_tracer_overlap_triangles(g._h, q.ctypes.data, None, 70, 17, prims.ctypes.data, cnt.ctypes.data) == 1 and "max_hits" in g.LastError()
    assert (prims == 77).all() and (cnt == 99).all()
    assert L.rt_tracer_overlap_triangles(g._h, None, None, 0, 4, None, None) == 0             # n = 0 is a no-op
    assert L.rt_tracer_overlap_triangles(g._h, q.ctypes.data, None, 70, 0, None, cnt.ctypes.data) == 0   # counts only: prims may be NULL
    assert np.array_equal(cnt, acc[:70, :37].sum(axis=1))
    with pytest.raises(ValueError):
        g.OverlapTriangles(q, 17)
    for bad in (np.zeros((4, 5), f32), f32(1.0), np.zeros((4, 8), f32)):
        with pytest.raises(ValueError):
            g.OverlapTriangles(bad)
    with pytest.raises(ValueError):
        g.OverlapTriangles(q, 4, after=np.zeros(3, np.int32))
    want = g.OverlapTriangles(q, 16)
    c = te.corners_of(q)
    for form in (c, c.reshape(-1, 9), te.nan_pads(q)):
        _assert_rows(g.OverlapTriangles(form), want, "triangle forms")
    g.close()


def test_torch_path_on_a_side_stream_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, queries, acc = _reference(1100)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(queries)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 4, 0):
            want = te.rows_of_table(acc, k)
            tp, tc = g.OverlapTriangles(t, k)
            assert tp.dtype == torch.int32 and tp.shape == (4097, k) and tc.dtype == torch.int32 and tc.shape == (4097,)
            assert tp.cpu().numpy().tobytes() == want[0].tobytes() and tc.cpu().numpy().tobytes() == want[1].tobytes()
            if k:
                after = tp[:, k - 1].contiguous()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):                               # on the caller's current stream
                    tp2, tc2 = g.OverlapTriangles(t, k)
                    np_, nc = g.OverlapTriangles(t, k, after=after)
                s.synchronize()
                assert torch.equal(tp2, tp) and torch.equal(tc2, tc)
                page2 = te.rows_of_table(acc, k, after=want[0][:, k - 1])
                assert np_.cpu().numpy().tobytes() == page2[0].tobytes() and nc.cpu().numpy().tobytes() == page2[1].tobytes()
            tp0, tc0 = g.OverlapTriangles(t[:0], k)
            assert tp0.shape == (0, k) and tc0.shape == (0,)
    for bad in (t.cpu(), t.double(), t[:, :9].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.OverlapTriangles(bad, 4)
    cur = torch.full((4097,), -1, dtype=torch.int32, device="cuda:0")
    for bad_after in (cur.cpu(), cur[:-1].contiguous(), cur.float(), np.full(4097, -1, np.int32)):
        with pytest.raises(ValueError):
            g.OverlapTriangles(t, 4, after=bad_after)
    flat = t.reshape(-1)
    out = torch.full((8 * 4,), 77, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((8,), 99, dtype=torch.int32, device="cuda:0")
    P, O, Cn, A = flat.data_ptr(), out.data_ptr(), cnt.data_ptr(), cur.data_ptr()
    for args in ((P + 4, None, 8, 4, O, Cn), (P + 8, A, 8, 4, O, Cn)):   # misaligned triangles
        assert L.rt_tracer_overlap_triangles_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, None, 8, 4, O, Cn), (P, None, 8, 4, None, Cn), (P, None, 8, 4, O, None), (P, None, 8, 17, O, Cn)):
        assert L.rt_tracer_overlap_triangles_device(g._h, *args, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (cnt == 99).all()                       # the outputs are untouched
    assert L.rt_tracer_overlap_triangles_device(g._h, None, None, 0, 4, None, None, None) == 0
    assert L.rt_tracer_overlap_triangles_device(g._h, P, A, 8, 4, O, Cn, None) == 0
    torch.cuda.synchronize()
    want = te.rows_of_table(acc[:8], 4)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and cnt.cpu().numpy().tobytes() == want[1].tobytes()
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    queries = queries_around(moved, 8192, 9)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.OverlapTriangles(queries, 16)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = {k: g.OverlapTriangles(queries, k) for k in (16, 4, 0)}        # the first of them refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    for k in (16, 4, 0):
        _assert_rows(got[k], g.OverlapTriangles(queries, k), "after the refit k=%d" % k)
    assert (first[0] != got[16][0]).any()                                # the scene did move
    _assert_rows(tuple(x[:512] for x in got[16]), te.expected(queries[:512], moved, 16), "the moved scene against the helper")
    g.close()


def test_overlap_triangles_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    queries = queries_around(rows, 4096, 7)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.OverlapTriangles(queries, 16)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.OverlapTriangles(queries, 16 if i % 4 < 2 else 4))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(8)
    assert len(got) == 8 and idle[1].any()
    for p, c in got:
        assert np.array_equal(p, idle[0][:, :p.shape[1]]) and np.array_equal(c, idle[1])
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    queries = queries_around(rows, 2000, 3, grow=0.5)
    acc = te.table(queries, rows)
    exp = te.rows_of_table(acc, 4)
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_rows(one.OverlapTriangles(queries, 4), exp, "one band against the helper")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_rows(m.OverlapTriangles(queries, 4), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_rows(m.OverlapTriangles(queries, 4), exp, "two bands, bvh")
    _assert_rows(m.OverlapTriangles(queries, 4, after=exp[0][:, 3]), te.rows_of_table(acc, 4, after=exp[0][:, 3]), "two bands, the cursor")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()


@pytest.mark.parametrize("edges", [False, True])
def test_self_intersections_of_a_cube_and_of_a_poked_cube(edges):
    for rows, want in ((te.cube_rows(), []), te.poked_cube_rows()):
        g = _tracer()
        assert g.SelfIntersections().shape == (0, 2)                     # no scene
        assert (g.UploadSceneEdges(te.to_edges(rows)) if edges else g.UploadScene(rows))
        g.UploadSpheres(SPHERES)                                         # spheres take no part
        for accel in (False, True):
            g.SetQueryAcceleration(accel)
            pairs = g.SelfIntersections()
            assert pairs.dtype == np.int32 and pairs.tolist() == [list(p) for p in want], (edges, accel)
        g.close()
