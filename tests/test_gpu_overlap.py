"""The region query on the device (RayTracer.Overlap / OverlapAll / Voxelize): the scan and the BVH walk against the numpy
restatement of overlap_expect, rows and counts exactly, for both upload layouts, both arithmetic modes (which must not change a
byte), with and without spheres, max_hits on both sides of the list-capacity switches and batches that end in partial waves and
blocks; the LDS chunk seams; the continuation cursor; the BVH walk against the scan kernel byte for byte on 65 536 boxes, with
any slack; the overflow path; non-finite records and empty scenes; a refitted tree, a running Trace left alone, multi-device
forwarding, the torch path, argument errors; and the voxelisation of a cube."""
import functools
import hashlib

import numpy as np
import pytest

import lattice_cases as lc
import overlap_expect as oe
import seam_cases as sc
from query_expect import edge_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
# two coincident spheres (both are listed, the lower prim first), among the triangles; one far away
SPHERES = f32([[0.5, 0.3, -1.0, 0.8], [0.5, 0.3, -1.0, 0.8], [40.0, -35.0, 20.0, 6.0]])
COUNTS = (1, 63, 64, 65)                                                 # partial waves; 4097 is a partial last block as well
KS = (0, 1, 3, 4, 5, 16)                                                 # 0 | 1: no list; 4 | 5: the list of 4 slots gives way to the one of 16


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _assert_rows(got, exp, label):
    prims, counts = got
    assert prims.dtype == np.int32 and prims.shape == exp[0].shape and counts.dtype == np.uint32 and counts.shape == exp[1].shape, label
    bad = np.nonzero((prims != exp[0]).any(axis=1) | (counts != exp[1]))[0]
    assert bad.size == 0, (label, bad.size, bad[:5], prims[bad[:2]], exp[0][bad[:2]], counts[bad[:3]], exp[1][bad[:3]])


EDGE_COUNTS = (1, 63, 64, 65, 255, 256, 257)       # the tree kernel's i >= n return; the last block of the scan, whose padding lanes
#                                                    must accept nothing and store nothing


def assert_block_edges(g, query, queries, acc, rows_of_table):
    """query (a bound method of g over 257 queries, acc their verdict table) at every count of EDGE_COUNTS, scan and tree, with
    no list and with one; the rows behind the count stay the caller's."""
    assert queries.shape[0] == 257
    exp = {k: rows_of_table(acc, k) for k in (0, 4)}
    assert (exp[0][1] > 4).any() and (exp[0][1] == 0).any()
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (0, 4):
            for n in EDGE_COUNTS:
                _assert_rows(query(queries[:n], k), (exp[k][0][:n], exp[k][1][:n]), "accel=%d k=%d n=%d" % (accel, k, n))


def test_query_counts_at_the_wave_and_block_edges():
    rows = oe.random_scene(1025, seed=77, span=3.0, edge=0.6)            # one triangle past a chunk, one sphere
    boxes = np.concatenate([oe.random_boxes(rows, 250, 5, width=1.5), oe.bad_boxes(oe.whole_box(rows)[0])])[:257]
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES[:1])
    assert_block_edges(g, g.Overlap, boxes, oe.table(boxes, rows, spheres=SPHERES[:1]), oe.rows_of_table)
    g.close()


def boxes_around(rows, n, seed, grow=2.0, edges=False):
    """n boxes, each the bounds of a random finite triangle grown on every side by up to `grow` times its largest extent (scale
    free: the deep ladder's clusters span 2^-28 .. 2^41)."""
    rng = np.random.default_rng(seed)
    A, B, C = oe.corners(rows, edges)
    fin = np.nonzero(np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1))[0]
    j = fin[rng.integers(0, fin.size, n)]
    mn, mx = np.minimum(np.minimum(A, B), C)[j].astype(np.float64), np.maximum(np.maximum(A, B), C)[j].astype(np.float64)
    ext = (mx - mn).max(axis=1, keepdims=True)
    return oe.boxes_of(mn - rng.uniform(-0.25, grow, (n, 3)) * ext, mx + rng.uniform(-0.25, grow, (n, 3)) * ext)


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, 4097 boxes of every population, and the verdict table with SPHERES' columns: one table for all."""
    rows = oe.random_scene(n_tris, seed=100 + n_tris, span=3.0, edge=0.6)
    tris = np.arange(0, n_tris, max(1, n_tris // 40))
    touching, _ = oe.touching_boxes(rows, tris)
    whole = oe.whole_box(rows, SPHERES)
    special = [touching, oe.point_boxes(rows, tris), whole, oe.bad_boxes(whole[0]), oe.unbounded_boxes(whole[0]),
               oe.sphere_boxes(SPHERES[0])[0], oe.sphere_boxes(SPHERES[2])[0], oe.nan_pads(touching[:16])]
    n_special = sum(b.shape[0] for b in special)
    n_rand = 4097 - n_special
    boxes = np.concatenate([oe.random_boxes(rows, n_rand // 2, 200 + n_tris, width=0.6), boxes_around(rows, n_rand - n_rand // 2, 300 + n_tris)] + special)
    boxes = np.ascontiguousarray(boxes[np.random.default_rng(n_tris).permutation(4097)])
    acc = oe.table(boxes, rows, spheres=SPHERES)
    for x in (rows, boxes, acc):
        x.setflags(write=False)
    return rows, boxes, acc


def test_the_populations_reach_what_they_are_for():
    _, boxes, acc = _reference(1100)
    counts = acc[:, :1100].sum(axis=1)
    for k in (1, 4, 16):
        assert (counts == 0).any() and (counts == 1).any() and (counts == k).any() and (counts > k).any(), k
    assert acc[:, 1100].any() and np.array_equal(acc[:, 1100], acc[:, 1101]) and not acc[:, 1100].all()
    assert (acc.sum(axis=1) == 1103).any()                               # the whole-scene box


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_max_hits_and_count(n_tris, spheres):
    rows, boxes, acc = _reference(n_tris)
    acc = acc if spheres else acc[:, :n_tris]
    exp = {k: oe.rows_of_table(acc, k) for k in KS}
    cursor = exp[4][0][:, 3].copy()                                      # a row's last prim where it is full, else none
    exp_after = {k: oe.rows_of_table(acc, k, after=cursor) for k in (1, 16)}
    digests = {}
    for edges in (False, True):
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
                    got = g.Overlap(boxes, k)
                    _assert_rows(got, exp[k], label)
                    blob.update(got[0].tobytes())
                    blob.update(got[1].tobytes())
                    for n in COUNTS:
                        _assert_rows(g.Overlap(boxes[:n], k), (exp[k][0][:n], exp[k][1][:n]), label + " n=%d" % n)
                for k in (1, 16):
                    _assert_rows(g.Overlap(boxes, k, after=cursor), exp_after[k], "cursor accel=%d k=%d" % (accel, k))
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_chunk_seams(n_tris):
    """A box around each petal's own point touches that petal alone (in the twin layout both twins, the lower prim first); a box
    down the stack touches every petal of the seam: the last record of a chunk, the first of the next, the last of the scene."""
    h = 1.0 / 16
    for layout in sc.layouts(n_tris):
        rows, info = sc.seam_scene(n_tris, layout)
        lo, hi, want = [], [], []
        for S, seam in info["seams"].items():
            tie = seam["tie"]
            for i in seam["members"]:
                if tie and i == tie[1]:
                    continue                                             # record S is the twin of S - 1 here: it has no place of its own
                x, y, z = sc.petal_point(i, S) + (sc.petal_z(i, S),)
                lo.append((x - h, y - h, z - h)), hi.append((x + h, y + h, z + h))
                want.append([i, tie[1]] if tie and i == tie[0] else [i])
            cx, cy = seam["centre"]
            lo.append((cx - h, cy - h, sc.Z0 - h)), hi.append((cx + h, cy + h, sc.Z0 + 8 * sc.DZ))
            want.append(list(seam["members"]))
        ball, touched = oe.sphere_boxes(sc.SPHERES[0])                   # the coincident spheres: prims n_tris and n_tris + 1
        boxes = np.concatenate([oe.boxes_of(lo, hi), ball])
        want += [[]] * ball.shape[0]
        acc = oe.table(boxes, rows, spheres=sc.SPHERES)
        for r, w in zip(acc, want):
            assert np.nonzero(r[:n_tris])[0].tolist() == w               # the helper says what the scene was made for
        assert acc[-5:, n_tris].tolist() == touched.tolist() and acc[-5:, n_tris + 1].tolist() == touched.tolist() and not acc[:, n_tris + 2:].any()
        assert any(n_tris - 1 in w for w in want) and (n_tris < 1024 or any(1023 in w for w in want)) and (n_tris < 1025 or any(1024 in w for w in want))
        for edges in (False, True):
            g = _tracer()
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            g.UploadSpheres(sc.SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 1, 4, 16):
                    _assert_rows(g.Overlap(boxes, k), oe.rows_of_table(acc, k), "%d %s edges=%d accel=%d k=%d" % (n_tris, layout, edges, accel, k))
                first = oe.rows_of_table(acc, 1)[0][:, 0]
                _assert_rows(g.Overlap(boxes, 4, after=first), oe.rows_of_table(acc, 4, after=first), "behind the first prim")
            g.close()


def test_overlap_all_enumerates_the_whole_scene_once_and_the_cursor_edges():
    rows, _, _ = _reference(1100)
    whole = oe.whole_box(rows, SPHERES)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    boxes = np.concatenate([whole, oe.random_boxes(rows, 30, 5, width=2.0)])
    sets = oe.accepted_sets(oe.table(boxes, rows, spheres=SPHERES))
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 5, 1):
            prims, offsets = g.OverlapAll(boxes if k > 1 else boxes[:1], k)
            assert prims.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == prims.shape[0]
            assert np.array_equal(prims[offsets[0]:offsets[1]], np.arange(1103))   # 0 .. 1102, once each, in order
            for i in range(offsets.shape[0] - 1):
                assert np.array_equal(prims[offsets[i]:offsets[i + 1]], sets[i])
        for after, count in ((1102, 0), (-1, 1103), (5000, 0), (2 ** 31 - 1, 0), (1101, 1), (0, 1102), (-2, 1103), (-2 ** 31, 1103)):
            p, c = g.Overlap(whole, 4, after=np.int32([after]))
            assert c[0] == count, (after, c)
            first = max(after + 1, 0) if after != -1 else 0
            assert p[0].tolist() == [first + s if s < count else -1 for s in range(4)], (after, p)
    g.close()


@pytest.mark.parametrize("scene", ["random10000", "rooms"])
def test_bvh_equals_scan_byte_for_byte_whatever_the_slack(scene):
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "random10000" else lc.rooms()
    boxes = np.concatenate([boxes_around(rows, 40000, 1), oe.random_boxes(rows, 25536, 2, width=1.0, snap=0.25 if scene == "rooms" else None)])
    assert boxes.shape[0] == 65536
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.Overlap(boxes, k) for k in (0, 4, 16)}
    assert (scan[16][1] == 0).any() and (scan[16][1] > 16).any()
    g.SetQueryAcceleration(True)
    for slack in (1000, 0, 1000000):
        g.DebugQueryAccelSlack(slack)
        for k in (0, 4, 16):
            got = g.Overlap(boxes, k)
            assert got[0].tobytes() == scan[k][0].tobytes() and got[1].tobytes() == scan[k][1].tobytes(), (scene, slack, k)
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_a_shortened_stack_restarts_list_and_count():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    n_tris = rows.shape[0] // 3
    boxes = np.concatenate([boxes_around(rows, 800, 3), boxes_around(rows, 200, 4, grow=40.0), oe.whole_box(rows)])
    acc = oe.table(boxes, rows)
    total = acc.sum(axis=1)
    assert (total > 16).any() and (total < 16).any() and (total < 3).any() and total[-1] == n_tris
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.Overlap(boxes, k) for k in (0, 3, 16)}
    for k in scan:
        _assert_rows(scan[k], oe.rows_of_table(acc, k), "deep scan k=%d" % k)
    g.SetQueryAcceleration(True)
    try:
        for cap in (None, 0, 1, 3):
            g.DebugQueryStackCap(cap)
            for k in scan:
                _assert_rows(g.Overlap(boxes, k), scan[k], "deep cap=%r k=%d" % (cap, k))
            cursor = scan[3][0][:, 2].copy()
            _assert_rows(g.Overlap(boxes, 16, after=cursor), oe.rows_of_table(acc, 16, after=cursor), "deep cap=%r cursor" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                    # (inf - inf and overflow are what the scene is made of)
def test_non_finite_records_empty_scenes_and_spheres_alone():
    rows = oe.random_scene(37, 3, span=3.0, edge=0.6).reshape(-1, 3, 4).copy()
    rows[5, 1, 0] = np.nan
    rows[11, 0, 1] = -np.inf
    rows[20, 0, :3], rows[20, 1, :3] = 3.0e38, -3.0e38                   # finite vertices whose edge overflows
    rows[30, 2] = rows[30, 1] = rows[30, 0]                              # a point: a finite record like any other
    rows = rows.reshape(-1, 4)
    good = oe.whole_box(rows)
    boxes = np.concatenate([good, oe.unbounded_boxes(good[0]), oe.boxes_of([-3.0e38] * 3, [3.0e38] * 3), boxes_around(rows, 200, 4), oe.point_boxes(rows, [30])])
    nothing = np.full_like(rows, np.nan)
    for scene, always in ((rows, 2), (nothing, 37)):
        for edges in (False, True):
            r = edge_rows(scene) if edges else scene
            acc = oe.table(boxes, r, edges=edges, spheres=SPHERES)
            g = _tracer()
            assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
            g.UploadSpheres(SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 4, 16):
                    _assert_rows(g.Overlap(boxes, k), oe.rows_of_table(acc, k), "non-finite edges=%d accel=%d k=%d" % (edges, accel, k))
            info = g.QueryAccelInfo()
            assert info["always_tested"] >= always and (scene is rows or info["nodes"] == 0)
            if scene is rows:
                assert acc[0, :37].sum() >= 34 and not acc[:, 5].any() and not acc[:, 11].any() and acc[-1, 30]
            else:
                assert not acc[:, :37].any() and acc[0, 37:39].all()
            g.close()
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        prims, counts = g.Overlap(boxes, 5)                              # no scene: nothing to touch
        assert prims.shape == (boxes.shape[0], 5) and not counts.any() and (prims == -1).all()
        prims, counts = g.Overlap(np.zeros((0, 8), f32), 3)
        assert prims.shape == (0, 3) and counts.shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        acc = oe.table(boxes, None, spheres=SPHERES)
        assert acc.any()
        for k in KS:
            _assert_rows(g.Overlap(boxes, k), oe.rows_of_table(acc, k), "spheres only accel=%d k=%d" % (accel, k))
        sb, _ = oe.sphere_boxes(SPHERES[0])
        counts = g.Overlap(sb, 0)[1]
        assert np.array_equal(counts, 2 * oe.sphere_rule(sb, SPHERES[:1])[:, 0]) and counts[:3].tolist() == [0, 2, 2] and counts[4] == 0   # inside the ball: nothing; the twins together
        g.close()


def test_argument_errors_leave_the_outputs_untouched_and_box_forms_agree():
    import raytracertest_amd as R
    rows, boxes, acc = _reference(37)
    L = R.api.load_library()
    g = _tracer()
    assert g.UploadScene(rows)
    b = np.ascontiguousarray(boxes[:70])
    prims = np.full((70, 4), 77, np.int32)
    cnt = np.full(70, 99, np.uint32)
    assert L.rt_tracer_overlap(g._h, None, None, 70, 4, prims.ctypes.data, cnt.ctypes.data) == 1 and "null" in g.LastError()
    assert L.rt_tracer_overlap(g._h, b.ctypes.data, None, 70, 4, None, cnt.ctypes.data) == 1
    assert L.rt_tracer_overlap(g._h, b.ctypes.data, None, 70, 4, prims.ctypes.data, None) == 1
    assert L.rt_tracer_overlap(g._h, b.ctypes.data, None, 70, 17, prims.ctypes.data, cnt.ctypes.data) == 1 and "max_hits" in g.LastError()
    assert (prims == 77).all() and (cnt == 99).all()
    assert L.rt_tracer_overlap(g._h, None, None, 0, 4, None, None) == 0             # n = 0 is a no-op
    assert L.rt_tracer_overlap(g._h, b.ctypes.data, None, 70, 0, None, cnt.ctypes.data) == 0   # counts only: prims may be NULL
    assert np.array_equal(cnt, acc[:70, :37].sum(axis=1))
    with pytest.raises(ValueError):
        g.Overlap(b, 17)
    for bad in (np.zeros((4, 5), f32), f32(1.0)):
        with pytest.raises(ValueError):
            g.Overlap(bad)
    with pytest.raises(ValueError):
        g.Overlap(b, 4, after=np.zeros(3, np.int32))
    want = g.Overlap(b, 16)
    six = np.ascontiguousarray(b[:, [0, 1, 2, 4, 5, 6]])
    for form in (six, (b[:, 0:3], b[:, 4:7]), oe.nan_pads(b)):
        _assert_rows(g.Overlap(form), want, "box forms")
    g.close()


def test_torch_path_on_a_side_stream_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, boxes, acc = _reference(1100)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(boxes)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 4, 0):
            want = oe.rows_of_table(acc, k)
            tp, tc = g.Overlap(t, k)
            assert tp.dtype == torch.int32 and tp.shape == (4097, k) and tc.dtype == torch.int32 and tc.shape == (4097,)
            assert tp.cpu().numpy().tobytes() == want[0].tobytes() and tc.cpu().numpy().tobytes() == want[1].tobytes()
            if k:
                after = tp[:, k - 1].contiguous()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):                               # on the caller's current stream
                    tp2, tc2 = g.Overlap(t, k)
                    np_, nc = g.Overlap(t, k, after=after)
                s.synchronize()
                assert torch.equal(tp2, tp) and torch.equal(tc2, tc)
                page2 = oe.rows_of_table(acc, k, after=want[0][:, k - 1])
                assert np_.cpu().numpy().tobytes() == page2[0].tobytes() and nc.cpu().numpy().tobytes() == page2[1].tobytes()
            tp0, tc0 = g.Overlap(t[:0], k)
            assert tp0.shape == (0, k) and tc0.shape == (0,)
    for bad in (t.cpu(), t.double(), t[:, :6].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.Overlap(bad, 4)
    cur = torch.full((4097,), -1, dtype=torch.int32, device="cuda:0")
    for bad_after in (cur.cpu(), cur[:-1].contiguous(), cur.float(), np.full(4097, -1, np.int32)):
        with pytest.raises(ValueError):
            g.Overlap(t, 4, after=bad_after)
    flat = t.reshape(-1)
    out = torch.full((8 * 4,), 77, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((8,), 99, dtype=torch.int32, device="cuda:0")
    P, O, Cn, A = flat.data_ptr(), out.data_ptr(), cnt.data_ptr(), cur.data_ptr()
    for args in ((P + 4, None, 8, 4, O, Cn), (P + 8, A, 8, 4, O, Cn)):   # misaligned boxes
        assert L.rt_tracer_overlap_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, None, 8, 4, O, Cn), (P, None, 8, 4, None, Cn), (P, None, 8, 4, O, None), (P, None, 8, 17, O, Cn)):
        assert L.rt_tracer_overlap_device(g._h, *args, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (cnt == 99).all()                       # the outputs are untouched
    assert L.rt_tracer_overlap_device(g._h, None, None, 0, 4, None, None, None) == 0
    assert L.rt_tracer_overlap_device(g._h, P, A, 8, 4, O, Cn, None) == 0
    torch.cuda.synchronize()
    want = oe.rows_of_table(acc[:8], 4)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and cnt.cpu().numpy().tobytes() == want[1].tobytes()
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    boxes = boxes_around(moved, 8192, 9)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.Overlap(boxes, 16)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = {k: g.Overlap(boxes, k) for k in (16, 4, 0)}                   # the first of them refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    for k in (16, 4, 0):
        _assert_rows(got[k], g.Overlap(boxes, k), "after the refit k=%d" % k)
    assert (first[0] != got[16][0]).any()                                # the scene did move
    _assert_rows(tuple(x[:512] for x in got[16]), oe.expected(boxes[:512], moved, 16), "the moved scene against the helper")
    g.close()


def test_overlap_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    boxes = boxes_around(rows, 4096, 7)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Overlap(boxes, 16)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.Overlap(boxes, 16 if i % 4 < 2 else 4))
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
    boxes = boxes_around(rows, 2000, 3, grow=0.5)
    acc = oe.table(boxes, rows)
    exp = oe.rows_of_table(acc, 4)
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_rows(one.Overlap(boxes, 4), exp, "one band against the helper")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_rows(m.Overlap(boxes, 4), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_rows(m.Overlap(boxes, 4), exp, "two bands, bvh")
    _assert_rows(m.Overlap(boxes, 4, after=exp[0][:, 3]), oe.rows_of_table(acc, 4, after=exp[0][:, 3]), "two bands, the cursor")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()


def test_voxelize_a_dyadic_cube_gives_the_analytic_shell():
    """The unit cube [0, 1]^3 as 12 triangles on the grid origin -1/2, spacing 1/4, 8^3 voxels: voxel (i, j, k) spans
    [-1/2 + i/4, -1/4 + i/4] per axis.  A closed voxel touches the cube's surface exactly when it meets the closed cube on every
    axis and does not lie strictly inside it on all three.  Everything is dyadic: the arithmetic is exact and touching counts."""
    q = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
    faces = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    tris = np.array([[q[a], q[b], q[c]] for f in faces for (a, b, c) in ((f[0], f[1], f[2]), (f[0], f[2], f[3]))])
    rows = np.zeros((12, 3, 4), f32)
    rows[:, :, :3] = tris
    a = -0.5 + 0.25 * np.arange(8)
    b = a + 0.25
    meets, inside = (b >= 0) & (a <= 1), (a > 0) & (b < 1)
    M = meets[:, None, None] & meets[None, :, None] & meets[None, None, :]
    I = inside[:, None, None] & inside[None, :, None] & inside[None, None, :]
    shell = M & ~I
    assert shell.sum() == 6 ** 3 - 2 ** 3
    g = _tracer()
    assert g.UploadScene(rows.reshape(-1, 4))
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        vox = g.Voxelize((-0.5, -0.5, -0.5), 0.25, (8, 8, 8))
        assert vox.dtype == np.bool_ and vox.shape == (8, 8, 8) and np.array_equal(vox, shell), accel
        assert np.array_equal(g.Voxelize((-0.5, -0.5, 0.0), (0.25, 0.25, 0.5), (8, 8, 1)), shell[:, :, 2:4].any(axis=2, keepdims=True))
    assert g.Voxelize((0, 0, 0), 1.0, (0, 3, 3)).shape == (0, 3, 3)
    g.close()
