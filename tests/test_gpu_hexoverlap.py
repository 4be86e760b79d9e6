"""The hexahedron-shaped region query on the device (RayTracer.OverlapHexahedra / OverlapHexahedraAll / PixelFrustum /
SelectRect): the scan and the BVH walk against the numpy restatement of hexoverlap_expect, rows and counts exactly, for both
upload layouts, both arithmetic modes (which must not change a byte), with and without spheres, max_hits on both sides of the
list-capacity switches and batches that end in partial waves; the LDS chunk seams; the continuation cursor; the BVH walk against
the scan byte for byte with any slack; the overflow path; non-finite regions and records, empty scenes; degenerate regions
against IntersectAll; aligned boxes against Overlap on the 1/8 lattice; pixel frusta against Pick; a refitted tree, a running
Trace left alone, multi-device forwarding, the torch path and argument errors."""
import functools
import hashlib

import numpy as np
import pytest

import hexoverlap_expect as he
import lattice_cases as lc
import overlap_expect as oe
import seam_cases as sc
from query_expect import edge_rows
from test_gpu_overlap import COUNTS, SPHERES, _assert_rows, _tracer, assert_block_edges

pytestmark = pytest.mark.gpu

f32 = np.float32
KS = (0, 1, 4, 5, 16)                                                    # 0: no list; 4 | 5: the list of 4 slots gives way to the one of 16


def regions_around(rows, n, seed, grow=2.0, edges=False):
    """n regions of the five kinds, each about the size of a random finite triangle's bounds grown by up to `grow` times (scale
    free)."""
    rng = np.random.default_rng(seed)
    A, B, C = he.corners(rows, edges)
    fin = np.nonzero(np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1) & np.isfinite(C).all(axis=1))[0]
    j = fin[rng.integers(0, fin.size, n)]
    mn, mx = np.minimum(np.minimum(A, B), C)[j].astype(np.float64), np.maximum(np.maximum(A, B), C)[j].astype(np.float64)
    ext = (mx - mn).max(axis=1)
    size = ext * (1.0 + rng.uniform(0.0, grow, n))
    centres = (mn + mx) / 2 + rng.uniform(-0.5, 0.5, (n, 3)) * size[:, None]
    unit = np.concatenate([he.frusta(np.zeros((n, 3)), seed + 1, 1.0)[0::5], he.sheared_boxes(np.zeros((n, 3)), seed + 2, 1.0)[1::5],
                           he.frusta(np.zeros((n, 3)), seed + 3, 1.0, pyramid=True)[2::5], he.random_segments(np.zeros((n, 3)), seed + 4, 1.0)[3::5],
                           he.aligned_boxes(np.zeros((n, 3)), seed + 5, 1.0)[4::5]])
    order = rng.permutation(n)
    return he.queries_of(unit[order].astype(np.float64) * size[:, None, None] + centres[:, None, :])


def test_query_counts_at_the_wave_and_block_edges():
    rows = he.random_scene(1025, seed=79, span=3.0, edge=0.6)            # one triangle past a chunk, one sphere
    queries = np.concatenate([he.regions_near(rows, 250, 5, size=1.0), he.bad_queries(he.regions_near(rows, 1, 6)[0])])[:257]
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES[:1])
    assert_block_edges(g, g.OverlapHexahedra, queries, he.table(queries, rows, spheres=SPHERES[:1]), he.rows_of_table)
    g.close()


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene, the mixed regions and the verdict table with SPHERES' columns: one table for all."""
    rows = he.random_scene(n_tris, seed=100 + n_tris, span=3.0, edge=0.6)
    n = 257 if n_tris >= 1000 else 300
    queries = he.mixed_queries(rows, n, 200 + n_tris)
    queries[:4] = he.queries_of(np.concatenate([
        he.box_corners([0.4, 0.2, -1.9], [0.6, 0.4, -1.0]),              # cuts the twin spheres
        he.box_corners([0.4, 0.2, -1.1], [0.6, 0.4, -0.9]),              # inside them: touches neither
        he.box_corners([-1.0, -1.0, -2.5], [2.0, 2.0, 0.5]),             # they are wholly inside it: accepted
        he.box_corners([40.0, -35.0, 20.0], [50.0, -25.0, 30.0])]))      # from the far one's centre out
    acc = he.table(queries, rows, spheres=SPHERES)
    for x in (rows, queries, acc):
        x.setflags(write=False)
    return rows, queries, acc


def test_the_populations_reach_what_they_are_for():
    _, queries, acc = _reference(1100)
    counts = acc[:, :1100].sum(axis=1)
    for k in (1, 4):
        assert (counts == 0).any() and (counts == 1).any() and (counts > k).any(), k
    assert (counts > 16).any()
    assert acc[0, 1100] and acc[0, 1101] and not acc[1, 1100:].any() and acc[2, 1100] and acc[2, 1101] and acc[3, 1102]
    assert np.array_equal(acc[:, 1100], acc[:, 1101])
    assert not np.isfinite(he.corners_of(queries)).all(axis=(1, 2)).all() and np.isnan(queries[:, 3::4]).any()


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_helper_every_layout_mode_max_hits_and_count(n_tris, spheres):
    rows, queries, acc = _reference(n_tris)
    acc = acc if spheres else acc[:, :n_tris]
    exp = {k: he.rows_of_table(acc, k) for k in KS}
    cursor = exp[4][0][:, 3].copy()                                      # a row's last prim where it is full, else none
    exp_after = {k: he.rows_of_table(acc, k, after=cursor) for k in (1, 16)}
    digests = {}
    for edges in (False, True):
        if edges:                                                        # the edge layout's records are the uploaded rows themselves
            assert np.array_equal(he.table(queries, edge_rows(rows), edges=True, spheres=SPHERES if spheres else None), acc)
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
                    got = g.OverlapHexahedra(queries, k)
                    _assert_rows(got, exp[k], label)
                    blob.update(got[0].tobytes())
                    blob.update(got[1].tobytes())
                    for n in COUNTS:
                        _assert_rows(g.OverlapHexahedra(queries[:n], k), (exp[k][0][:n], exp[k][1][:n]), label + " n=%d" % n)
                for k in (1, 16):
                    _assert_rows(g.OverlapHexahedra(queries, k, after=cursor), exp_after[k], "cursor accel=%d k=%d" % (accel, k))
                if accel:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 0
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_chunk_seams(n_tris):
    """A small box, frustum or segment at each petal's own point touches that petal alone (in the twin layout both twins); a thin
    box down the stack touches every petal of the seam: the last record of a chunk, the first of the next, the last of the
    scene.  One region spans the whole scene."""
    h = 1.0 / 16
    for layout in sc.layouts(n_tris):
        rows, info = sc.seam_scene(n_tris, layout)
        regs, want = [], []
        for S, seam in info["seams"].items():
            tie = seam["tie"]
            for i in seam["members"]:
                if tie and i == tie[1]:
                    continue                                             # record S is the twin of S - 1 here: it has no place of its own
                x, y, z = sc.petal_point(i, S) + (sc.petal_z(i, S),)
                kind = i % 3
                if kind == 0:
                    regs.append(he.box_corners([x - h, y - h, z - h], [x + h, y + h, z + h])[0])
                elif kind == 1:                                          # a small frustum looking down through the point
                    regs.append(np.concatenate([[[x - h / 2, y - h / 2, z + h], [x + h / 2, y - h / 2, z + h], [x - h / 2, y + h / 2, z + h],
                                                 [x + h / 2, y + h / 2, z + h]], [[x - h, y - h, z - h], [x + h, y - h, z - h],
                                                                                 [x - h, y + h, z - h], [x + h, y + h, z - h]]]))
                else:
                    regs.append(he.segments([[x, y, z - h]], [[x, y, z + h]])[0])
                want.append([i, tie[1]] if tie and i == tie[0] else [i])
            cx, cy = seam["centre"]
            regs.append(he.box_corners([cx - h, cy - h, sc.Z0 - h], [cx + h, cy + h, sc.Z0 + 8 * sc.DZ])[0])
            want.append(list(seam["members"]))
        queries = he.queries_of(np.concatenate([np.asarray(regs, f32), he.box_corners([-100, -100, -100], [100, 100, 100])]))
        acc = he.table(queries, rows, spheres=sc.SPHERES)
        for row, w in zip(acc[:-1], want):
            assert np.nonzero(row[:n_tris])[0].tolist() == w             # the helper says what the scene was made for
        assert acc[-1, :n_tris].all() and acc[-1, n_tris:].all()        # every record, and every sphere wholly inside it
        assert any(n_tris - 1 in w for w in want) and (n_tris < 1024 or any(1023 in w for w in want)) and (n_tris < 1025 or any(1024 in w for w in want))
        for edges in (False, True):
            g = _tracer()
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            g.UploadSpheres(sc.SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 1, 4, 16):
                    _assert_rows(g.OverlapHexahedra(queries, k), he.rows_of_table(acc, k), "%d %s edges=%d accel=%d k=%d" % (n_tris, layout, edges, accel, k))
                first = he.rows_of_table(acc, 1)[0][:, 0]
                _assert_rows(g.OverlapHexahedra(queries, 4, after=first), he.rows_of_table(acc, 4, after=first), "behind the first prim")
                assert g.OverlapHexahedra(queries[-1:], 16)[1][0] == n_tris + len(sc.SPHERES)      # counts far above 16
            g.close()


def test_overlap_hexahedra_all_enumerates_a_stack_once_and_the_cursor_edges():
    rows = np.zeros((111, 4), f32)
    rows[0::3, :3], rows[1::3, :3], rows[2::3, :3] = [-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]          # 37 coincident triangles
    spheres = f32([[0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.5, 0.5], [0.0, -0.25, 2.0, 0.25]])
    rod = he.queries_of(he.box_corners([-0.125, -0.125, -1], [0.125, 0.125, 3]))
    queries = np.concatenate([rod, he.regions_near(rows, 30, 5, size=1.0)])
    acc = he.table(queries, rows, spheres=spheres)
    assert acc[0].all() and acc.shape[1] == 40
    sets = he.accepted_sets(acc)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(spheres)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 5, 1):
            prims, offsets = g.OverlapHexahedraAll(queries if k > 1 else queries[:1], k)
            assert prims.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == prims.shape[0]
            assert np.array_equal(prims[offsets[0]:offsets[1]], np.arange(40))      # 0 .. 39, once each, in order
            for i in range(offsets.shape[0] - 1):
                assert np.array_equal(prims[offsets[i]:offsets[i + 1]], sets[i])
        for after, count in ((39, 0), (-1, 40), (5000, 0), (2 ** 31 - 1, 0), (38, 1), (0, 39), (-2, 40), (-2 ** 31, 40)):
            p, c = g.OverlapHexahedra(rod, 4, after=np.int32([after]))
            assert c[0] == count, (after, c)
            first = max(after + 1, 0) if after != -1 else 0
            assert p[0].tolist() == [first + s if s < count else -1 for s in range(4)], (after, p)
    g.close()


@pytest.mark.parametrize("scene", ["random10000", "rooms"])
def test_bvh_equals_scan_byte_for_byte_whatever_the_slack(scene):
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "random10000" else lc.rooms()
    queries = np.concatenate([regions_around(rows, 12000, 1), regions_around(rows, 4384, 2, grow=10.0)])
    if scene == "rooms":                                                 # regions that end ON the lattice's planes
        rng = np.random.default_rng(3)
        lo = np.round(rng.uniform(-2, 2, (2000, 3))) - lc.SHIFT
        queries[:2000] = he.queries_of(he.box_corners(lo, lo + np.round(rng.uniform(0, 2, (2000, 3)))))
    assert queries.shape[0] == 16384
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.OverlapHexahedra(queries, k) for k in (0, 4, 16)}
    assert (scan[16][1] == 0).any() and (scan[16][1] > 16).any()
    _assert_rows(tuple(x[:128] for x in scan[16]), he.expected(queries[:128], rows, 16), "the scan against the helper")
    g.SetQueryAcceleration(True)
    for slack in (1000, 0, 1000000):
        g.DebugQueryAccelSlack(slack)
        for k in (0, 4, 16):
            got = g.OverlapHexahedra(queries, k)
            assert got[0].tobytes() == scan[k][0].tobytes() and got[1].tobytes() == scan[k][1].tobytes(), (scene, slack, k)
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_a_shortened_stack_restarts_list_and_count():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    queries = np.concatenate([regions_around(rows, 400, 3), regions_around(rows, 112, 4, grow=40.0)])
    g = _tracer()
    assert g.UploadScene(rows)
    scan = {k: g.OverlapHexahedra(queries, k) for k in (0, 3, 16)}
    total = scan[0][1]
    assert (total > 16).any() and (total < 16).any() and (total < 3).any()
    _assert_rows(tuple(x[:96] for x in scan[16]), he.expected(queries[:96], rows, 16), "deep scan against the helper")
    g.SetQueryAcceleration(True)
    g.OverlapHexahedra(queries[:1], 0)                                   # builds the tree
    depth = g.QueryAccelInfo()["depth"]
    try:
        for cap in (None, 0, 1, 3, 3 * depth - 1):
            g.DebugQueryStackCap(cap)
            for k in scan:
                _assert_rows(g.OverlapHexahedra(queries, k), scan[k], "deep cap=%r k=%d" % (cap, k))
            cursor = scan[3][0][:, 2].copy()
            g.SetQueryAcceleration(False)
            want = g.OverlapHexahedra(queries, 16, after=cursor)
            g.SetQueryAcceleration(True)
            _assert_rows(g.OverlapHexahedra(queries, 16, after=cursor), want, "deep cap=%r cursor" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")                    # (inf - inf and overflow are what the scene is made of)
def test_non_finite_regions_and_records_empty_scenes_and_spheres_alone():
    rows = he.random_scene(37, 3, span=3.0, edge=0.6).reshape(-1, 3, 4).copy()
    rows[5, 1, 0] = np.nan
    rows[11, 0, 1] = -np.inf
    rows[20, 0, :3], rows[20, 1, :3] = 3.0e38, -3.0e38                   # finite vertices whose edge overflows
    rows[30, 2] = rows[30, 1] = rows[30, 0]                              # a point: a finite record like any other
    rows = rows.reshape(-1, 4)
    p30 = rows[90, :3]
    special = he.queries_of(np.concatenate([he.box_corners([-3.0e38] * 3, [3.0e38] * 3), he.box_corners([-9, -9, -9], [9, 9, 40]),
                                            he.box_corners(p30, p30), he.segments([p30], [p30 + f32(1)])]))
    good = he.regions_near(rows, 1, 9)[0]
    queries = np.concatenate([special, he.bad_queries(good), he.nan_pads(good[None]), good[None], regions_around(rows, 100, 4),
                              he.regions_near(rows, 50, 6, size=6.0)])
    nothing = np.full_like(rows, np.nan)
    for scene, always in ((rows, 2), (nothing, 37)):
        for edges in (False, True):
            r = edge_rows(scene) if edges else scene
            acc = he.table(queries, r, edges=edges, spheres=SPHERES)
            assert not acc[4:76].any() and np.array_equal(acc[76], acc[77])        # a NaN or infinite corner accepts nothing; the pads are not read
            g = _tracer()
            assert (g.UploadSceneEdges(r) if edges else g.UploadScene(r))
            g.UploadSpheres(SPHERES)
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                for k in (0, 4, 16):
                    _assert_rows(g.OverlapHexahedra(queries, k), he.rows_of_table(acc, k), "non-finite edges=%d accel=%d k=%d" % (edges, accel, k))
            info = g.QueryAccelInfo()
            assert info["always_tested"] >= always and (scene is rows or info["nodes"] == 0)
            if scene is rows:
                assert acc[:, :37].any() and not acc[:, 5].any() and not acc[:, 11].any() and acc[2, 30] and acc[3, 30]
            else:
                assert not acc[:, :37].any() and acc[:, 37:39].any()
            g.close()
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        prims, counts = g.OverlapHexahedra(queries, 5)                   # no scene: nothing to touch
        assert prims.shape == (queries.shape[0], 5) and not counts.any() and (prims == -1).all()
        prims, counts = g.OverlapHexahedra(np.zeros((0, 32), f32), 3)
        assert prims.shape == (0, 3) and counts.shape == (0,)
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        ball = he.queries_of(np.concatenate([he.box_corners([-1.0, -1.0, -2.5], [2.0, 2.0, 0.5]),       # the twins wholly inside it
                                             he.box_corners([0.4, 0.2, -1.1], [0.6, 0.4, -0.9])]))      # wholly inside the twins
        q = np.concatenate([ball, queries])
        acc = he.table(q, None, spheres=SPHERES)
        assert acc[0, :2].all() and not acc[1].any() and acc[2:].any()
        for k in KS:
            _assert_rows(g.OverlapHexahedra(q, k), he.rows_of_table(acc, k), "spheres only accel=%d k=%d" % (accel, k))
        g.close()


def test_degenerate_regions_and_segments_against_intersect_all():
    rows = he.random_scene(37, 61, span=1.5, edge=0.8)
    A, B, C = (x.astype(np.float64) for x in he.corners(rows))
    centroid, normal = (A + B + C) / 3, np.cross(B - A, C - A)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    rng = np.random.default_rng(62)
    d = normal + rng.uniform(-0.3, 0.3, normal.shape)
    p, q = (centroid - 1.5 * d).astype(f32), (centroid + 1.5 * d).astype(f32)
    segs = he.queries_of(he.segments(p, q))
    pyramids = he.queries_of(he.frusta(centroid, 63, 0.8, pyramid=True))
    queries = np.concatenate([segs, pyramids])
    acc = he.table(queries, rows)
    g = _tracer()
    assert g.UploadScene(rows)
    crossed = [set() for _ in range(37)]                                 # the ray queries cull back faces: both directions
    for a, b in ((p, q), (q, p)):
        hits, counts = g.IntersectAll(np.c_[a, b - a, np.zeros(37, f32), np.ones(37, f32)].astype(f32), 16)
        assert counts.max() < 16
        for i in range(37):
            crossed[i] |= set(hits["prim"][i, :counts[i]].tolist())
    assert all(i in crossed[i] for i in range(37))
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        _assert_rows(g.OverlapHexahedra(queries, 16), he.rows_of_table(acc, 16), "degenerate accel=%d" % accel)
        prims, offsets = g.OverlapHexahedraAll(segs)
        for i in range(37):
            assert sorted(crossed[i]) == prims[offsets[i]:offsets[i + 1]].tolist(), (accel, i)
    assert acc[np.arange(37), np.arange(37)].all() and acc[37 + np.arange(37), np.arange(37)].all()
    g.close()


def test_aligned_boxes_on_the_eighth_lattice_answer_as_overlap():
    import raytracertest_amd as R
    rows = np.clip(oe.random_scene(400, 5, edge=1.0, span=1.5, snap=0.125), -2, 2)
    rng = np.random.default_rng(6)
    lo = np.round(rng.uniform(-2, 1.5, (600, 3)) * 8) / 8
    hi = np.minimum(lo + np.round(rng.uniform(0, 1.0, (600, 3)) * 8) / 8, 2.0)
    touching, tags = oe.touching_boxes(rows, range(0, 400, 9))
    boxes = np.concatenate([oe.boxes_of(lo, hi), touching[[t[2] for t in tags]]])
    corners = R.RayTracer.box_corners(boxes[:, 0:3], boxes[:, 4:7])
    g = _tracer()
    assert g.UploadScene(rows)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (0, 4, 16):
            want = g.Overlap(boxes, k)
            assert want[1].sum() > 2000
            _assert_rows(g.OverlapHexahedra(corners, k), want, "lattice accel=%d k=%d" % (accel, k))
    g.close()


def test_pixel_frusta_against_pick_on_the_cornell_scene():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    g = _tracer(size=(64, 48))
    assert g.UploadScene(rows)
    xs, ys = np.meshgrid(np.arange(64), np.arange(48))
    pix = np.stack([xs.ravel(), ys.ravel()], axis=1)
    hits, rays = g.Pick(pix, return_rays=True)
    hits, rays = hits.reshape(48, 64), rays.reshape(48, 64, 6)
    assert (hits["prim"] >= 0).any()
    picked = 0
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for (x0, y0, x1, y1), near, far in (((0, 0, 63, 47), 0.0, 10.0), ((10, 8, 30, 40), 0.0, 10.0), ((20, 20, 23, 22), 0.5, 2.5),
                                            ((40, 5, 63, 30), 1.0, 3.0), ((5, 30, 50, 47), 0.0, 2.0), ((31, 23, 33, 25), 0.0, 10.0)):
            corners = g.PixelFrustum(x0, y0, x1, y1, near, far)
            want4 = rays[[y0, y0, y1, y1], [x0, x1, x0, x1]]
            assert np.array_equal(corners, R.RayTracer.frustum_corners(want4, *R.RayTracer.cap_parameters(want4, near, far))[0])
            sel = g.SelectRect(x0, y0, x1, y1, near=near, far=far)
            assert sel.dtype == np.int32 and np.array_equal(sel, np.unique(sel))
            assert np.array_equal(sel, he.accepted_sets(he.table(he.queries_of(corners), rows))[0])
            inner = hits[y0 + 1:y1, x0 + 1:x1]                           # strictly inside: not on the border row or column
            seen = inner["prim"][(inner["prim"] >= 0) & (inner["t"] > near) & (inner["t"] < far)]
            assert set(seen.tolist()) <= set(sel.tolist()), ((x0, y0, x1, y1), near, far, accel)
            picked += seen.size
        # the whole image, far beyond the room: every triangle some pixel's ray meets, in front or hidden
        everything = g.SelectRect(0, 0, 63, 47, far=10.0)
        inner = rays[1:47, 1:63].reshape(-1, 6)
        g.SetQueryAcceleration(False)
        all_hits, counts = g.IntersectAll(np.c_[inner, np.zeros(inner.shape[0], f32), np.full(inner.shape[0], 10.0, f32)].astype(f32), 16)
        met = set(all_hits["prim"][np.arange(16)[None, :] < counts[:, None]].tolist())
        assert counts.max() < 16 and len(met) >= 20 and met <= set(everything.tolist())
    assert picked > 2 * 3000                                             # the rectangles did see the scene
    with pytest.raises(ValueError):
        g.SelectRect(0, 0, 10, 10, far=np.inf)
    with pytest.raises(TypeError):
        g.SelectRect(0, 0, 10, 10)                                       # far is required
    g.close()


def test_argument_errors_leave_the_outputs_untouched_and_corner_forms_agree():
    import raytracertest_amd as R
    rows, queries, acc = _reference(37)
    L = R.api.load_library()
    g = _tracer()
    assert g.UploadScene(rows)
    q = np.ascontiguousarray(queries[:70])
    prims = np.full((70, 4), 77, np.int32)
    cnt = np.full(70, 99, np.uint32)
    assert L.rt_tracer_overlap_hexahedra(g._h, None, None, 70, 4, prims.ctypes.data, cnt.ctypes.data) == 1 and "null" in g.LastError()
    assert L.rt_tracer_overlap_hexahedra(g._h, q.ctypes.data, None, 70, 4, None, cnt.ctypes.data) == 1
    assert L.rt_tracer_overlap_hexahedra(g._h, q.ctypes.data, None, 70, 4, prims.ctypes.data, None) == 1
    assert L.rt_tracer_overlap_hexahedra(g._h, q.ctypes.data, None, 70, 17, prims.ctypes.data, cnt.ctypes.data) == 1 and "max_hits" in g.LastError()
    assert (prims == 77).all() and (cnt == 99).all()
    assert L.rt_tracer_overlap_hexahedra(g._h, None, None, 0, 4, None, None) == 0             # n = 0 is a no-op
    assert L.rt_tracer_overlap_hexahedra(g._h, q.ctypes.data, None, 70, 0, None, cnt.ctypes.data) == 0   # counts only: prims may be NULL
    assert np.array_equal(cnt, acc[:70, :37].sum(axis=1))
    with pytest.raises(ValueError):
        g.OverlapHexahedra(q, 17)
    for bad in (np.zeros((4, 5), f32), f32(1.0), np.zeros((4, 24), f32)):
        with pytest.raises(ValueError):
            g.OverlapHexahedra(bad)
    with pytest.raises(ValueError):
        g.OverlapHexahedra(q, 4, after=np.zeros(3, np.int32))
    want = g.OverlapHexahedra(q, 16)
    c = he.corners_of(q)
    for form in (c, q.reshape(-1, 8, 4), he.nan_pads(q)):
        _assert_rows(g.OverlapHexahedra(form), want, "corner forms")
    g.close()


def test_torch_path_on_a_side_stream_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, queries, acc = _reference(1100)
    n = queries.shape[0]
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(queries)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        for k in (16, 4, 0):
            want = he.rows_of_table(acc, k)
            tp, tc = g.OverlapHexahedra(t, k)
            assert tp.dtype == torch.int32 and tp.shape == (n, k) and tc.dtype == torch.int32 and tc.shape == (n,)
            assert tp.cpu().numpy().tobytes() == want[0].tobytes() and tc.cpu().numpy().tobytes() == want[1].tobytes()
            if k:
                after = tp[:, k - 1].contiguous()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):                               # on the caller's current stream
                    tp2, tc2 = g.OverlapHexahedra(t, k)
                    np_, nc = g.OverlapHexahedra(t, k, after=after)
                s.synchronize()
                assert torch.equal(tp2, tp) and torch.equal(tc2, tc)
                page2 = he.rows_of_table(acc, k, after=want[0][:, k - 1])
                assert np_.cpu().numpy().tobytes() == page2[0].tobytes() and nc.cpu().numpy().tobytes() == page2[1].tobytes()
            tp0, tc0 = g.OverlapHexahedra(t[:0], k)
            assert tp0.shape == (0, k) and tc0.shape == (0,)
    for bad in (t.cpu(), t.double(), t[:, :24].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.OverlapHexahedra(bad, 4)
    cur = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    for bad_after in (cur.cpu(), cur[:-1].contiguous(), cur.float(), np.full(n, -1, np.int32)):
        with pytest.raises(ValueError):
            g.OverlapHexahedra(t, 4, after=bad_after)
    flat = t.reshape(-1)
    out = torch.full((8 * 4,), 77, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((8,), 99, dtype=torch.int32, device="cuda:0")
    P, O, Cn, A = flat.data_ptr(), out.data_ptr(), cnt.data_ptr(), cur.data_ptr()
    for args in ((P + 4, None, 8, 4, O, Cn), (P + 8, A, 8, 4, O, Cn)):   # misaligned corners
        assert L.rt_tracer_overlap_hexahedra_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, None, 8, 4, O, Cn), (P, None, 8, 4, None, Cn), (P, None, 8, 4, O, None), (P, None, 8, 17, O, Cn)):
        assert L.rt_tracer_overlap_hexahedra_device(g._h, *args, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (cnt == 99).all()                       # the outputs are untouched
    assert L.rt_tracer_overlap_hexahedra_device(g._h, None, None, 0, 4, None, None, None) == 0
    assert L.rt_tracer_overlap_hexahedra_device(g._h, P, A, 8, 4, O, Cn, None) == 0
    torch.cuda.synchronize()
    want = he.rows_of_table(acc[:8], 4)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and cnt.cpu().numpy().tobytes() == want[1].tobytes()
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    queries = regions_around(moved, 2048, 9)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.OverlapHexahedra(queries, 16)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    assert g.QueryAccelInfo()["valid"] == 0
    got = {k: g.OverlapHexahedra(queries, k) for k in (16, 4, 0)}        # the first of them refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0 and g.QueryAccelInfo()["valid"] == 1
    g.SetQueryAcceleration(False)
    for k in (16, 4, 0):
        _assert_rows(got[k], g.OverlapHexahedra(queries, k), "after the refit k=%d" % k)
    assert (first[0] != got[16][0]).any()                                # the scene did move
    _assert_rows(tuple(x[:128] for x in got[16]), he.expected(queries[:128], moved, 16), "the moved scene against the helper")
    g.close()


def test_overlap_hexahedra_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    queries = regions_around(rows, 2048, 7)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.OverlapHexahedra(queries, 16)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.OverlapHexahedra(queries, 16 if i % 4 < 2 else 4))
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
    queries = regions_around(rows, 500, 3, grow=0.5)
    acc = he.table(queries, rows)
    exp = he.rows_of_table(acc, 4)
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_rows(one.OverlapHexahedra(queries, 4), exp, "one band against the helper")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_rows(m.OverlapHexahedra(queries, 4), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_rows(m.OverlapHexahedra(queries, 4), exp, "two bands, bvh")
    _assert_rows(m.OverlapHexahedra(queries, 4, after=exp[0][:, 3]), he.rows_of_table(acc, 4, after=exp[0][:, 3]), "two bands, the cursor")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()
