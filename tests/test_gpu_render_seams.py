"""The render kernels on the scene-size seams of their lists (tests/render_seam_cases.py): the small scenes' list builders
(region_pair_lists_kernel | region_lists_kernel | tile_lists_kernel, K = 2 | 4, lists exactly full, the 10-bit header fields, the
certain-winner verdict with the winner and its rival in chosen steps and passes), the full scan's LDS chunks, and the block,
wave, HBM and macro lists of the larger scenes at their capacities.  Every case: render accumulators, sample counts, RNG states
and BGRA8 image bit for bit against the oracle, both arithmetic modes, after one Trace of two iterations and again after a
TraceEnqueue step on the kept lists -- and the readbacks (stored tile lists, rt_tracer_info, the wave lists' counts, the
instrumented launch's counters) show that the case reached its seam."""
import numpy as np
import pytest

import render_seam_cases as rc

pytestmark = pytest.mark.gpu
CAM = rc.CAMERA
SPP = rc.SPP
LDS = {"classify": 4 * 192 * 40 + 1024 * 4 + 160, "forms": 4 * 84 * 104 + 448 * 4 + 160}     # (dense_cases.lds_bytes)
LDS["dense"] = LDS["forms"]
_TILES = {}


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    from raytracertest_amd import api
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return api


def tile_counts(case):
    """(lo, hi, clear, status) of the case's frame and partials: computed once per (frame, kinds), the cover count added"""
    key = (case["frame"], tuple(sorted(case["partials"].values())))
    if key not in _TILES:
        probe = dict(case, covers=[], partials={k: kind for k, kind in enumerate(sorted(case["partials"].values()))})
        lo, hi, clear, status = rc.tile_counts(probe)
        _TILES[key] = (lo, hi, clear, {kind: status[k] for k, kind in probe["partials"].items()})
    lo, hi, clear, by_kind = _TILES[key]
    c = len(case["covers"])
    return lo + c, hi + c, clear, {i: by_kind[kind] for i, kind in case["partials"].items()}


def tracer(rt, case, mode, monkeypatch, seed, **kw):
    W, H = rc.FRAMES[case["frame"]]
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)                                       # (read when the tracer is created)
    opts = dict(case["options"], **kw)
    g = rt.RayTracer((W, H), (0, 0, 0), CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=seed, math_mode=mode, **opts)
    for k in case["env"]:
        monkeypatch.delenv(k)
    rows, edges = rc.scene(case)
    assert (g.UploadSceneEdges if edges else g.UploadScene)(rows)
    return g


def oracle_frames(orc, case, mode, seed, nearest=False, row0=0, rows=None):
    """the oracle's four buffers after trace(2, SPP) and after the trace(1, SPP) behind it"""
    W, H = rc.FRAMES[case["frame"]]
    o = orc.OracleTracer(W, H, CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=seed, row0=row0, rows=rows,
                         contract=1 - mode, nthreads=8, hit_mode=int(nearest), smooth_normals=bool(case["options"].get("smooth_normals")))
    rows_, edges = rc.scene(case)
    assert (o.upload_scene_edges if edges else o.upload_scene)(rows_)
    out = []
    for iters in (2, 1):
        o.trace(iters, SPP)
        out.append(tuple(a.copy() for a in (o.render, o.counts, o.rng, o.image)))
    return out


def buffers(g):
    return g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image()


def render(g):
    """one Trace of two iterations, then a TraceEnqueue step on the lists it kept (a split launch on the tall frames)"""
    g.Trace(2, SPP, 0); assert g.Wait()
    first = buffers(g)
    g.TraceEnqueue(1, SPP); g.Sync()
    return [first, buffers(g)]


def same(what, got, want, row0=0, rows=None):
    for step, (gs, ws) in enumerate(zip(got, want)):
        for name, a, b in zip(("render", "counts", "rng", "image"), gs, ws):
            a = a[row0:row0 + (a.shape[0] if rows is None else rows)]
            d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
            assert d.size == 0, "%s, step %d: %s differs in %d words, first at (row, x, ...) %s" % (what, step, name, d.shape[0], d[0].tolist())


def listed(words, tx, ty):
    w0 = int(words[ty, tx, 0])
    return w0 & 0x3FF, (w0 >> 10) & 0x3FF, bool(w0 >> 31), words[ty, tx, 1:1 + (w0 & 0x3FF)].astype(np.int64)


def check_tile_lists(case, g):
    """the stored lists are the designed ones: length, ascending indices, every cover, the partials that reach the tile; the
    verdict follows from the list: the farthest listed triangle is the certain winner when it is a cover, the rival is certain
    only where every ray meets it, and a listed rival that is not leaves the tile uncertain"""
    ny, nx = rc.tiles_of(case["frame"])
    words = g.DebugTileListWords()
    prom = case["promise"]
    assert words.shape == (ny, (rc.FRAMES[case["frame"]][0] + 31) // 32 * 4, 1 + prom["bin_list"]), words.shape
    assert not (words[:, nx:, 0] & 0x3FF).any(), "a slot right of the image has a list"
    lo, hi, clear, status = tile_counts(case)
    covers = np.array(case["covers"])
    rival = next((i for i, k in case["partials"].items() if k == "rival"), None)
    certain_tiles = 0
    for ty in range(ny):
        for tx in range(nx):
            count, winner, certain, lst = listed(words, tx, ty)
            where = (case["name"], tx, ty, count, winner, certain)
            assert lo[ty, tx] <= count <= hi[ty, tx] and (not clear[ty, tx] or count == covers.size), where
            assert (np.diff(lst) > 0).all() and np.isin(covers, lst).all() and np.isin(lst, list(covers) + list(case["partials"])).all(), where
            for i, st in status.items():
                assert st[ty, tx] == 0 or i in lst, where + (i, "a partial that rays of the tile meet is not listed")
            if rival is not None and rival in lst:
                assert not certain or (winner == rival and status[rival][ty, tx] == 2), where
            else:
                assert certain and winner == case["winner"], where
            certain_tiles += certain
    if prom.get("full"):
        assert (words[:, :nx, 0] & 0x3FF).max() == prom["bin_list"] == case["n"]
    if rival is not None:
        assert 0 < certain_tiles < nx * ny, "the frame does not mix traced and certain-winner tiles"
    return words


def check_stats_against_lists(case, g, words):
    """tiles_by_list of the instrumented launch is what the stored lists say (slots right of the image: empty lists)"""
    ny, nx = rc.tiles_of(case["frame"])
    st = g.TraceStats(SPP)
    w0 = words[:, :, 0]
    count, certain = (w0 & 0x3FF).astype(int), (w0 >> 31) != 0
    want = {"sure": int(certain.sum()), "0": int(((count == 0) & ~certain).sum()), "1": int(((count == 1) & ~certain).sum()),
            "2": int(((count == 2) & ~certain).sum()), "more": int(((count > 2) & ~certain).sum())}
    assert st["tiles_by_list"] == want, (case["name"], st, want)
    assert st["bin_candidates"] == int(count.sum()) and st["bin_rounds"] == count.size, (case["name"], st)


SMALL = [c for c in rc.CASES if c["group"] == "small"]
SCAN = [c for c in rc.CASES if c["group"] == "scan"]
LARGE = [c for c in rc.CASES if c["group"] == "large"]


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_small_scene_lists_at_their_seams(rt, orc, monkeypatch, case):
    k = SMALL.index(case)
    seed = 101 + k
    for mode in (0, 1):
        want = oracle_frames(orc, case, mode, seed)
        g = tracer(rt, case, mode, monkeypatch, seed)
        same("%s mode %d" % (case["name"], mode), render(g), want)
        info = g.Info()
        assert info["samples_in_flight"] == case["promise"]["k"] and info["n_tris"] == case["n"], info
        words = check_tile_lists(case, g)
        if mode == 0:
            check_stats_against_lists(case, g, words)
        g.close()
        if mode == k % 2:                                              # the same lists, the verdicts unused
            h = tracer(rt, case, mode, monkeypatch, seed, no_sure_hit=True)
            same("%s mode %d no_sure_hit" % (case["name"], mode), render(h), want)
            assert h.TraceStats(SPP)["tiles_by_list"]["sure"] == 0
            h.close()
    if case["nearest"]:
        g = tracer(rt, case, 0, monkeypatch, seed, nearest_hit=True)
        same(case["name"] + " nearest", render(g), oracle_frames(orc, case, 0, seed, nearest=True))
        g.close()


@pytest.mark.parametrize("case", SCAN, ids=[c["name"] for c in SCAN])
def test_full_scan_chunks_at_their_seams(rt, orc, monkeypatch, case):
    seed = 301 + SCAN.index(case)
    prom = case["promise"]
    for mode in (0, 1):
        g = tracer(rt, case, mode, monkeypatch, seed)
        same("%s mode %d" % (case["name"], mode), render(g), oracle_frames(orc, case, mode, seed))
        info = g.Info()
        assert (info["lds_chunk"], info["lds_bytes"], info["samples_in_flight"]) == (prom["lds_chunk"], prom["lds_bytes"], prom["k"]), info
        g.close()
    if case["nearest"]:
        g = tracer(rt, case, 1, monkeypatch, seed, nearest_hit=True)
        same(case["name"] + " nearest", render(g), oracle_frames(orc, case, 1, seed, nearest=True))
        g.close()


def bands_of(case, mode):
    """the row bands the oracle renders where the whole frame would cost more than about 1e9 ray-triangle tests"""
    if not case["promise"].get("bands"):
        return [(0, None)]
    if case["frame"] == "wide":                                        # across the split row of the enqueued launch (168)
        return [(160, 16)]
    if case["frame"] == "column":                                      # the same (264)
        return [(260, 8)]
    return [(16, 8)]


def wave_walk(case):
    """(first round, (candidates, rounds) of one walk) of a wave over what the levels above leave it: the compacted block list,
    or -- when that overflowed -- the macro tile's list (the covers) or, without macro lists, the scene"""
    prom, n = case["promise"], case["n"]
    L, Lb = (84, 448) if prom["path"] == "forms" else (192, 1024)
    keep = np.zeros(n, bool)
    keep[case["covers"]] = True
    if keep.sum() <= Lb or not case["options"].get("no_macro_bins"):
        keep = np.ones(int(keep.sum()), bool)
    first = rc.classify_walk(keep, L)[0]
    return first, rc.classify_rounds(keep, L)


def check_classify_stats(case, g):
    """bin_candidates / bin_rounds of the instrumented launch are what classify()'s rule yields for the designed keep pattern
    in every wave: no out reached the wave level, and a step that does not fit opened the next round"""
    ny, nx = rc.tiles_of(case["frame"])
    assert nx % 4 == 0, "every wave of the launch has pixels"
    st = g.TraceStats(SPP)
    batches = (SPP + 3) // 4
    first, (cand, rounds) = wave_walk(case)
    if rounds == 1:
        per_wave = (cand, 1)
    elif case["promise"]["path"] == "forms":                           # one classification with forms ahead of the sample loop
        per_wave = (first + batches * cand, 1 + batches * rounds)
    else:
        per_wave = (batches * cand, batches * rounds)
    assert (st["bin_candidates"], st["bin_rounds"]) == (nx * ny * per_wave[0], nx * ny * per_wave[1]), (case["name"], st, per_wave)


@pytest.mark.parametrize("case", LARGE, ids=[c["name"] for c in LARGE])
def test_larger_scene_lists_at_their_seams(rt, orc, monkeypatch, case):
    seed = 501 + LARGE.index(case)
    prom = case["promise"]
    ny, nx = rc.tiles_of(case["frame"])
    W, H = rc.FRAMES[case["frame"]]
    for mode in (0, 1):
        g = tracer(rt, case, mode, monkeypatch, seed)
        got = render(g)
        what = "%s mode %d" % (case["name"], mode)
        for row0, rows in bands_of(case, mode):
            same(what, got, oracle_frames(orc, case, mode, seed, row0=row0, rows=rows), row0, rows)
        if prom.get("bands"):                                          # the whole frame against the full scan
            f = tracer(rt, case, mode, monkeypatch, seed, no_binning=True)
            same(what + " against no_binning", got, render(f))
            f.close()
        info = g.Info()
        assert (info["samples_in_flight"], info["lds_bytes"], info["n_tris"]) == (4, LDS[prom["path"]], case["n"]), info
        if prom["path"] == "dense":
            counts, cap = g.DebugWaveListCounts(0)
            assert cap == 84 and counts.size == (W + 31) // 32 * 4 * ny
            counts = counts.reshape(ny, -1)[:, :nx].astype(np.int64)
            if prom.get("wave_full"):                                  # count == wave_cap fits; one more is the overflow mark
                lo, hi, clear, status = tile_counts(case)
                over = counts == rc.NO_LIST
                assert (counts[~over] == 84).all() and (over | (lo <= 84)).all() and (~over | (hi > 84)).all(), (what, counts)
                assert over.any() == bool(case["partials"]) and not over.all()
            else:
                assert (counts[counts != rc.NO_LIST] <= 84).all() and (counts > 0).any()
        else:
            with pytest.raises(rt.RtError, match="no wave lists"):
                g.DebugWaveListCounts(0)
        if prom.get("stats") and mode == 0:
            check_classify_stats(case, g)
        g.close()
    if case["nearest"]:
        g = tracer(rt, case, 0, monkeypatch, seed, nearest_hit=True)
        got = render(g)
        for row0, rows in bands_of(case, 0):
            same(case["name"] + " nearest", got, oracle_frames(orc, case, 0, seed, nearest=True, row0=row0, rows=rows), row0, rows)
        g.close()
