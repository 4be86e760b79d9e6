"""The designed render scenes (tests/render_seam_cases.py) hold what they promise under the oracle alone, without a device:
every cover is hit by every probed ray of every tile, no out by any; the designated winner is the farthest hit wherever the
rival does not reach and the rival beats it where it does; the per-tile candidate counts are the covers plus the partials that
meet the tile; and removing the designated record, or letting the later twin win, changes the oracle's frame at the designated
pixels -- a kernel that skipped that record could not pass tests/test_gpu_render_seams.py."""
import numpy as np
import pytest

import render_seam_cases as rc

CAM = rc.CAMERA
LENS32 = rc.LENS.astype(np.float32)


def _oracle(orc, case, contract=1, row0=0, rows=None, **scene_kw):
    W, H = rc.FRAMES[case["frame"]]
    rows_, edges = rc.scene(case, **scene_kw)
    o = orc.OracleTracer(W, H, CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=3, row0=row0, rows=rows,
                         contract=contract, nthreads=8, smooth_normals=bool(case["options"].get("smooth_normals")))
    assert (o.upload_scene_edges if edges else o.upload_scene)(rows_)
    return o


def _probed_tiles(case):
    """every tile of the frame, thinned out where the scene is large (the corners of the frame stay)"""
    ny, nx = rc.tiles_of(case["frame"])
    tiles = [(tx, ty) for ty in range(ny) for tx in range(nx)]
    keep = max(24, int(4e5 // case["n"]))
    if len(tiles) > keep:
        step = len(tiles) // keep + 1
        tiles = sorted(set(tiles[::step]) | {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)})
    return tiles


def _tile_pixels(case, tx, ty):
    """the tile's 64 pixels; its four corner pixels where the scene is large"""
    W, H = rc.FRAMES[case["frame"]]
    if case["n"] > 1500:
        return [(x, y) for y in (ty * 8, min(ty * 8 + 7, H - 1)) for x in (tx * 8, min(tx * 8 + 7, W - 1))]
    return [(x, y) for y in range(ty * 8, min(ty * 8 + 8, H)) for x in range(tx * 8, min(tx * 8 + 8, W))]


def test_the_table_has_the_sizes_and_positions_the_seams_need():
    assert len(rc.BY_NAME) == len(rc.CASES)
    small = [c for c in rc.CASES if c["group"] == "small"]
    for n in (31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257):
        mine = [c for c in small if c["n"] == n and c["partials"]]
        assert {c["winner"] for c in mine} == {w for w in (0, 63, 64, n - 1) if w < n}, n
    rivals = [(c["winner"], next(i for i, k in c["partials"].items() if k == "rival")) for c in small if c["partials"]]
    for w in (63, 64):                                                # the rival in an earlier and in a later step than the winner
        assert any(a == w and r < 8 for a, r in rivals) and any(a == w and r >= 64 * (w // 64 + 1) for a, r in rivals), w
    assert any(a == 0 and r >= 64 for a, r in rivals) and any(a > 64 and r == 1 for a, r in rivals)
    for n, bl in ((32, 32), (64, 64), (256, 256), (960, 960)):
        c = rc.BY_NAME["small_full_n%d" % n]
        assert c["covers"] == list(range(n)) and c["promise"]["bin_list"] == bl
    assert rc.BY_NAME["small_full_n960"]["winner"] == 959
    assert all(c["promise"]["bin_list"] == 288 and c["options"] == {"bin_list": 288} for c in small if c["n"] == 257)
    assert {len(c["covers"]) for c in small if "cand" in c["name"]} == {4, 5, 8, 9, 16, 17}
    scan = [c for c in rc.CASES if c["group"] == "scan"]
    assert {c["n"] for c in scan} == {1023, 1024, 1025, 2049, 37, 4096, 4097}
    for c in scan:
        ch = c["promise"]["lds_chunk"]
        assert c["options"]["no_binning"] and c["winner"] in (ch - 1, ch, c["n"] - 1) and c["twins"] in (None, ch - 1)
    assert {(c["n"], c["winner"]) for c in scan} >= {(1025, 1023), (1025, 1024), (2049, 2048), (37, 0), (37, 1), (37, 36), (4097, 4095), (4097, 4096)}
    assert {c["n"] for c in scan if c["twins"] is not None} == {1025, 2049, 37, 4097}
    large = {c["name"]: c for c in rc.CASES if c["group"] == "large"}
    assert len(large["large_n1100_block1024"]["covers"]) == 1024 and len(large["large_n1100_block1025"]["covers"]) == 1025
    assert len(large["large_n4096_forms448"]["covers"]) == 448 and len(large["large_n4096_forms449"]["covers"]) == 449
    assert len(large["large_n4096_dense84"]["covers"]) == 84 and len(large["large_n300_macro40"]["covers"]) == 40
    assert len(large["large_n300_macro41"]["covers"]) == 41
    assert {c["n"] for c in large.values() if c["filler"]} == {2047, 2048, 4095, 4096, 50000, 50001, 65536, 65537}
    frames = {c["frame"] for c in rc.CASES}
    assert frames == {"a", "b", "tall", "wide", "column"} and rc.FRAMES["tall"][1] >= 128
    assert all(c["frame"] not in ("wide", "column") or c["n"] in (2047, 2048, 65536, 65537) for c in rc.CASES)
    for f in ("wide", "column"):                                      # more than 4 x 4 macro tiles of 128 x 64: the super level
        assert ((rc.FRAMES[f][0] + 127) // 128) * ((rc.FRAMES[f][1] + 63) // 64) > 16


def test_the_keep_patterns_break_a_round_mid_step():
    """classify()'s rule on the designed keep patterns: the round closes at L - 1 when the next step would overflow"""
    c = rc.BY_NAME["large_n1100_midstep"]
    keep = np.zeros(c["n"], bool); keep[c["covers"]] = True
    assert keep[:192].sum() == 191 and keep[192:256].all()
    assert rc.classify_rounds(keep, 192) == (1025, 6) and rc.classify_rounds(keep[:192], 192) == (191, 1)
    c = rc.BY_NAME["large_n4096_forms449"]
    keep = np.zeros(c["n"], bool); keep[c["covers"]] = True
    assert keep[:128].sum() == 83 and keep[128:192].all()
    cand, rounds = rc.classify_rounds(keep, 84)
    assert (cand, rounds) == (449, 7)                                 # 83 | 64 x 5 | 46 with the outs behind them
    assert rc.classify_rounds(np.ones(1024, bool), 192) == (1024, 6) and rc.classify_rounds(np.ones(448, bool), 84) == (448, 7)
    assert rc.classify_rounds(np.ones(257, bool), 192) == (257, 2) and rc.classify_rounds(np.ones(84, bool), 84) == (84, 1)
    assert rc.classify_rounds(np.zeros(300, bool), 192) == (0, 1)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_case_holds_what_it_promises_under_the_oracle(orc, case):
    n = case["n"]
    o = _oracle(orc, case)
    covers = np.array(case["covers"])
    part = np.array(sorted(case["partials"]), int)
    is_out = np.ones(n, bool)
    is_out[covers] = False
    is_out[part] = False
    lo, hi, clear, status = rc.tile_counts(case)
    depth = rc.depths(case)
    assert len({round(d, 9) for i, (d, _, _) in depth.items() if i != (case["twins"] or -2) + 1}) == len(covers) - (case["twins"] is not None)
    rival = next((i for i, k in case["partials"].items() if k == "rival"), None)
    seen = {"rival_wins": 0, "winner_wins": 0, "edge": 0}
    for tx, ty in _probed_tiles(case):
        probe, nohit = o.tile_probe(_tile_pixels(case, tx, ty), LENS32)
        rays = int(probe["rays"][0])
        assert rays == len(_tile_pixels(case, tx, ty)) * len(LENS32) and nohit == 0
        assert (probe["hits"][covers] == rays).all(), (case["name"], tx, ty, "a cover is missed by some ray")
        if case["filler"] is None:
            assert not probe["hits"][is_out].any(), (case["name"], tx, ty, "an out is hit")
        met = int((probe["hits"] > 0).sum()) if case["filler"] is None else None
        if met is not None:
            least = lo[ty, tx] if n <= 1500 else len(covers)             # (corner pixels alone may miss a partial that reaches the tile)
            assert least <= met <= hi[ty, tx] and (not clear[ty, tx] or met == len(covers)), (case["name"], tx, ty, met)
        for i in part:
            st = status[int(i)][ty, tx]
            assert st == 1 or int(probe["hits"][i]) == (rays if st == 2 else 0), (case["name"], tx, ty, int(i), st)
        w = case["winner"]
        if w is None:
            continue
        first = case["twins"] if case["twins"] is not None else w
        rst = 0 if rival is None else status[rival][ty, tx]
        if rst == 0:                                                   # the designated winner is the farthest hit of every ray
            assert int(probe["wins"][first]) == rays, (case["name"], tx, ty)
            seen["winner_wins"] += 1
        elif rst == 2:                                                 # the rival beats it
            assert int(probe["wins"][rival]) == rays and int(probe["wins"][w]) == 0, (case["name"], tx, ty)
            seen["rival_wins"] += 1
        else:
            seen["edge"] += 0 < int(probe["wins"][rival]) < rays
    if case["winner"] is not None:
        assert seen["winner_wins"] > 0
    if rival is not None and n <= 1500:
        assert seen["rival_wins"] > 0 and seen["edge"] > 0, seen


def _band(case):
    """rows of the frame that a teeth frame renders: all of a small frame, a few of a large one or of a large scene"""
    W, H = rc.FRAMES[case["frame"]]
    rows = H if case["n"] * W * H < 4e8 else max(1, min(H, int(4e8 // (case["n"] * W))))
    return (H - rows) // 2, rows


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_teeth_the_designated_record_decides_the_frame(orc, case):
    r0, rows = _band(case)
    ref = _oracle(orc, case, row0=r0, rows=rows)
    ref.trace(1, 1)
    w = rc.designated(case)
    gone = _oracle(orc, case, row0=r0, rows=rows, without=w)
    gone.trace(1, 1)
    changed = (ref.render.view(np.uint32) != gone.render.view(np.uint32)).any(axis=2)
    assert np.array_equal(ref.rng, gone.rng)
    if case["winner"] is not None:
        # wherever the rival does not reach, the pixel shows the designated record: without it, another colour
        _, _, _, status = rc.tile_counts(case)
        rival = next((i for i, k in case["partials"].items() if k == "rival"), None)
        free = np.ones(changed.shape, bool) if rival is None else np.kron(status[rival] == 0, np.ones((8, 8), bool))[r0:r0 + rows, :changed.shape[1]]
        assert free.any() and changed[free].all(), (case["name"], int(changed[free].sum()), int(free.sum()))
    else:
        assert changed.any(), case["name"]
    if case["twins"] is not None:                                      # the later twin winning: the other normals' colour
        swapped = _oracle(orc, case, row0=r0, rows=rows, swap_twins=True)
        swapped.trace(1, 1)
        assert (ref.render.view(np.uint32) != swapped.render.view(np.uint32)).any(axis=2).all(), case["name"]
