"""seam_cases.py under the oracle and the numpy restatements, without a device: for every size and both arithmetic contracts
each designated record -- the last of a chunk, the first of the next, the last of the scene -- is its ray's, segment's or point's
unique answer or exact tie, so test_gpu_query_seams.py aims where it says; and a reference that loses such a record, or lets
the later record keep a tie, answers the targeted populations differently, so a kernel that does either cannot pass there.
The same for the sweeps and query triangles of SphereCast and TriangleDistance, against spherecast_expect and tridistance_expect."""
import numpy as np
import pytest

import closest_expect as ce
import exposure_expect as ee
import nearest_expect as ne
import seam_cases as sc
from allhits_expect import expected_all_hits, hit_table_uv, same_rows
from occluded_expect import expected_occluded, in_interval
from query_expect import expected_hits, same_hits

_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case(orc, n_tris, contract):
    """The stack layout's scene, its populations and the oracle's table of the distinct rays, once per session."""
    key = (n_tris, contract)
    if key not in _cache:
        rows, info = sc.seam_scene(n_tris)
        rays, tags = sc.distinct_rays(n_tris, rows)
        _cache[key] = {"rows": rows, "info": info, "rays": rays, "tags": tags, "table": hit_table_uv(orc, rays, rows, None, contract)}
    return _cache[key]


def contracts(orc):
    return (orc.FMA, orc.STRICT)


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_scene_is_what_it_says(n_tris):
    rows, info = sc.seam_scene(n_tris)
    t = rows.reshape(-1, 3, 4)
    assert t.shape[0] == n_tris and info["last"] in info["seam_of"] and not t[:, :, 3].any()
    petals = sorted(info["seam_of"])
    assert petals == [i for S in sc.SEAMS for i in range(S - 4, S + 4) if i < n_tris]
    filler = np.setdiff1d(np.arange(n_tris), petals)
    assert (t[filler, :, 0] < -2.0).all() and (t[petals, :, 0] > 3.0).all()
    assert sc.layouts(n_tris) == (("stack", "tie") if n_tris > 1024 else ("stack",))
    assert info["applies"] == {"tie": False, "stack": True, "cut": n_tris >= 2048, "last": True}
    tie_rows, tie_info = sc.seam_scene(n_tris, "tie")
    differ = np.nonzero((_bits(tie_rows).reshape(n_tris, -1) != _bits(rows).reshape(n_tris, -1)).any(axis=1))[0]
    assert differ.tolist() == [S for S in sc.SEAMS if S < n_tris]        # one record per seam, nothing else
    for S in differ:
        assert tie_info["seams"][S]["tie"] == (S - 1, S) and tie_rows.reshape(-1, 12)[S].tobytes() == rows.reshape(-1, 12)[S - 1].tobytes()
    assert tie_info["applies"]["tie"] == (n_tris > 1024) and tie_info["applies"]["last"] == (n_tris - 1 not in sc.SEAMS)
    # every batch spans blocks and ends in a partial wave; the late-finisher batch is whole blocks for K = 1, 2, 4
    rays, idx, distinct, tags = sc.ray_batch(n_tris, rows)
    segs, sidx, stags = sc.segment_batch(n_tris, rows)
    pts, ptags = sc.point_batch(n_tris, rows)
    for n in (sc.N_RAYS, rays.shape[0], segs.shape[0], pts.shape[0]):
        assert n > 256 and n % 64 != 0
    assert set(idx[:sc.N_RAYS]) == set(range(distinct.shape[0])) and len(stags) == segs.shape[0] and len(ptags) == pts.shape[0]
    assert np.array_equal(_bits(segs[:, :6]), _bits(distinct[sidx]))
    assert sc.late_finisher(n_tris, rows, 300)[0].shape == (sc.LATE, 8) and sc.LATE % (256 * 4) == 0
    bad = ~np.isfinite(distinct).all(axis=1) | ~distinct[:, 3:].any(axis=1)
    assert bad.sum() >= 19                                               # NaN, inf and zero-direction lanes ride along


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_every_targeted_ray_has_its_designated_winner(orc, n_tris):
    for contract in contracts(orc):
        c = case(orc, n_tris, contract)
        rows, info, rays, tags, table = c["rows"], c["info"], c["rays"], c["tags"], c["table"]
        hit, t = table[0], table[1]
        exp = {nearest: expected_hits(orc, rays, rows, None, contract, nearest) for nearest in (False, True)}
        for nearest in (False, True):                                    # the fold over the table IS the reference's scan
            assert same_hits(sc.winners(table, nearest), exp[nearest])
        far, near = exp[False], exp[True]
        for j, (kind, S, i) in enumerate(tags):
            if kind in ("front", "centroid", "behind"):
                assert np.nonzero(hit[j])[0].tolist() == [i], (n_tris, kind, i)      # isolated: the brute force finds nothing else
                assert far["prim"][j] == i and far["t"][j] == t[j, i]
                z = sc.petal_z(i, S)
                if kind == "behind":
                    assert t[j, i] == np.float32(sc.BELOW - z) < 0 and near["prim"][j] == -1
                else:
                    assert t[j, i] == np.float32(-z / (2.0 if kind == "centroid" else 1.0)) and near["prim"][j] == i
            elif kind.startswith("stack"):
                m = sc.members(n_tris, S)
                assert np.nonzero(hit[j])[0].tolist() == m
                ts = t[j, m]
                assert (np.diff(ts) < 0).all() and np.unique(ts).size == len(m)              # distinct, descending in index
                assert ts.tolist() == [(sc.ABOVE if kind == "stack_front" else sc.BELOW) - sc.petal_z(i, S) for i in m]
                assert far["prim"][j] == m[0]                                                 # the largest t: the lowest index
                assert near["prim"][j] == (m[-1] if kind == "stack_front" else -1)
        last = info["last"]
        assert {(k, i) for k, _, i in tags if i == last} == {("front", last), ("behind", last), ("centroid", last)}
        # the tie layout: the same rays; record S is record S - 1 again
        if "tie" in sc.layouts(n_tris):
            tie_rows, tie_info = sc.seam_scene(n_tris, "tie")
            tt = sc.tie_table(table, tie_info)
            for S in (s for s in sc.SEAMS if s < n_tris):
                pair = [j for j, (kind, s, i) in enumerate(tags) if s == S and (i == S - 1 or kind.startswith("stack"))]
                assert len(pair) == 5
                direct = hit_table_uv(orc, rays[pair], tie_rows, None, contract)         # the oracle itself on the twins
                assert all(np.array_equal(_bits(a), _bits(b[pair])) for a, b in zip(direct[1:], tt[1:])) and np.array_equal(direct[0], tt[0][pair])
                for r, j in enumerate(pair):
                    assert direct[0][r, S - 1] and direct[0][r, S]
                    assert _bits(direct[1][r, S - 1:S]) == _bits(direct[1][r, S:S + 1])      # a tie bit for bit
                    if tags[j][0] in ("front", "centroid", "behind"):
                        assert np.nonzero(direct[0][r])[0].tolist() == [S - 1, S]
                vacated = sc.find(tags, "front", S, S)
                assert len(vacated) == 1 and not tt[0][vacated[0]].any()
            for nearest in (False, True):
                w = sc.winners(tt, nearest)
                if contract == orc.FMA:                                                  # (the fold again, on the twins' scene)
                    assert same_hits(w, expected_hits(orc, rays, tie_rows, None, contract, nearest))
                high = sc.winners(tt, nearest, tie_high=True)
                for S in (s for s in sc.SEAMS if s < n_tris):
                    for j in sc.find(tags, "front", S, S - 1) + sc.find(tags, "centroid", S, S - 1):
                        assert w["prim"][j] == S - 1 and high["prim"][j] == S            # teeth: the later record must not win
                    j = sc.find(tags, "behind", S, S - 1)[0]
                    assert (w["prim"][j], high["prim"][j]) == ((-1, -1) if nearest else (S - 1, S))
        # teeth: a scan that loses the first record of the second chunk, or the scene's last, answers differently
        for lost in {last} | ({sc.CHUNK} if n_tris > sc.CHUNK else set()):
            S = info["seam_of"][lost]
            for nearest in (False, True):
                w = sc.winners(table, nearest, drop={lost})
                for j in sc.find(tags, "front", S, lost) + sc.find(tags, "centroid", S, lost):
                    assert exp[nearest]["prim"][j] == lost and w["prim"][j] == -1
            if lost == sc.members(n_tris, S)[-1]:                        # the highest petal: the stack ray's nearest hit
                j = sc.find(tags, "stack_front", S)[0]
                assert near["prim"][j] == lost and sc.winners(table, True, drop={lost})["prim"][j] == lost - 1


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_segments_cut_where_they_say(orc, n_tris):
    for contract in contracts(orc):
        c = case(orc, n_tris, contract)
        rows, info, table = c["rows"], c["info"], c["table"]
        segs, idx, tags = sc.segment_batch(n_tris, rows)
        inside = in_interval(segs, (table[0][idx], table[1][idx]))
        seen = set()
        for j, (kind, S, i) in enumerate(tags):
            got = np.nonzero(inside[j])[0].tolist()
            m = sc.members(n_tris, S) if S else []
            if kind == "only_last":
                assert got == [info["last"]] == [i]
            elif kind == "far_half":
                assert got == [x for x in m if x < S] and len(got) >= 3
            elif kind == "near_half":
                assert got == [x for x in m if x >= S] and got
            elif kind == "closed_tie":
                assert got == [i] and segs[j, 6] == segs[j, 7] == table[1][idx[j], i]        # closed exactly at the t
            elif kind == "dead":
                assert got == [] and not segs[j, 6] <= segs[j, 7]
            seen.add(kind)
        assert seen >= {"turns", "only_last", "far_half", "closed_tie", "dead"} and (("near_half" in seen) == (n_tris > 1024))
        exp = expected_occluded(orc, segs, rows, None, contract, (table[0][idx], table[1][idx]))
        assert exp.any() and not exp.all()
        # the sorted lists: a stack's row holds its petals in ascending t = descending index; four hits cut on the seam
        rows16 = expected_all_hits(table, segs, 16, idx)
        rows4 = expected_all_hits(table, segs, 4, idx)
        for j, (kind, S, i) in enumerate(tags):
            if kind == "turns" and c["tags"][idx[j]][0] == "stack_front" and segs[j, 7] == np.inf:
                m = sc.members(n_tris, S)
                assert rows16[1][j] == len(m) and rows16[0]["prim"][j, :len(m)].tolist() == m[::-1]
                assert (np.diff(rows16[0]["t"][j, :len(m)]) > 0).all()
                if len(m) == 8:
                    assert rows4[0]["prim"][j].tolist() == [S + 3, S + 2, S + 1, S]           # the second chunk's, all of them
                seen.add("row")
        assert "row" in seen
        # the late finisher: one segment that only the last record occludes, 1023 that a record of the first chunk does
        for position in (300, 0, sc.LATE - 1):
            late, lidx = sc.late_finisher(n_tris, rows, position)
            ins = in_interval(late, (table[0][lidx], table[1][lidx]))
            assert (ins.sum(axis=1) == 1).all()
            who = ins.argmax(axis=1)
            odd = np.nonzero(who == info["last"])[0]
            assert odd.tolist() == [position] and (np.delete(who, position) < min(sc.CHUNK, info["last"])).all()
            want = expected_occluded(orc, late, rows, None, contract, (table[0][lidx], table[1][lidx]))
            lost = sc.drop_columns(table, {info["last"]})                # teeth: a block that leaves one chunk (or record) early
            less = expected_occluded(orc, late, rows, None, contract, (lost[0][lidx], lost[1][lidx]))
            assert want.all() and np.nonzero(want != less)[0].tolist() == [position]
        early, eidx = sc.late_finisher(n_tris, rows)
        ins = in_interval(early, (table[0][eidx], table[1][eidx]))
        assert (ins.sum(axis=1) == 1).all() and (ins.argmax(axis=1) < min(sc.CHUNK, info["last"])).all()
        # teeth for the lists: without record 1024 (or the last) the stack rows change
        lost = sc.drop_columns(table, {sc.CHUNK if n_tris > sc.CHUNK else info["last"]})
        assert not same_rows(expected_all_hits(lost, segs, 4, idx), rows4) and not same_rows(expected_all_hits(lost, segs, 16, idx), rows16)
        if "tie" in sc.layouts(n_tris):                                  # the twins: adjacent in a row, the lower index first
            tt = sc.tie_table(table, sc.seam_scene(n_tris, "tie")[1])
            tie16 = expected_all_hits(tt, segs, 16, idx)
            pairs = 0
            for j, (kind, S, i) in enumerate(tags):
                if kind == "closed_tie" and i == S - 1 and S < n_tris:
                    assert tie16[1][j] == 2 and tie16[0]["prim"][j, :2].tolist() == [S - 1, S]
                    assert tie16[0]["t"][j, 0] == tie16[0]["t"][j, 1] == segs[j, 6]
                    pairs += 1
                if kind == "turns" and c["tags"][idx[j]][0] == "stack_front" and segs[j, 7] == np.inf and S < n_tris:
                    p = tie16[0]["prim"][j, :tie16[1][j]].tolist()
                    assert p.index(S) == p.index(S - 1) + 1
            assert pairs >= 2


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_every_targeted_point_has_its_designated_answer(n_tris):
    rows, info = sc.seam_scene(n_tris)
    pts, tags = sc.point_batch(n_tris, rows)
    for layout in sc.layouts(n_tris):
        lrows, linfo = sc.seam_scene(n_tris, layout)
        twins = {S: s["tie"] for S, s in linfo["seams"].items() if s["tie"]}
        for edges in (False, True):
            tab = ce.table(pts, sc.edge_rows(lrows) if edges else lrows, edges)
            t = tab[0]
            exp = ce.winners(tab, pts[:, 3])
            rows16 = ne.expected_all(tab, pts[:, 3], 16)
            seen = set()
            for j, (kind, S, i) in enumerate(tags):
                order = np.argsort(t[j], kind="stable")
                if kind in ("near", "under"):
                    if S in twins and i in twins[S]:                     # equal t for exactly the pair (the twin's own place is empty)
                        if i == S - 1:
                            assert order[:2].tolist() == [S - 1, S] and _bits(t[j, S - 1:S]) == _bits(t[j, S:S + 1]) and t[j, order[1]] < t[j, order[2]]
                            assert exp["prim"][j] == S - 1 and rows16[0]["prim"][j, :2].tolist() == [S - 1, S]
                            seen.add("pair")
                    else:
                        assert order[0] == i == exp["prim"][j] and t[j, i] < t[j, order[1]]          # the unique minimum
                        assert t[j, i] == np.float32(0.0625) ** 2
                elif kind == "fourth" and not (S in twins):
                    four = [S + 3, S + 2, S + 1, S] if i == S else [S - 4, S - 3, S - 2, S - 1]
                    assert rows16[1][j] == 4 and rows16[0]["prim"][j, :4].tolist() == four
                    assert rows16[0]["t"][j, 3] == pts[j, 3] and exp["prim"][j] == four[0]            # closed: the 4th is accepted
                    seen.add("fourth")
                elif kind in ("nan", "negative"):
                    assert exp["prim"][j] == -1 and rows16[1][j] == 0
                elif kind == "beside" and not twins:
                    assert exp["prim"][j] in sc.members(n_tris, S)
            assert ("pair" in seen) == bool(twins) and ("fourth" in seen) == linfo["applies"]["cut"]
            # the cursor on a twin pair's first record: the continuation starts with the twin
            after = sc.tie_cursor(pts, tags, exp)
            cont = ne.expected_all(tab, pts[:, 3], 4, after)
            for j, (kind, S, i) in enumerate(tags):
                if kind in ("near", "under") and i == S - 1:
                    assert after["prim"][j] == S - 1
                    assert cont[0]["prim"][j, 0] != S - 1
                    if S in twins:
                        assert cont[0]["prim"][j, 0] == S and _bits(cont[0]["t"][j, :1]) == _bits(after["t"][j:j + 1])
            # teeth: a scan without record 1024 (or the last one) has another nearest primitive for that record's points
            lost = sc.CHUNK if n_tris > sc.CHUNK else info["last"]
            less = ce.winners(tuple(np.delete(x, lost, axis=1) for x in tab), pts[:, 3])
            changed = np.nonzero(less["t"] != exp["t"])[0]
            if layout == "stack":
                assert changed.size and all(tags[j][2] == lost or tags[j][0] in ("beside", "fourth", "general") for j in changed)
                assert {j for j, tg in enumerate(tags) if tg[0] == "near" and tg[2] == lost} <= set(changed.tolist())
            # ... and one that lets the later twin win names another primitive, bit-equal t or not
            if twins:
                flipped = ce.winners(tuple(x[:, ::-1] for x in tab), pts[:, 3])
                high = t.shape[1] - 1 - flipped["prim"]
                tied = [j for j, tg in enumerate(tags) if tg[0] in ("near", "under") and tg[2] == tg[1] - 1 and tg[1] in twins]
                assert tied and all(high[j] == tags[j][1] and exp["prim"][j] == tags[j][1] - 1 for j in tied)


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_the_exposure_points_see_the_last_record_and_the_sky(orc, n_tris):
    from raytracertest_amd import api
    dirs = ee.as_dirs4(api.hemisphere_directions(64))
    pts = sc.exposure_points(n_tris)
    assert pts.shape == (5, 8) and np.array_equal(pts[0], pts[4])
    rows, info = sc.seam_scene(n_tris)
    segs = ee.exposure_segments(pts[:4], dirs)
    for contract in contracts(orc):
        table = hit_table_uv(orc, segs, rows, None, contract)
        inside = in_interval(segs, (table[0], table[1])).reshape(4, 64, -1)
        blocked = inside.any(axis=2)
        only_last = inside[0, :, info["last"]] & (inside[0].sum(axis=1) == 1)
        assert only_last.any() and (~blocked[0]).any()                   # a bit that only the last record clears, and an open one
        assert blocked[0, 0] and blocked[1, 0]                           # n_dirs = 1: both waves finish, one of them in the last chunk
        assert (inside[1].argmax(axis=1)[blocked[1]] < sc.CHUNK).all()   # point 1 finishes in the first chunk or never
        assert blocked[2].any() and 0 < blocked.sum() < blocked.size
        lost = sc.drop_columns(table, {info["last"]})                    # teeth
        masks = ee.pack_masks(~blocked)
        less = ee.pack_masks(~in_interval(segs, (lost[0], lost[1])).any(axis=1).reshape(4, 64))
        assert masks[0] != less[0] and ee.popcount(less[:1])[0] - ee.popcount(masks[:1])[0] == only_last.sum()


# ---- sweeps and query triangles -------------------------------------------------------------------------------------------

def _same_tables(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def _seam_records(n_tris):
    """The records whose loss the targeted rows must notice: S - 1 and S of every seam, as far as the scene has them, and the
    scene's last."""
    return sorted({i for S in sc.SEAMS for i in (S - 1, S) if i < n_tris} | {n_tris - 1})


def _check_named(tags, prim, t, linfo, label):
    """Every targeted row against its tag under one layout -> the rows aimed at a twin pair's first record.  On the tie layout
    the twin's own place is empty (a sweep finds nothing, a query triangle its neighbour), a row aimed at S - 1 answers S - 1,
    and a stack whose highest petal was record S has S - 1 on top."""
    twins = {S: s["tie"] for S, s in linfo["seams"].items() if s["tie"]}
    pair_rows = []
    for j, (kind, S, i) in enumerate(tags):
        if kind == "general":
            continue
        if S in twins and i == S:                                        # aimed at the record that moved away
            if kind in ("down", "up", "start", "cut"):
                assert prim[j] == -1, (label, kind, i, prim[j])
            elif kind in ("axis_down", "beside"):
                assert prim[j] == S - 1, (label, kind, i, prim[j])
                pair_rows.append(j)
            elif kind == "near":
                assert prim[j] not in (-1, S), (label, kind, i, prim[j])
            continue
        assert prim[j] == i, (label, kind, S, i, prim[j])
        if S in twins and i == S - 1:
            pair_rows.append(j)
    for j in pair_rows:
        S = tags[j][1]
        assert prim[j] == S - 1 and _bits(t[j, S - 1:S]) == _bits(t[j, S:S + 1]) and np.isfinite(t[j, S]), (label, tags[j])
    return pair_rows


def _check_reach(tags, prim, n_tris):
    aimed = {int(prim[j]) for j, tg in enumerate(tags) if tg[0] != "general"}
    assert n_tris - 1 in aimed and (n_tris < 1024 or 1023 in aimed) and (n_tris < 1025 or 1024 in aimed), (n_tris, sorted(aimed))


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_every_targeted_sweep_has_its_designated_contact(n_tris):
    rows, info = sc.seam_scene(n_tris)
    sw, tags = sc.sweep_batch(n_tris, rows)
    assert sw.shape[0] > 256 and sw.shape[0] % 64 != 0 and len(tags) == sw.shape[0]
    aimed = np.array([tg[0] != "general" for tg in tags])
    kinds = {tg[0] for tg in tags}
    assert kinds == {"down", "up", "start", "axis_down", "axis_up", "cut", "bad", "general"}
    tab = sc.sweep_table(sw, rows)
    exp = sc.sweep_winners(tab, sw)
    assert ce.same_hits(exp, sc.spe.expected(sw, rows))
    _check_named(tags, exp["prim"], tab[0], info, (n_tris, "stack"))
    _check_reach(tags, exp["prim"], n_tris)
    r = np.float32(sc.SWEEP_R)
    for j, (kind, S, i) in enumerate(tags):                              # the exact t of the dyadic sweeps
        if kind == "down":
            assert exp["t"][j] == np.float32(sc.ABOVE - sc.petal_z(i, S)) - r and np.isinf(np.delete(tab[0][j], i)).all()
        elif kind == "up":
            assert exp["t"][j] == np.float32(sc.petal_z(i, S) - sc.BELOW) - r and np.isinf(np.delete(tab[0][j], i)).all()
        elif kind == "start":
            assert exp["t"][j] == 0 and (np.delete(tab[0][j], i) > 0).all()
        elif kind == "cut" and i >= 0:
            assert exp["t"][j] == sw[j, 7]
        elif kind in ("axis_down", "axis_up"):
            m = sc.members(n_tris, S)
            assert np.nonzero(np.isfinite(tab[0][j]))[0].tolist() == m and np.unique(tab[0][j, m]).size == len(m)
    # teeth: a scan that loses a record beside a seam, or the scene's last, answers targeted sweeps differently
    for lost in _seam_records(n_tris):
        less = sc.sweep_winners(tab, sw, drop={lost})
        changed = set(ce.differing(less, exp).tolist())
        mine = {j for j, tg in enumerate(tags) if tg[0] != "general" and tg[2] == lost}
        assert mine and mine <= changed, (n_tris, lost)
        assert all(less["prim"][j] != lost for j in mine)
    for layout in sc.layouts(n_tris)[1:]:                                # the twins
        lrows, linfo = sc.seam_scene(n_tris, layout)
        tt = sc.tie_table(tab, linfo)
        assert _same_tables([x[aimed] for x in tt], sc.sweep_table(sw[aimed], lrows))    # the restatement itself on the twins' scene
        w = sc.sweep_winners(tt, sw)
        pair_rows = _check_named(tags, w["prim"], tt[0], linfo, (n_tris, layout))
        assert {tags[j][0] for j in pair_rows} >= {"down", "up", "start"}
        high = sc.sweep_winners(tt, sw, tie_high=True)                   # teeth: the later record must not win
        assert all(high["prim"][j] == tags[j][1] for j in pair_rows)
        assert (high["prim"][aimed] != w["prim"][aimed]).sum() == len(pair_rows)


@pytest.mark.parametrize("n_tris", sc.SIZES)
def test_every_targeted_query_triangle_has_its_designated_answer(n_tris):
    rows, info = sc.seam_scene(n_tris)
    q, tags = sc.triangle_batch(n_tris, rows)
    assert q.shape[0] > 256 and q.shape[0] % 64 != 0 and len(tags) == q.shape[0]
    aimed = np.array([tg[0] != "general" for tg in tags])
    kinds = {tg[0] for tg in tags}
    assert kinds == {"near", "beside", "nan", "negative", "general"} | {k for k, n in (("under", 1024), ("fourth", 2048)) if n_tris >= n}
    tab = sc.triangle_table(q, rows)
    exp = sc.triangle_winners(tab, q[:, 3])
    assert sc.tde.same(exp, sc.tde.expected(q, rows))
    hits = exp[0]
    _check_named(tags, hits["prim"], tab[0], info, (n_tris, "stack"))
    _check_reach(tags, hits["prim"], n_tris)
    for j, (kind, S, i) in enumerate(tags):
        order = np.argsort(tab[0][j], kind="stable")
        if kind in ("near", "under"):
            assert hits["t"][j] == np.float32(0.0625) ** 2 and tab[0][j, order[0]] < tab[0][j, order[1]]     # the unique minimum
            assert (exp[1]["x"][j], exp[1]["y"][j], exp[1]["z"][j]) == (q[j, 0], q[j, 1], q[j, 2])           # ... from the corner P0
        elif kind == "fourth":
            fourth = S if i > S else S - 1
            assert q[j, 3] == tab[0][j, fourth] and (tab[0][j] <= q[j, 3]).sum() == 4                        # closed: four petals, cut on the seam
            assert sorted(np.nonzero(tab[0][j] <= q[j, 3])[0].tolist()) == ([S, S + 1, S + 2, S + 3] if i > S else [S - 4, S - 3, S - 2, S - 1])
    for lost in _seam_records(n_tris):                                   # teeth, as for the sweeps
        less = sc.triangle_winners(tab, q[:, 3], drop={lost})
        changed = set(sc.tde.differing(less, exp).tolist())
        mine = {j for j, tg in enumerate(tags) if tg[0] != "general" and tg[2] == lost}
        assert mine and mine <= changed, (n_tris, lost)
        assert all(less[0]["prim"][j] != lost for j in mine)
    for layout in sc.layouts(n_tris)[1:]:
        lrows, linfo = sc.seam_scene(n_tris, layout)
        tt = sc.tie_table(tab, linfo)
        assert _same_tables([x[aimed] for x in tt], sc.triangle_table(q[aimed], lrows))
        w = sc.triangle_winners(tt, q[:, 3])
        pair_rows = _check_named(tags, w[0]["prim"], tt[0], linfo, (n_tris, layout))
        assert {tags[j][0] for j in pair_rows} >= {"near", "under"}
        high = sc.triangle_winners(tt, q[:, 3], tie_high=True)
        assert all(high[0]["prim"][j] == tags[j][1] for j in pair_rows)
        flipped = np.nonzero(aimed & (high[0]["prim"] != w[0]["prim"]))[0]              # (the triangle at the twin's empty place as well)
        assert set(pair_rows) <= set(flipped.tolist()) and all(high[0]["prim"][j] == w[0]["prim"][j] + 1 == tags[j][1] for j in flipped)
