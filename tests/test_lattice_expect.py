"""The lattice scenes of lattice_cases.py without a device: the host builder's trees on them (flat child boxes, copies spread
over many leaves), the three numpy restatements of the BVH kernels walking those trees against the oracle's brute force, that
the populations reach the branches they are made for (NaN and +-inf in the box test, exact ties between leaves, hits on an
interval's end), and that the comparison notices a traversal without the tie rule or with non-strict pruning."""
import numpy as np
import pytest

import lattice_cases as lc
from allhits_expect import (check_bvh_all_hits, expected_all_hits, hit_table_uv, same_rows, sets_from_table, truncated,
                            walk_tree_all_hits)
from occluded_expect import check_bvh_occluded, conditioning_matrix, expected_occluded, in_interval, walk_tree_occluded
from query_accel_expect import EMPTY, LEAF, WELL_CONDITIONED, check_against_scan, check_tree, conditioning, leaf_span, walk_tree
from query_expect import edge_rows, expected_hits, same_hits

SCENES = ("rooms", "copies", "cornell32")
MIN_RATIO = 0.4                                 # below 1 / sqrt(3) / sqrt(2) = 0.408: see test_lattice_hits_are_well_conditioned
_cache = {}


def case(orc, scene, contract):
    """The scene, its tree, its populations and their hit tables under one arithmetic mode, made once per session."""
    key = (scene, contract)
    if key in _cache:
        return _cache[key]
    from raytracertest_amd import api, scenes
    c = {"exact": ()}
    if scene == "rooms":
        c["rows"] = lc.rooms()
    elif scene == "copies":
        c["rows"], c["first"], c["second"], c["third"] = lc.copies()
    else:
        c["rows"] = scenes.cornell32()
    c["tree"] = api.bvh_build(c["rows"])
    if scene == "rooms":
        c["pops"], c["ab"] = lc.rooms_populations(orc, c["rows"], c["tree"][0], contract)
        c["exact"] = lc.LATTICE
    elif scene == "copies":
        c["pops"] = {"copies": lc.copies_rays(), "control": lc.control_rays(c["rows"])}
        c["exact"] = ("copies",)
    else:
        c["pops"] = lc.cornell_populations(orc, c["rows"], contract)
        c["pops"]["frame"] = np.ascontiguousarray(c["pops"]["frame"][::5])       # the walks take every fifth pinhole ray
    if contract == orc.STRICT:                   # the second arithmetic mode takes every second ray (the lattice's are exact in both)
        c["pops"] = {k: np.ascontiguousarray(r[np.arange(r.shape[0]) % 4 % 3 == 0]) for k, r in c["pops"].items()}   # 0, 3, 4, 7
    c["table"] = {k: hit_table_uv(orc, r, c["rows"], None, contract) for k, r in c["pops"].items()}
    c["segs"] = {k: lc.segments(k, r, c["table"][k]) for k, r in c["pops"].items()}
    c["hits"] = {(k, nearest): lc.hits_from_table(t, nearest) for k, t in c["table"].items() for nearest in (False, True)}
    _cache[key] = c
    return c


def walked(orc, scene, contract):
    """The walks of every population of a case, made once: ({(population, query, ...): (got, expected)}, their counters)."""
    c = case(orc, scene, contract)
    if "walks" not in c:
        c["stats"] = {}
        c["walks"] = _check_walks(orc, c, contract, list(c["pops"]), stats=c["stats"])
    return c["walks"], c["stats"]


def flat_children(nodes):
    """How many present child boxes have lo == hi on some axis."""
    return sum(int(((nodes["lo"][:, :, c] == nodes["hi"][:, :, c]).any(axis=1) & (nodes["child"][:, c] != EMPTY)).sum())
               for c in range(4))


def leaves_holding(nodes, recs, prims):
    """The number of leaves that hold at least one of the upload indices `prims`."""
    count = 0
    for nd in nodes:
        for c in range(4):
            ref = int(nd["child"][c])
            if ref != EMPTY and ref & LEAF:
                first, n = leaf_span(ref)
                count += bool(np.isin(recs["index"][first:first + n], prims).any())
    return count


def multiplicity(table, nearest):
    """Per ray: how many triangles tie at the winning t (the largest; nearest: the smallest t > 0), 0 without a hit."""
    hit, t = table[0], table[1]
    out = np.zeros(hit.shape[0], np.int64)
    for i in range(hit.shape[0]):
        ts = t[i][hit[i]]
        ts = ts[ts > 0] if nearest else ts
        if ts.size:
            out[i] = int((ts == (ts.min() if nearest else ts.max())).sum())
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_tree_structure_of_the_lattice_scenes(orc, scene):
    from raytracertest_amd import api
    c = case(orc, scene, orc.FMA)
    for edges in (False, True):
        up = edge_rows(c["rows"]) if edges else c["rows"]
        nodes, recs, info = api.bvh_build(up, edges)
        depth = check_tree(nodes, recs, info, up, edges)
        assert info["always_tested"] == 0
        flat = flat_children(nodes)
        print("%s edges=%d: %d nodes, %d leaves, depth %d, %d flat child boxes" % (scene, edges, info["nodes"], info["leaves"], depth, flat))
        if scene == "rooms":
            assert c["rows"].shape == (3 * 480, 4) and depth >= 4
            assert flat >= 50                                            # (112: the leaves of one wall; no inner box is flat)
        elif scene == "cornell32":
            assert flat >= 1
        else:
            assert c["first"].size == 33 and c["second"].size == 9
            assert leaves_holding(nodes, recs, c["first"]) >= 9
            assert (np.diff(c["first"]) > 1).sum() >= 16                 # scattered upload indices


@pytest.mark.parametrize("contract", [0, 1])
def test_lattice_hits_are_well_conditioned(orc, contract):
    """Why the lattice populations may not use the exclusion: quad triangles are right triangles with unit legs, the directions
    are axes, face and space diagonals, and a triangle that contains the ray has det = 0 and is no hit; so every accepted hit has
    det / (|d| |e1| |e2|) >= 1 / sqrt(3) / sqrt(2) = 0.408 (a space diagonal against a record whose e2 is the hypotenuse), far
    above the contract's 2^-10.  Asserted over every hit the oracle lists; the rounded origins of on_surface and the pairs
    (d = b - a in fp32) keep the same directions."""
    c = case(orc, "rooms", contract)
    for name in lc.LATTICE:
        rays, hit = c["pops"][name], c["table"][name][0]
        ratio = conditioning_matrix(rays, c["rows"])[hit]
        print("rooms %s contract=%d: %d rays, %d hits, smallest ratio %.4f" % (name, contract, rays.shape[0], int(hit.sum()), ratio.min()))
        assert hit.sum() > rays.shape[0] and ratio.min() >= MIN_RATIO, (name, ratio.min())
        win = expected_hits(orc, rays[::4], c["rows"], None, contract)   # the same figure by the other helper, for some winners
        assert conditioning(rays[::4], c["rows"], win["prim"]).min() >= MIN_RATIO
    c = case(orc, "copies", contract)
    rays, hit = c["pops"]["copies"], c["table"]["copies"][0]
    ratio = conditioning_matrix(rays, c["rows"])
    both = np.r_[c["first"], c["second"], c["third"]]
    on_copies = ratio[:, both][hit[:, both]].min()
    print("copies contract=%d: smallest ratio %.4f on the copies, %.4f over every hit" % (contract, on_copies, ratio[hit].min()))
    assert on_copies >= MIN_RATIO               # (0.82 by construction: steep rays on a fat triangle)
    assert ratio[hit].min() >= 64 * WELL_CONDITIONED                     # the general-position neighbours: inside the contract


@pytest.mark.parametrize("contract", [0, 1])
def test_populations_reach_what_they_are_for(orc, contract):
    """NaN and +-inf in the restated box test, ties of four and more triangles at the winning t, all 33 copies at one t, and
    segments decided by a hit that lies on an end of the interval, bit for bit.

    At the product's rho = 2^-8 an origin ON a wall gives no NaN: the slab planes are lo - pad and hi + pad, pad > 0, so
    (lo - pad) - o is never 0 there.  The NaN branch is reached by the part of in_plane that lattice_cases.padded_plane_rays
    puts into the padded planes of the dumped tree; the on-wall origins reach it with bare boxes (rho = 0), which is also what
    the device test runs at slack 0."""
    c = case(orc, "rooms", contract)
    nodes, recs, info = c["tree"]
    reach = walked(orc, "rooms", contract)[1]
    for key, st in reach.items():
        if key[0] in ("axis", "in_plane"):
            print("rooms contract=%d %s: %s" % (contract, key, st))
            assert st.get("inf_rays", 0) > 0, key
            if key[0] == "in_plane":
                assert st.get("nan_rays", 0) > 0, key
    for name in ("in_plane", "on_surface"):                              # the on-wall origins: a NaN with bare boxes
        st = {}
        walk_tree(orc, nodes, recs, info, c["pops"][name], c["rows"], contract, rho=np.float32(0), stats=st)
        print("rooms contract=%d %s rho=0: %s" % (contract, name, st))
        assert st.get("nan_rays", 0) >= c["pops"][name].shape[0] // 4
    neg = c["pops"]["axis"][:, 3:]
    assert (np.signbit(neg) & (neg == 0)).any(axis=1).sum() >= c["pops"]["axis"].shape[0] // 4      # -0.0 in a direction

    for nearest in (False, True):
        m = multiplicity(c["table"]["vertex"], nearest)
        print("rooms vertex contract=%d nearest=%d: largest tie %d, %d rays with >= 4" % (contract, nearest, m.max(), int((m >= 4).sum())))
        assert (m >= 4).sum() >= 10

    # the pairs: occluded over [0, 1] by hits at t == 1 (or t == 0) alone, and visible once that end is taken out
    rays, table = c["pops"]["pairs"], c["table"]["pairs"]
    fam = lc.pair_segments(rays, table)
    inside = in_interval(fam["unit"], (table[0], table[1]))
    t = table[1]
    at_b = inside.any(axis=1) & (~inside | (t == np.float32(1))).all(axis=1)
    at_a = inside.any(axis=1) & (~inside | (t == np.float32(0))).all(axis=1)
    occ = {k: expected_occluded(orc, s, c["rows"], None, contract, (table[0], table[1])) for k, s in fam.items()}
    print("rooms pairs contract=%d: %d pairs, occluded %s, decided at t == 1 alone %d, at t == 0 alone %d"
          % (contract, rays.shape[0], {k: int(v.sum()) for k, v in occ.items()}, int(at_b.sum()), int(at_a.sum())))
    assert at_b.sum() >= 1 and occ["unit"][at_b].all() and not occ["short_of_b"][at_b].any()
    assert at_a.sum() >= 1 and occ["unit"][at_a].all() and not occ["past_a"][at_a].any()
    assert occ["at_a_hit"].sum() >= rays.shape[0] // 2 and not occ["empty"].any()
    assert (~occ["unit"]).any() and (rays[:, 3:] == 0).all(axis=1).sum() >= 1    # visible pairs too; the identical points

    c = case(orc, "copies", contract)
    hit, t = c["table"]["copies"][0], c["table"]["copies"][1]
    first, second = c["first"], c["second"]
    all33 = hit[:, first].all(axis=1) & (t[:, first] == t[:, first[:1]]).all(axis=1)
    all42 = all33 & hit[:, second].all(axis=1) & (t[:, second] == t[:, first[:1]]).all(axis=1)
    print("copies contract=%d: %d rays, all 33 copies at one t for %d, all 42 for %d" % (contract, hit.shape[0], int(all33.sum()), int(all42.sum())))
    assert all33.sum() >= 20 and all42.sum() >= 10 and (~hit[:, first].any(axis=1)).sum() >= 10


def _check_walks(orc, c, contract, names, stats=None, **switch):
    """Every walk of the populations `names` with what the brute force expects, as {(population, query, ...): (got, expected)}.
    stats: receives each walk's box-test counters under the same keys.  (`control` takes max_hits 4 and 16 only: its far origins
    inflate every box and the walk visits the whole tree.)"""
    nodes, recs, info = c["tree"]
    rows = c["rows"]
    out = {}
    occ_switch = {k: v for k, v in switch.items() if k != "tie_rule"}    # (the any-hit walk has no tie rule)
    for name in names:
        rays, table = c["pops"][name], c["table"][name]
        segs, idx = c["segs"][name]
        st = (lambda *key: stats.setdefault(key, {})) if stats is not None else (lambda *key: None)
        for nearest in (False, True):
            got, _ = walk_tree(orc, nodes, recs, info, rays, rows, contract, nearest, stats=st(name, "intersect", nearest), **switch)
            out[name, "intersect", nearest] = (got, c["hits"][name, nearest])
        sub = (table[0][idx], table[1][idx])
        exp = expected_occluded(orc, segs, rows, None, contract, sub)
        got, _ = walk_tree_occluded(orc, nodes, recs, info, segs, rows, None, contract, stats=st(name, "occluded"), **occ_switch)
        out[name, "occluded"] = (got, exp)
        exp16 = expected_all_hits(table, segs, 16, idx)
        for max_hits in ((4, 16) if name == "control" else (1, 4, 5, 16)):
            hits, counts, _ = walk_tree_all_hits(orc, nodes, recs, info, segs, rows, max_hits, None, contract,
                                                 stats=st(name, "all_hits", max_hits), **switch)
            out[name, "all_hits", max_hits] = ((hits, counts), truncated(exp16, max_hits))
    return out


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("scene", SCENES)
def test_winners_read_off_the_hit_table_are_the_oracle_scan(orc, scene, contract):
    """lattice_cases.hits_from_table (the largest t, or the smallest t > 0, of a ray's row of the oracle's hit table; equal t to
    the lowest upload index) is expected_hits, the scan in upload order with strict comparisons: checked on every third ray."""
    c = case(orc, scene, contract)
    for name, rays in c["pops"].items():
        for nearest in (False, True):
            assert same_hits(c["hits"][name, nearest][::3], expected_hits(orc, rays[::3], c["rows"], None, contract, nearest)), (name, nearest)


@pytest.mark.parametrize("contract", [0, 1])
@pytest.mark.parametrize("scene", SCENES)
def test_restated_walks_against_brute_force(orc, scene, contract):
    """walk_tree (both hit rules), walk_tree_occluded and walk_tree_all_hits (max_hits 1, 4, 5, 16) under the contracts' checks;
    the lattice populations and the copies' rays are bit-exact as well, with no ray under the exclusion."""
    c = case(orc, scene, contract)
    rows = c["rows"]
    for (name, query, *arg), (got, exp) in walked(orc, scene, contract)[0].items():
        rays, table = c["pops"][name], c["table"][name]
        segs, idx = c["segs"][name]
        label = "%s %s %s %s contract=%d" % (scene, name, query, arg, contract)
        if query == "intersect":
            used = check_against_scan(got, exp, rays, rows, label=label)
            assert (exp["prim"] >= 0).any(), label
            same = same_hits(got, exp)
        elif query == "occluded":
            used = check_bvh_occluded(got, exp, segs, rows, orc, None, contract, table=(table[0][idx], table[1][idx]), label=label)
            assert exp.any() and (~exp).any(), label
            same = np.array_equal(got, exp)
        else:
            E, W = sets_from_table(table, segs, rows, idx)
            used = check_bvh_all_hits(got, exp, E, W, arg[0], every=name not in c["exact"], label=label)
            same = same_rows(got, exp)
        if name in c["exact"]:
            assert used == 0 and same, label


@pytest.mark.parametrize("contract", [0, 1])
def test_a_walk_without_the_tie_rule_is_noticed(orc, contract):
    """Teeth: a traversal that lets the first VISITED triangle keep a tie (walk_tree) or keeps equal t in the order of arrival
    (walk_tree_all_hits) changes answers on `vertex` and on the copies' rays, under both hit rules and at max_hits 4."""
    for scene, name in (("rooms", "vertex"), ("copies", "copies")):
        c = case(orc, scene, contract)
        nodes, recs, info = c["tree"]
        rays, table = c["pops"][name], c["table"][name]
        segs, idx = c["segs"][name]
        for nearest in (False, True):
            exp = c["hits"][name, nearest]
            got, _ = walk_tree(orc, nodes, recs, info, rays, c["rows"], contract, nearest, tie_rule=False)
            changed = int((got["prim"] != exp["prim"]).sum())
            print("%s %s contract=%d nearest=%d without the tie rule: %d of %d rays change"
                  % (scene, name, contract, nearest, changed, rays.shape[0]))
            assert changed >= 1 and np.array_equal(got["t"], exp["t"])   # another triangle of the same tie
            with pytest.raises(AssertionError):
                check_against_scan(got, exp, rays, c["rows"], label="no tie rule")
        exp = expected_all_hits(table, segs, 4, idx)
        got = walk_tree_all_hits(orc, nodes, recs, info, segs, c["rows"], 4, None, contract, tie_rule=False)[:2]
        changed = int(((got[0]["prim"] != exp[0]["prim"]).any(axis=1) | (got[1] != exp[1])).sum())
        print("%s %s contract=%d IntersectAll(4) without the tie rule: %d of %d rows change" % (scene, name, contract, changed, segs.shape[0]))
        assert changed >= 1
        E, W = sets_from_table(table, segs, c["rows"], idx)
        with pytest.raises(AssertionError):
            check_bvh_all_hits(got, exp, E, W, 4, label="no tie rule")
    c = case(orc, "copies", contract)                                    # and what the rule gives: the lowest upload indices, in order
    segs, idx = c["segs"]["copies"]
    exp = expected_all_hits(c["table"]["copies"], segs, 16, idx)
    both = np.sort(np.r_[c["first"], c["second"], c["third"]])
    full = np.nonzero((exp[1] == 16) & np.isin(exp[0]["prim"][:, 0], both))[0]
    assert full.size >= 5
    for i in full:
        p = exp[0]["prim"][i]
        tied = p[exp[0]["t"][i] == exp[0]["t"][i, 0]]
        assert (np.diff(tied) > 0).all() and tied.size >= 4


def test_non_strict_pruning_on_bare_boxes_is_noticed(orc):
    """Teeth for the strictness of the pop and prune comparisons (g < lim, exit < tmin, enter > tmax, enter > t_last): with bare
    boxes (rho = 0) a flat box's enter and exit EQUAL the t of the wall inside it, so the non-strict forms drop tied triangles and
    hits on an interval's end.  With rho = 0 and strict comparisons the exact populations still equal the brute force (their box
    arithmetic is exact; every third ray of each is walked); on_surface and pairs are left out of that claim, since their rounded origins make bare boxes lose hits
    for their own reasons.  Outcome: the non-strict walks change answers in every query, so that is asserted -- Intersect 4
    in_plane + 47 vertex rays, Occluded 9 vertex rays, IntersectAll 5 + 105 rows over max_hits 1, 4, 5, 16; no axis ray changes
    (from a cell centre or quarter point along an axis nothing ties and no hit lies on an interval's end)."""
    full = case(orc, "rooms", orc.FMA)
    names = ["axis", "in_plane", "vertex"]
    c = {"tree": full["tree"], "rows": full["rows"], "pops": {k: np.ascontiguousarray(full["pops"][k][::3]) for k in names}}
    c["table"] = {k: tuple(x[::3] for x in full["table"][k]) for k in names}
    c["segs"] = {k: lc.segments(k, c["pops"][k], c["table"][k]) for k in names}
    c["hits"] = {(k, nearest): np.ascontiguousarray(full["hits"][k, nearest][::3]) for k in names for nearest in (False, True)}
    zero = np.float32(0)
    strict = _check_walks(orc, c, orc.FMA, names, rho=zero)
    loose = _check_walks(orc, c, orc.FMA, names, rho=zero, strict=False)
    changed = {}
    for key, (got, exp) in strict.items():
        g2 = loose[key][0]
        if key[1] == "intersect":
            assert same_hits(got, exp), key
            n = int((g2.view(np.uint32).reshape(-1, 4) != exp.view(np.uint32).reshape(-1, 4)).any(axis=1).sum())
        elif key[1] == "occluded":
            assert np.array_equal(got, exp), key
            n = int((g2 != exp).sum())
        else:
            assert same_rows(got, exp), key
            m = exp[1].shape[0]
            n = int(((g2[0].view(np.uint32).reshape(m, -1) != exp[0].view(np.uint32).reshape(m, -1)).any(axis=1) | (g2[1] != exp[1])).sum())
        changed[key] = n
    print("rho = 0, strict=False, rays that change:", changed)
    for query in ("intersect", "occluded", "all_hits"):
        assert sum(n for key, n in changed.items() if key[1] == query) >= 1, query
