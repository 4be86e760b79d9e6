"""The numpy restatements of the eight newer queries at scales 2^k (tests/range_cases.py), without a device: inside each query's
stated range the answers on the lattice populations are the k = 0 answers exactly rescaled, and one step beyond either end some
row differs (the ranges are not vacuous); and on the scene of the device tests every restated tree walk gives the brute-force
bytes at every k of TREE_KS, down to where squares underflow and up to where they overflow -- SphereCast's through the range
guard of its walk, without which it loses records at both ends."""
import numpy as np
import pytest

import range_cases as rc
import spherecast_expect as se

_base = {}


def _tree(rows):
    from raytracertest_amd import api
    return api.bvh_build(rows)


def _at(kind, query, k):
    rows, spheres = rc.scene(kind)
    r, s = rc.scaled_scene(rows, spheres, k)
    return rc.brute_force(query, r, s, rc.scaled_populations(rc.populations(kind), k))


def _base_answer(kind, query):
    if (kind, query) not in _base:
        _base[kind, query] = _at(kind, query, 0)
    return _base[kind, query]


@pytest.mark.parametrize("query", rc.QUERIES)
def test_inside_its_range_a_query_answers_the_rescaled_bytes_and_beyond_it_does_not(query):
    lo, hi = rc.RANGE[query]
    base = _base_answer("lattice", query)
    n = base[0].shape[0]
    assert n // 3 <= rc.found(query, base) and all(lo <= k <= hi for k in rc.INVARIANCE_KS)
    for k in rc.INVARIANCE_KS + (lo, hi):
        got = _at("lattice", query, k)
        bad = rc.differing_rows(got, rc.rescaled(query, base, k))
        assert bad.size == 0, (query, k, bad[:5])
    for k in (lo - 1, hi + 1):
        got = _at("lattice", query, k)
        bad = rc.differing_rows(got, rc.rescaled(query, base, k))
        print("%s at k = %d, one step beyond [%d, %d]: %d of %d rows differ, %d of %d queries still find something"
              % (query, k, lo, hi, bad.size, n, rc.found(query, got), rc.found(query, base)))
        assert bad.size > 0, (query, k)


def test_the_populations_reach_what_they_are_for():
    for kind in ("lattice", "slivers"):
        pops = rc.scaled_populations(rc.populations(kind), 0)
        rows, spheres = rc.scene(kind)
        for query in rc.QUERIES:
            a = _base_answer(kind, query)
            n, hit = a[0].shape[0], rc.found(query, a)
            print("%s %s: %d of %d find something" % (kind, query, hit, n))
            assert hit >= n // 3 and (kind == "lattice" or n - hit >= n // 10), (kind, query, hit, n)
        cast = _base_answer(kind, "spherecast_kept")[0]
        assert ((cast["prim"] >= 0) & (cast["t"] == 0)).sum() >= 50 and ((cast["prim"] >= 0) & (cast["t"] > 0)).sum() >= 50
        assert np.isfinite(pops["points"][:, 3]).sum() >= 100 and np.isinf(pops["points"][:, 3]).sum() >= 100
    assert _tree(rc.scene("slivers")[0])[2]["always_tested"] == 1       # the bad record
    # the scaling is exact: back again gives the bits, at both ends of TREE_KS
    rows = rc.scene("slivers")[0]
    for k in (min(rc.TREE_KS), max(rc.TREE_KS)):
        back = rc.scaled_scene(rc.scaled_scene(rows, None, k)[0], None, -k)[0]
        assert np.array_equal(back.view(np.uint32), rows.view(np.uint32), ) or np.array_equal(back[~np.isnan(rows)], rows[~np.isnan(rows)])
    low = _at("slivers", "closest", -64)[0]                              # squared distances in the subnormals, not flushed
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((low["prim"] >= 0) & (low["t"] > 0) & (low["t"] < tiny)).sum() >= 100


@pytest.mark.parametrize("k", rc.TREE_KS)
def test_every_restated_walk_gives_the_brute_force_bytes_at_every_scale(k):
    rows, spheres = rc.scene("slivers")
    r, s = rc.scaled_scene(rows, spheres, k)
    pops = rc.scaled_populations(rc.populations("slivers"), k)
    tree = _tree(r)
    line = []
    for query in rc.TREE_QUERIES:
        want = rc.brute_force(query, r, s, pops)
        got = rc.tree_walk(query, tree, r, s, pops)
        bad = rc.differing_rows(got, want)
        line.append("%s %d/%d" % (query, rc.found(query, want), want[0].shape[0]))
        assert bad.size == 0, (query, k, bad[:5])
    print("k = %d: found / queries: %s" % (k, ", ".join(line)))


def test_without_the_range_guard_the_sweep_walk_loses_records_at_both_ends():
    rows, spheres = rc.scene("slivers")
    changed = {}
    for k in (-76, -70, 0, 60):
        r, s = rc.scaled_scene(rows, spheres, k)
        sweeps = rc.scaled_populations(rc.populations("slivers"), k)["sweeps_kept"]
        with np.errstate(all="ignore"):
            want = se.expected(sweeps, r, spheres=s)
            got, _ = se.walk_tree_spherecast(*_tree(r), sweeps, r, spheres=s, range_guard=False)
        changed[k] = int(se.differing(got, want).size)
    print("sweeps whose unguarded walk differs from brute force, of %d: %s" % (sweeps.shape[0], changed))
    assert changed[0] == 0 and changed[-76] > 1000 and changed[-70] > 0 and changed[60] > 10
