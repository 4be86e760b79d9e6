"""The small-scene kernels (TracePath::SmallLists and its four list builders, the full scan beside them; tests/small_cases.py)
against the oracle under every render option: both arithmetic modes, both hit rules, spheres, smooth normals, each builder,
the filtered and the unfiltered kernel, the certain-winner switches, unsplit, split, interleaved, band and ragged frames, partial
sample passes at K = 1, 2 and 4, fused iterations, cadences and owing steps, lists kept and rebuilt -- all four buffers bit for
bit.  Each case also proves what it ran: K and the LDS of its trace kernel (rt_tracer_info), the builder kernel by its kind
(rt_dbg_list_builds), the kinds of tiles in its lists (rt_dbg_read_tile_lists) and the draws it owes (rt_dbg_owed_state).
tests/test_small_cases.py shows on the CPU that every option a case uses changes the oracle's frame.

What the read-backs do not show: whether the trace kernel skipped a tile whose list says certain.  The builders set that flag
from the geometry alone -- for nearest hit, spheres, smooth normals and no_sure_hit too, where only the kernel ignores it
(rt_trace.hpp: sure_ok) -- so for those cases the test checks the flag's documented meaning (every probed ray of the tile hits
the winner and nothing farther) and that the tracer owes no draws; that no tile was skipped follows from the frame alone: a
skipped tile shows the farthest triangle in its face colour, and the CPU teeth show that this is another frame."""
import numpy as np
import pytest

import small_cases as sc

pytestmark = pytest.mark.gpu
BY_NAME = {c["name"]: c for c in sc.CASES}
ENV = {"per_pixel": "RT_MI355X_NO_SURE_TABLE", "no_owe": "RT_MI355X_NO_OWE"}


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    from raytracertest_amd import api
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return api


def first_difference(a, b):
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
    return None if d.size == 0 else (d.shape[0], d[0].tolist())


def run(rt, monkeypatch, case):
    """the case on a fresh tracer: (the four buffers, what the tracer says it ran)"""
    f = sc.frame(case)
    seed = sc.seed_of(case)
    tris, edges = sc.scene(case, seed)
    env = {ENV[case["winners"]]: "1"} if case["winners"] in ENV else {}
    if sc.interleave(case) is not None:
        env["RT_MI355X_ROW_INTERLEAVE"] = str(sc.interleave(case))
    for k, v in env.items():                                             # (read when the tracer is created)
        monkeypatch.setenv(k, v)
    g = rt.RayTracer((f["W"], f["rows"]), (0, 0, 0), f["angles"], f["fov"], sc.FOCAL, sc.APERTURE, seed=seed,
                     math_mode=rt.MATH_FMA if case["math"] == "fma" else rt.MATH_STRICT, full_height=f["full_h"], row_begin=f["row_begin"],
                     nearest_hit=case["hit"] == "near", smooth_normals="smooth" in case["extras"],
                     no_filter=case["kernel"] == "unfiltered", no_binning=case["kernel"] == "scan",
                     no_sure_hit=case["winners"] == "traced", samples_in_flight=case["extra"].get("k", 0))
    for k in env:
        monkeypatch.delenv(k)
    assert (g.UploadSceneEdges if edges else g.UploadScene)(tris)
    if "spheres" in case["extras"]:
        g.UploadSpheres(sc.SPHERES)
    if case["reuse"] == "rebuilt":
        g.SetListReuse(False)
    n, spp = sc.iterations(case), case["spp"]
    whole = case["shape"] == "unsplit"                                   # Trace() launches are never split: the split frames enqueue
    if case["iters"] == "one":
        g.TraceEnqueue(1, spp); g.Sync()
    elif case["iters"] == "steps":
        g.TraceEnqueueN(1, spp, sc.n_steps(case))
    elif case["iters"] == "fused":
        assert 1 < n <= g.FusedIterations(spp), (n, g.FusedIterations(spp))
        if whole:
            g.Trace(n, spp, 0); assert g.Wait()
        else:
            g.TraceEnqueue(n, spp); g.Sync()
    else:
        if whole:
            updates = []
            g.SetUpdateCallback(lambda img, size: updates.append(size))
            g.Trace(n, spp, 1); assert g.Wait()
            assert updates, "no update point: the launches were not cut"
        else:
            for i in range(n):
                g.Launch(spp, clear_first=i == 0, emit_image=i == n - 1)
            g.Sync()
    ran = {"owed": g.DebugOwedState()["owed_draws"]}                     # before the read-back that settles them
    got = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
    ran["owed_after"] = g.DebugOwedState()["owed_draws"]
    ran["info"] = g.Info()
    ran["builds"] = g.DebugListBuilds()
    if case["kernel"] != "scan":
        ran["lists"] = g.DebugTileLists()
    else:
        with pytest.raises(rt.RtError, match="no tile lists"):
            g.DebugTileLists()
    g.close()
    return got, ran


def assert_equals_oracle(case, got, o):
    for name, a, b in zip(("render", "counts", "rng", "image"), got, (o.render, o.counts, o.rng, o.image)):
        diff = first_difference(a, b)
        assert diff is None, "%s: %s differs from the oracle in %d words, first at (row, x, ...) %s" % (case["name"], name, *diff)
    assert (got[1] == sc.iterations(case) * case["spp"]).all()           # (a steps case: what one step accumulates)


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_small_scene_kernels_equal_the_oracle_under_every_option(rt, orc, monkeypatch, case):
    got, ran = run(rt, monkeypatch, case)
    assert_equals_oracle(case, got, sc.oracle(orc, case))

    # which trace kernel ran, and which builder
    info = ran["info"]
    assert info["samples_in_flight"] == sc.samples_in_flight(case) and info["lds_bytes"] == sc.lds_bytes(case), info
    want = [0, 0, 0, 0]
    if case["kernel"] != "scan":
        want[sc.builder_kind(case)] = sc.list_builds(case)
    assert ran["builds"] == want, (case["name"], ran["builds"], want)
    # owed draws: every step after the first of a case with certain winners, unless RT_MI355X_NO_OWE; settled by the read-back
    assert ran["owed"] == sc.owed_draws(case) and ran["owed_after"] == 0, (case["name"], ran["owed"], sc.owed_draws(case))
    if case["winners"] == "table" and case["iters"] == "steps" and sc.has_certain_winners(case):
        assert ran["owed"] > 0
    if case["kernel"] == "scan":
        return

    # the tiles of the stored lists against the oracle's probe of every tile (its pixels x 9 lens points).  The lists are
    # conservative and the probed rays are rays of the tile, so: a tile flagged certain is a certain candidate of the probe with
    # the same winner; a traced tile with an empty list is one whose probed rays hit nothing; and a traced tile's list is at
    # least as long as the number of triangles its probed rays hit.
    count, winner, certain = ran["lists"]
    kind, cpu_winner, met = sc.tile_kinds(orc, case)
    ny, nx = kind.shape
    count, winner, certain = count[:ny, :nx], winner[:ny, :nx], certain[:ny, :nx]      # the tiles that hold pixels
    kinds = (int(certain.sum()), int((~certain & (count == 0)).sum()), int((~certain & (count > 0)).sum()))
    cpu_kinds = (int((kind == sc.CERTAIN).sum()), int((kind == sc.NOTHING).sum()), int((kind == sc.MIXED).sum()))
    print(case["name"], "builds", ran["builds"], "certain / traced and empty / traced with candidates:", kinds, "probe:", cpu_kinds)
    assert (kind[certain] == sc.CERTAIN).all() and (winner[certain] == cpu_winner[certain]).all(), case["name"]
    assert (kind[~certain & (count == 0)] == sc.NOTHING).all(), case["name"]
    assert (count[~certain] >= met[~certain]).all() and (count <= case["n_tris"]).all(), case["name"]
    assert kinds[0] <= cpu_kinds[0] and kinds[1] <= cpu_kinds[1] and kinds[2] >= cpu_kinds[2], (case["name"], kinds, cpu_kinds)
    if sc.hot(case):
        assert kinds[0] >= 8 and kinds[1] >= 1 and kinds[2] >= 8, (case["name"], kinds)


@pytest.mark.parametrize("name", sc.HOT_ANCHORS)
def test_the_certain_winner_switches_change_the_work_never_the_answer(rt, orc, monkeypatch, name):
    """each hot anchor again under per_pixel, no_owe and traced: the four buffers of `table`, byte for byte -- and the oracle's"""
    case = BY_NAME[name]
    assert case["winners"] == "table" and sc.hot(case)
    base, ran = run(rt, monkeypatch, case)
    o = sc.oracle(orc, case)
    assert_equals_oracle(case, base, o)
    for winners in ("per_pixel", "no_owe", "traced"):
        variant = dict(case, winners=winners)
        got, ran_v = run(rt, monkeypatch, variant)
        for what, a, b in zip(("render", "counts", "rng", "image"), got, base):
            assert a.tobytes() == b.tobytes(), "%s under %s: %s differs from the same case under table" % (name, winners, what)
        assert_equals_oracle(variant, got, o)
        assert ran_v["builds"] == ran["builds"] and ran_v["owed"] == sc.owed_draws(variant)
        for a, b in zip(ran_v["lists"], ran["lists"]):                  # the same lists, certain flags included: only the kernel's use of them differs
            assert np.array_equal(a, b)
