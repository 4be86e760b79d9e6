"""The dense-scene kernels (DenseLists, ClassifyForms, Classify; tests/dense_cases.py) against the oracle under every render
option: both arithmetic modes, both hit rules, spheres, smooth normals, overflowing lists, split launches with super tiles, row
bands, partial sample passes, fused and unfused iterations -- all four buffers bit for bit.  Each case also proves which
kernel it ran (rt_tracer_info, the wave lists in HBM), and the oracle shows that each option it uses changes the frame.

Plus the instrumented kernels (TraceStats): the frame they compute is the oracle's."""
import numpy as np
import pytest

import dense_cases as dc

pytestmark = pytest.mark.gpu
NO_LIST = 0xFFFFFFFF


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    from raytracertest_amd import api
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return api


def oracle(orc, case, seed, tris, edges, *, math=None, hit=None, spheres=None, smooth=None, row0=0, rows=None):
    """the case's oracle over rows [row0, row0 + rows) of the tracer's band, with one option changed if asked"""
    W, band_rows, full_h, band_r0 = dc.SHAPES[case["shape"]]
    cam = dc.CAMERA
    math = case["math"] if math is None else math
    hit = case["hit"] if hit is None else hit
    smooth = "smooth" in case["extras"] if smooth is None else smooth
    spheres = "spheres" in case["extras"] if spheres is None else spheres
    o = orc.OracleTracer(W, full_h or band_rows, cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=seed,
                         row0=band_r0 + row0, rows=band_rows if rows is None else rows, contract=1 if math == "fma" else 0,
                         nthreads=8, hit_mode=int(hit == "near"), smooth_normals=smooth)
    assert (o.upload_scene_edges if edges else o.upload_scene)(tris)
    if spheres:
        o.upload_spheres(dc.SPHERES)
    o.trace(dc.iterations(case), case["spp"])
    return o


def first_difference(a, b):
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
    return None if d.size == 0 else (d.shape[0], d[0].tolist())


@pytest.mark.parametrize("case", dc.CASES, ids=[c["name"] for c in dc.CASES])
def test_dense_kernels_equal_the_oracle_under_every_option(rt, orc, monkeypatch, case):
    W, rows, full_h, row_begin = dc.SHAPES[case["shape"]]
    seed = 7919 * (dc.CASES.index(case) + 1) % 100003
    tris, edges = dc.scene(case, seed)
    if case["path"] == "nopretest":
        monkeypatch.setenv("RT_MI355X_NO_PRETEST", "1")         # (read when the tracer is created)
    cam = dc.CAMERA
    g = rt.RayTracer((W, rows), (0, 0, 0), cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=seed,
                     math_mode=rt.MATH_FMA if case["math"] == "fma" else rt.MATH_STRICT, full_height=full_h, row_begin=row_begin,
                     nearest_hit=case["hit"] == "near", smooth_normals="smooth" in case["extras"],
                     no_macro_bins=case["path"] == "forms", no_filter=case["path"] == "nofilter",
                     bin_list=32 if case["path"] == "overflow" else 0, samples_in_flight=case["extra"].get("k", 0))
    monkeypatch.delenv("RT_MI355X_NO_PRETEST", raising=False)
    assert (g.UploadSceneEdges if edges else g.UploadScene)(tris)
    if "spheres" in case["extras"]:
        g.UploadSpheres(dc.SPHERES)
    if case["extra"].get("reuse") is False:
        g.SetListReuse(False)
    n, spp = dc.iterations(case), case["spp"]
    whole = case["shape"] == "unsplit"                        # Trace() launches are never split: the split frames enqueue
    if case["iters"] == "one":
        g.TraceEnqueue(1, spp); g.Sync()
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
    got = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())

    # which kernel ran
    info = g.Info()
    assert info["samples_in_flight"] == dc.samples_in_flight(case) and info["lds_bytes"] == dc.lds_bytes(case), info
    halves = dc.halves(case)
    if case["path"] in ("dense", "overflow"):
        cap = dc.LIST_CAP[case["path"]]
        for h, h_rows in enumerate(halves):
            counts, c = g.DebugWaveListCounts(h)
            assert c == cap and counts.size == ((W + 31) // 32) * ((h_rows + 7) // 8) * 4, (h, c, counts.size)
            over = counts == NO_LIST
            assert (counts[~over] <= cap).all()
            if case["path"] == "dense":
                assert (counts[~over] > 0).any(), "every list empty"
            else:
                assert over.any(), "no list overflowed: the hbm_overflow fallback did not run"
            if "spheres" in case["extras"] and case["shape"] == "split":     # (the 8:1 frame reaches past the cloud)
                assert (counts == 0).any(), "no tile with an empty list under the side sphere"
        if len(halves) == 1:
            with pytest.raises(rt.RtError, match="no wave lists"):
                g.DebugWaveListCounts(1)
    else:
        for h in (0, 1):
            with pytest.raises(rt.RtError, match="no wave lists"):
                g.DebugWaveListCounts(h)
    g.close()

    o = oracle(orc, case, seed, tris, edges)
    for name, a, b in zip(("render", "counts", "rng", "image"), got, (o.render, o.counts, o.rng, o.image)):
        diff = first_difference(a, b)
        assert diff is None, "%s: %s differs from the oracle in %d words, first at (row, x, ...) %s" % (case["name"], name, *diff)
    assert (got[1] == n * spp).all()

    # teeth: the oracle with one option of the case changed renders a different frame (checked on 16 rows of the band)
    r = rows // 2 - 8
    ref = o.render[r:r + 16].view(np.uint32)
    flips = {"math": dict(math="strict" if case["math"] == "fma" else "fma"),
             "hit": dict(hit="far" if case["hit"] == "near" else "near")}
    if "spheres" in case["extras"]:
        flips["spheres"] = dict(spheres=False)
    if "smooth" in case["extras"]:
        flips["smooth"] = dict(smooth=False)
    for what, kw in flips.items():
        t = oracle(orc, case, seed, tris, edges, row0=r, rows=16, **kw)
        assert not np.array_equal(t.render.view(np.uint32), ref), "%s: the oracle renders the same frame with %s changed" % (case["name"], what)


@pytest.mark.parametrize("mode", [0, 1])
def test_trace_stats_launch_computes_the_oracle_frame(rt, orc, mode):
    """rt_tracer_trace_stats clears the accumulators and runs one instrumented launch (the STATS kernels, dispatched by nothing
    else): on a fresh tracer its render, counts and RNG states equal the oracle's trace(1, s) -- a small scene (SmallLists),
    a dense one (ClassifyForms with counters), the unfiltered kernel (lane-level counters) and the full scan."""
    from raytracertest_amd import scenes
    W, H, spp = 96, 40, 5
    cam = dc.CAMERA
    dense = scenes.random_triangles(5000, 77)
    for scn, kw in ((scenes.cornell32(), {}), (dense, {}), (dense, dict(no_filter=True)), (scenes.random_triangles(600, 78), dict(no_binning=True))):
        g = rt.RayTracer((W, H), (0, 0, 0), cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=21, math_mode=mode, **kw)
        o = orc.OracleTracer(W, H, cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=21, contract=1 - mode, nthreads=8)
        assert g.UploadScene(scn) and o.upload_scene(scn)
        st = g.TraceStats(spp)
        o.trace(1, spp)
        what = "%d triangles %s" % (scn.shape[0] // 3, kw)
        assert any(v for k, v in st.items() if k != "tiles_by_list") or any(st["tiles_by_list"].values()), (what, st)
        for name, a, b in zip(("render", "counts", "rng"), (g.RenderBuffer(), g.SampleCounts(), g.RngStates()), (o.render, o.counts, o.rng)):
            diff = first_difference(a, b)
            assert diff is None, "%s: %s differs from the oracle in %d words, first at %s" % (what, name, *diff)
        if scn is dense and not kw:
            with pytest.raises(rt.RtError, match="no wave lists"):     # the instrumented launch classifies in the kernel
                g.DebugWaveListCounts(0)
        g.close()
