"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the
same seeded inputs.  Bar: bit-exact for everything (floats included) within one arithmetic
mode; the fp32 tolerance north_star allows is only needed ACROSS modes and is stated in
test_mode_tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    from raytracertest_amd import api
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return api


# ------------------------------------------------------------------ C1: the reference's KATs on the device
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("eps_mode", [0, 1])
def test_kats_on_device(rt, kats, mode, eps_mode):
    rays = np.array([np.concatenate([c["origin"], c["dir"]]) for c in kats], np.float32)
    tris = np.array([np.concatenate([c["a"], c["b"], c["c"]]) for c in kats], np.float32)
    hit, tuv, nrm, pt = rt.dbg_hit_triangle(rays, tris, math_mode=mode, eps_mode=eps_mode)
    for i, c in enumerate(kats):
        assert bool(hit[i]) == c["hit"], c["name"]
        if c["hit"]:
            assert int(u32(tuv[i, 0])) == int(c["t_bits"], 16), c["name"]      # t bit-checked
            assert np.array_equal(tuv[i, 1:], np.array([c["u"], c["v"]], np.float32)), c["name"]
            assert np.array_equal(nrm[i], np.array(c["normal"], np.float32)), c["name"]
            assert np.array_equal(pt[i], np.array(c["hitpoint"], np.float32)), c["name"]


@pytest.mark.parametrize("mode", [0, 1])
def test_hit_triangle_random_vs_oracle(rt, orc, mode):
    contract = 1 - mode                       # RT_MATH_FMA = 0 <-> oracle contract = 1
    rng = np.random.default_rng(42)
    n = 4000
    tris = rng.uniform(-2, 2, (n, 9)).astype(np.float32)
    tris[:, 2::3] -= 5.0
    rays = np.zeros((n, 6), np.float32)
    rays[:, :3] = rng.uniform(-0.5, 0.5, (n, 3))
    # aim at a random barycentric point so that many rays hit, some exactly on edges
    bary = rng.uniform(-0.2, 1.2, (n, 2)).astype(np.float32)
    bary[::7] = np.round(bary[::7])
    a, b, c = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    target = a + bary[:, :1] * (b - a) + bary[:, 1:] * (c - a)
    rays[:, 3:] = target - rays[:, :3]
    hit, tuv, nrm, pt = rt.dbg_hit_triangle(rays, tris, math_mode=mode)
    nh = 0
    for i in range(n):
        ray = orc.ray_make(rays[i, :3], rays[i, 3:], True, contract)
        h, t, u, v = orc.hit_triangle(ray, a[i], b[i], c[i], contract, 0)
        assert h == bool(hit[i]), i
        if h:
            nh += 1
            assert np.array_equal(u32(tuv[i]), u32([t, u, v])), i
        assert np.array_equal(u32(nrm[i]), u32(orc.triangle_normal(a[i], b[i], c[i], contract))), i
    assert 500 < nh < n - 500


def test_midrange_sqrt_and_reciprocal_are_exact_for_every_float_of_their_range(rt):
    """normalize skips the scaling/special-case steps of the generic sqrt and division when the
    squared length is in [2^-96, 2^96]: proven equal by enumeration of all 1.6e9 operands."""
    from raytracertest_amd import api
    seen, bad_sqrt, bad_rcp, example = api.dbg_check_midrange()
    assert seen == 0x6F800000 - 0x0F800000 + 1
    assert (bad_sqrt, bad_rcp) == (0, 0), "first mismatching operand bits: 0x%08x" % example


def test_sincos_bitexact(rt, orc):
    x = np.concatenate([np.linspace(0, 6.2831309, 50001), np.linspace(-40, 40, 20001),
                        [0.0, 1e-30, 1.5707964, 3.1415927, 6.2831855]]).astype(np.float32)
    s, c = rt.dbg_sincos(x)
    ref = np.array([orc.sincos(v) for v in x], np.float32)
    assert np.array_equal(u32(s), u32(ref[:, 0])) and np.array_equal(u32(c), u32(ref[:, 1]))


def test_uniform_stream_bitexact(rt, orc):
    states = np.array([orc.rng_init(seed, sub) for seed, sub in [(1, 0), (1, 1), (7, 2073599), (2**40 + 3, 99)]])
    out, st = rt.dbg_uniform(states, 64)
    for i in range(states.shape[0]):
        s = states[i].copy()
        ref = np.array([orc.rng_uniform(s) for _ in range(64)], np.float32)
        assert np.array_equal(u32(out[i]), u32(ref))
        assert np.array_equal(st[i], s)
    assert out.min() > 0.0 and out.max() <= 1.0


# ------------------------------------------------------------------ frame-level parity
SCENES = {}


def scene(name):
    from raytracertest_amd import scenes
    if name not in SCENES:
        SCENES[name] = {"demo3": scenes.demo3, "kat": scenes.kat_triangle, "cornell": scenes.cornell32,
                        "rand300": lambda: scenes.random_triangles(300, 777)}[name]()
    return SCENES[name]


def run_pair(rt, orc, W, H, scn, iterations, samples, *, mode=0, angles=(0.0, 0.0), fov=70.0, focal=3.0,
             aperture=0.05, seed=1, spheres=None, **kw):
    import raytracertest_amd as R
    g = R.RayTracer((W, H), (0, 0, 0), angles, fov, focal, aperture, seed=seed, math_mode=mode, **kw)
    o = orc.OracleTracer(W, H, angles, fov, focal, aperture, seed=seed, contract=1 - mode, nthreads=8)
    if scn is not None:
        assert g.UploadScene(scn) and o.upload_scene(scn)
    if spheres is not None:
        g.UploadSpheres(spheres)
        o.upload_spheres(spheres)
    assert np.array_equal(g.RngStates(), o.rng), "RNG states after init"
    g.Trace(iterations, samples, 0)
    assert g.Wait()
    o.trace(iterations, samples)
    return g, o


def assert_frame_equal(g, o):
    assert np.array_equal(g.SampleCounts(), o.counts)
    assert np.array_equal(g.RngStates(), o.rng), "RNG states after trace"
    gr, orr = g.RenderBuffer(), o.render
    bad = np.argwhere(u32(gr) != u32(orr))
    assert bad.size == 0, "first differing render values at %s: %s vs %s" % (
        bad[:4].tolist(), gr[tuple(bad[0])], orr[tuple(bad[0])])
    assert np.array_equal(g.Image(), o.image)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,W,H,it,spp", [("demo3", 38, 21, 3, 1), ("cornell", 67, 41, 2, 5),
                                             ("rand300", 70, 33, 1, 16), ("kat", 16, 16, 1, 2)])
def test_trace_bitexact(rt, orc, mode, name, W, H, it, spp):
    g, o = run_pair(rt, orc, W, H, scene(name), it, spp, mode=mode)
    assert_frame_equal(g, o)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 70), (70, 1), (7, 3), (33, 9), (257, 5), (5, 129)])
def test_degenerate_and_ragged_frame_sizes(rt, orc, W, H):
    """Frames smaller than a tile, one pixel wide/high, and sizes that leave partial tiles on both axes."""
    g, o = run_pair(rt, orc, W, H, scene("cornell"), 3, 2)
    assert_frame_equal(g, o)
    g, o = run_pair(rt, orc, W, H, scene("rand300"), 1, 3, nearest_hit=False)
    assert_frame_equal(g, o)


@pytest.mark.parametrize("cam", [dict(fov=180.0), dict(fov=179.9), dict(fov=0.01), dict(fov=0.0), dict(focal=0.0), dict(focal=1e30),
                                 dict(aperture=1e6), dict(focal=0.0, aperture=0.0), dict(fov=360.0), dict(fov=-70.0),
                                 dict(focal=float("inf")), dict(aperture=float("nan"))])
@pytest.mark.parametrize("mode", [0, 1])
def test_extreme_camera_parameters_follow_the_oracle_bit_for_bit(rt, orc, cam, mode):
    """Degenerate cameras (infinite / zero / NaN / negative parameters): whatever the arithmetic yields --
    inf, NaN, all-miss -- the HIP path and the oracle yield the same values (a NaN matches any NaN: x86 and
    gfx950 propagate different payloads), with the tile classification switched off by its own non-finite
    guard where needed."""
    kw = dict(fov=70.0, focal=3.0, aperture=0.05); kw.update(cam)
    for name in ("cornell", "rand300"):
        g, o = run_pair(rt, orc, 40, 24, scene(name), 2, 3, mode=mode, **kw)
        assert np.array_equal(g.SampleCounts(), o.counts) and np.array_equal(g.RngStates(), o.rng)
        gr, orr = g.RenderBuffer(), o.render
        same = (u32(gr) == u32(orr)) | (np.isnan(gr) & np.isnan(orr))
        assert same.all(), "first differing render values at %s" % np.argwhere(~same)[:4].tolist()
        assert np.array_equal(g.Image(), o.image)


def test_degenerate_spheres_follow_the_oracle(rt, orc):
    """Radius 0, negative and huge radii, a sphere around the lens, non-finite centres."""
    sph = np.array([[0.0, 0.0, -5.0, 0.0], [0.5, 0.2, -4.0, -0.7], [0.0, 0.0, 0.0, 2.0], [0.0, 0.0, -50.0, 45.0],
                    [np.inf, 0.0, -3.0, 1.0], [np.nan, 0.0, -3.0, 1.0], [0.3, -0.4, -2.0, 1e-30]], np.float32)
    import raytracertest_amd as R
    for nearest in (False, True):
        for mode in (0, 1):
            g = R.RayTracer((48, 30), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=mode, nearest_hit=nearest)
            o = orc.OracleTracer(48, 30, (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, contract=1 - mode, nthreads=8, hit_mode=int(nearest))
            g.UploadScene(scene("cornell")); o.upload_scene(scene("cornell"))
            g.UploadSpheres(sph); o.upload_spheres(sph)
            g.Trace(2, 2, 0); assert g.Wait(); o.trace(2, 2)
            gr, orr = g.RenderBuffer(), o.render
            same = (u32(gr) == u32(orr)) | (np.isnan(gr) & np.isnan(orr))
            assert same.all(), (nearest, mode, np.argwhere(~same)[:4].tolist())
            assert np.array_equal(g.Image(), o.image) and np.array_equal(g.RngStates(), o.rng)


def test_several_tracers_render_concurrently(rt, orc):
    """Four tracers (own streams, own render threads) tracing at the same time on one device."""
    import raytracertest_amd as R
    specs = [("cornell", 64, 40, 5, 2, 3), ("rand300", 50, 30, 3, 3, 0), ("demo3", 38, 21, 40, 1, 10), ("cornell", 33, 57, 2, 4, 1)]
    pairs = []
    for i, (name, W, H, it, spp, upd) in enumerate(specs):
        g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=20 + i)
        o = orc.OracleTracer(W, H, (0.0, 0.0), 70.0, 3.0, 0.05, seed=20 + i, nthreads=4)
        g.UploadScene(scene(name)); o.upload_scene(scene(name))
        g.SetUpdateCallback(lambda img, size: None)
        pairs.append((g, o, it, spp, upd))
    for rep in range(3):
        for g, o, it, spp, upd in pairs:
            g.Trace(it, spp, upd)                       # all four render threads run now
        for g, o, it, spp, upd in pairs:
            assert g.Wait()
            o.trace(it, spp)
            assert_frame_equal(g, o)


def test_empty_scene_is_all_background(rt, orc):
    g, o = run_pair(rt, orc, 45, 31, None, 2, 3)
    assert_frame_equal(g, o)
    assert (g.SampleCounts() == 6).all()


def test_trace_rotated_camera_and_params(rt, orc):
    import raytracertest_amd as R
    W, H = 64, 40
    g = R.RayTracer((W, H), (1, 2, 3), (0.2, -0.3), 55.0, 4.0, 0.2, seed=9)
    o = orc.OracleTracer(W, H, (0.2, -0.3), 55.0, 4.0, 0.2, seed=9, nthreads=8)
    scn = scene("cornell")
    g.UploadScene(scn); o.upload_scene(scn)
    g.RotateCamera((0.1, 3.0)); o.rotate_camera((0.1, 3.0))          # look backwards-ish: demo-like
    g.SetCameraParameters(80.0, 2.5, 0.0); o.set_camera_parameters(80.0, 2.5, 0.0)
    g.Trace(2, 3, 0); assert g.Wait(); o.trace(2, 3)
    assert_frame_equal(g, o)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_samples_in_flight_invariance(rt, orc, K):
    g, o = run_pair(rt, orc, 45, 27, scene("rand300"), 1, 7, samples_in_flight=K)
    assert_frame_equal(g, o)


def test_filter_off_equals_filter_on(rt, orc):
    g, o = run_pair(rt, orc, 61, 35, scene("rand300"), 1, 8, no_filter=True)
    assert_frame_equal(g, o)


def test_lds_chunking_invariance(rt, orc):
    g, o = run_pair(rt, orc, 40, 24, scene("rand300"), 2, 4, lds_chunk=64, no_binning=True)   # 300 triangles -> 5 chunks
    assert g.Info()["lds_chunk"] == 64 and g.Info()["lds_bytes"] == 64 * 36
    assert_frame_equal(g, o)


def test_sphere_config_c2_small(rt, orc):
    from raytracertest_amd import scenes
    _, sph = scenes.sphere1()
    g, o = run_pair(rt, orc, 96, 96, None, 1, 1, focal=10.0, aperture=0.0, spheres=sph)
    assert_frame_equal(g, o)
    img = g.Image()
    assert (img[48, 48] & 0xFF) > 200          # centre of the sphere: normal ~ +z -> blue channel high


def test_mixed_triangles_and_spheres(rt, orc):
    sph = np.array([[0, 0, -2.5, 0.4], [0.5, 0.3, -2.0, 0.2]], np.float32)
    g, o = run_pair(rt, orc, 50, 30, scene("cornell"), 1, 3, spheres=sph)
    assert_frame_equal(g, o)


def test_row_band_partition_invariance(rt, orc):
    import raytracertest_amd as R
    W, H = 53, 37
    scn = scene("rand300")
    whole, o = run_pair(rt, orc, W, H, scn, 2, 3)
    full = whole.RenderBuffer()
    bands = [(0, 10), (10, 9), (19, 18)]
    for r0, n in bands:
        b = R.RayTracer((W, n), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, full_height=H, row_begin=r0)
        b.UploadScene(scn)
        b.Trace(2, 3, 0); assert b.Wait()
        assert np.array_equal(u32(b.RenderBuffer()), u32(full[r0:r0 + n]))
        assert np.array_equal(b.RngStates(), whole.RngStates()[r0:r0 + n])
        assert np.array_equal(b.Image(), whole.Image()[r0:r0 + n])


def test_mode_tolerance(rt, orc):
    """The fp32 tolerance between the two arithmetic modes (what north_star's 'stated
    per-channel fp32 tolerance' has to cover: the reference's GPU build fuses, its host
    build does not).  Stated: per channel |a-b| <= 2e-6 * samples on pixels whose hit/miss
    pattern agrees; at most 0.5% of pixels may flip a silhouette sample; BGRA8 within +-1
    on the agreeing pixels."""
    import raytracertest_amd as R
    W, H, spp = 96, 54, 8
    res = []
    for mode in (0, 1):
        g = R.RayTracer((W, H), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=1, math_mode=mode)
        g.UploadScene(scene("cornell"))
        g.Trace(1, spp, 0); assert g.Wait()
        res.append((g.RenderBuffer(), g.Image()))
    d = np.abs(res[0][0] - res[1][0]).max(axis=2)
    agree = d <= 2e-6 * spp
    assert agree.mean() >= 0.995
    ch = lambda im, s: ((im >> s) & 0xFF).astype(np.int32)
    for s in (0, 8, 16):
        assert np.abs(ch(res[0][1], s) - ch(res[1][1], s))[agree].max() <= 1


# ------------------------------------------------------------------ API behaviour (RayTracerImpl.cu:69-87,236-315)
def test_callbacks_cadence_and_stop(rt):
    import raytracertest_amd as R
    g = R.RayTracer((38, 21), (0, 0, 0), (0, 0), 70.0, 10.0, 4.0, seed=3)
    g.UploadScene(scene("demo3"))
    updates, finished = [], []
    g.SetUpdateCallback(lambda img, size: updates.append((size, int(img.shape[0]), int(img.shape[1]))))
    g.SetFinishedCallback(lambda img, size: finished.append((size, img.copy())))
    g.Trace(10, 1, 3)                      # i = 3, 6, 9 -> three updates (i > 0 && i % 3 == 0)
    assert g.Wait()
    assert updates == [(38 * 21 * 4, 21, 38)] * 3 and len(finished) == 1
    assert np.array_equal(finished[0][1], g.Image())
    assert (g.SampleCounts() == 10).all()
    # updateInterval 0 -> no updates (RayTracerImpl.cu:256)
    updates.clear(); finished.clear()
    g.Trace(4, 2, 0); assert g.Wait()
    assert updates == [] and len(finished) == 1 and (g.SampleCounts() == 8).all()
    # a stopped run fires no finished callback (:280-284)
    finished.clear()
    g.SetUpdateCallback(lambda img, size: g.Stop())
    g.Trace(1000, 1, 1)
    assert g.Wait() is False and finished == []
    assert 0 < int(g.SampleCounts().max()) < 1000


def test_upload_scene_rejects_bad_sizes(rt):
    import raytracertest_amd as R
    g = R.RayTracer((16, 16), seed=1)
    assert g.UploadScene(scene("demo3"))
    assert g.UploadScene(np.zeros((4, 4), np.float32)) is False        # :121-125, previous scene kept
    assert g.UploadScene(np.zeros((2, 4), np.float32)) is False
    assert g.Info()["n_tris"] == 3 and "invalid triangle list" in g.LastError()


def test_resize_recreates_state(rt, orc):
    import raytracertest_amd as R
    g = R.RayTracer((20, 10), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=5)
    g.UploadScene(scene("cornell"))
    g.Trace(1, 2, 0); assert g.Wait()
    g.Resize((33, 19))
    o = orc.OracleTracer(33, 19, (0, 0), 70.0, 3.0, 0.05, seed=5, nthreads=4)
    o.upload_scene(scene("cornell"))
    assert np.array_equal(g.RngStates(), o.rng)
    g.Trace(1, 3, 0); assert g.Wait(); o.trace(1, 3)
    assert_frame_equal(g, o)


def test_consecutive_traces_continue_the_stream(rt, orc):
    """RNG states persist across Trace calls (never re-seeded): two identical Trace calls
    give different images, and the oracle follows."""
    g, o = run_pair(rt, orc, 40, 22, scene("cornell"), 1, 2)
    first = g.RenderBuffer().copy()
    g.Trace(1, 2, 0); assert g.Wait(); o.trace(1, 2)
    assert_frame_equal(g, o)
    assert not np.array_equal(first, g.RenderBuffer())


def test_candidate_lists_reused_across_iterations_follow_camera_and_scene_changes(rt, orc):
    """Iterations 2..n of a Trace reuse the tile candidate lists of iteration 1 (small scenes).
    The lists must be rebuilt after anything they depend on changes between Traces: camera
    rotation, lens parameters, a new scene with the same triangle count, a resize."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    W, H = 70, 44
    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=4)
    o = orc.OracleTracer(W, H, (0.0, 0.0), 70.0, 3.0, 0.05, seed=4, nthreads=8)
    a, b = scenes.random_triangles(120, 1), scenes.random_triangles(120, 2)
    g.UploadScene(a); o.upload_scene(a)
    g.Trace(3, 2, 0); assert g.Wait(); o.trace(3, 2); assert_frame_equal(g, o)
    g.RotateCamera((0.3, -0.7)); o.rotate_camera((0.3, -0.7))
    g.Trace(3, 1, 0); assert g.Wait(); o.trace(3, 1); assert_frame_equal(g, o)
    g.SetCameraParameters(40.0, 6.0, 0.4); o.set_camera_parameters(40.0, 6.0, 0.4)
    g.Trace(2, 3, 0); assert g.Wait(); o.trace(2, 3); assert_frame_equal(g, o)
    g.UploadScene(b); o.upload_scene(b)                      # same count, different triangles
    g.Trace(4, 1, 0); assert g.Wait(); o.trace(4, 1); assert_frame_equal(g, o)
    g.Resize((W + 9, H - 5))
    o = orc.OracleTracer(W + 9, H - 5, (0.3, -0.7), 40.0, 6.0, 0.4, seed=4, nthreads=8)
    o.upload_scene(b)
    g.Trace(3, 2, 0); assert g.Wait(); o.trace(3, 2); assert_frame_equal(g, o)


@pytest.mark.parametrize("name,n_it,spp", [("cornell", 9, 2), ("rand300", 5, 3), ("demo3", 70, 1)])
def test_fused_iterations_equal_separate_launches(rt, orc, name, n_it, spp):
    """Iterations nobody observes run as one launch: same bits as one launch per iteration
    (rt_tracer_launch), as the oracle's loop, and with the update cadence unchanged."""
    import raytracertest_amd as R
    W, H = 50, 30
    scn = scene(name)
    a = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=12)
    b = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=12)
    c = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=12)
    o = orc.OracleTracer(W, H, (0.0, 0.0), 70.0, 3.0, 0.05, seed=12, nthreads=8)
    for g in (a, b, c):
        assert g.UploadScene(scn)
    o.upload_scene(scn)
    a.TraceEnqueue(n_it, spp); a.Sync()                      # fused groups
    for i in range(n_it):                                    # one launch per iteration
        b.Launch(spp, clear_first=(i == 0), emit_image=(i + 1 == n_it))
    b.Sync()
    updates = []
    c.SetUpdateCallback(lambda img, size: updates.append(img.copy()))
    c.Trace(n_it, spp, 4); assert c.Wait()                   # fused between update points
    o.trace(n_it, spp)
    for g in (a, b, c):
        assert np.array_equal(u32(g.RenderBuffer()), u32(o.render))
        assert np.array_equal(g.SampleCounts(), o.counts) and np.array_equal(g.RngStates(), o.rng)
        assert np.array_equal(g.Image(), o.image)
    assert len(updates) == (n_it - 1) // 4


def test_fused_launch_argument_checks(rt):
    import raytracertest_amd as R
    g = R.RayTracer((20, 12), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=3)
    g.UploadScene(scene("cornell"))
    n = g.FusedIterations(4)
    assert n == 16 and g.FusedIterations(64) == 1 and g.FusedIterations(100) == 1     # <= 64 samples per pixel per launch
    g.Launch(4, clear_first=True, emit_image=True, iterations=n); g.Sync()
    assert (g.SampleCounts() == 4 * n).all()
    with pytest.raises(R.RtError):
        g.Launch(4, iterations=n + 1)
    assert "exceed" in g.LastError()
    plain = R.RayTracer((20, 12), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=3, no_binning=True)
    assert plain.FusedIterations(1) == 1                      # only the default (classified, filtered) kernels fuse


def test_image_mirror_receives_the_emitted_image(rt):
    """rt_tracer_set_image_mirror: the emitting launch writes the BGRA8 image into a caller-owned device
    buffer too (what the multi-GPU step uses as the gather's send buffer).  The caller-owned buffer here is the image
    buffer of a second, idle tracer of the same size."""
    import raytracertest_amd as R
    from raytracertest_amd.api import BUF_IMAGE
    W, H = 70, 37
    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=3)
    g.UploadScene(scene("cornell"))
    other = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=4)
    assert not other.Image().any()
    g.SetImageMirror(other.DevicePointer(BUF_IMAGE))
    g.TraceEnqueue(3, 2); g.Sync()
    assert g.Image().any() and np.array_equal(other.Image(), g.Image())
    g.SetImageMirror(None)
    before = other.Image()
    g.TraceEnqueue(1, 2); g.Sync()
    assert np.array_equal(before, other.Image()) and not np.array_equal(before, g.Image())
    g.close(); other.close()


def test_trace_enqueue_matches_trace(rt, orc):
    g, o = run_pair(rt, orc, 48, 28, scene("rand300"), 2, 4)
    import raytracertest_amd as R
    h = R.RayTracer((48, 28), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    h.UploadScene(scene("rand300"))
    h.TraceEnqueue(2, 4); h.Sync()
    assert np.array_equal(u32(h.RenderBuffer()), u32(g.RenderBuffer()))
    assert np.array_equal(h.Image(), g.Image())
    ms, n = h.KernelTime()
    assert 1 <= n <= 2 and ms > 0.0        # sampled launches (every 16th carries events; the first always does)


# ------------------------------------------------------------------ per-tile classification (BIN) vs full scan
def _bin_pair(W, H, scn, it, spp, mode=0, **cam):
    import raytracertest_amd as R
    out = []
    for no_binning in (False, True):
        g = R.RayTracer((W, H), (0, 0, 0), cam.get("angles", (0.0, 0.0)), cam.get("fov", 70.0),
                        cam.get("focal", 3.0), cam.get("aperture", 0.05), seed=cam.get("seed", 1),
                        math_mode=mode, no_binning=no_binning)
        assert g.UploadScene(scn)
        g.Trace(it, spp, 0)
        assert g.Wait()
        out.append((g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image()))
    a, b = out
    bad = np.argwhere(u32(a[0]) != u32(b[0]))
    assert bad.size == 0, "binning changed %d render values, first at %s" % (bad.shape[0], bad[0].tolist())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    return a


def _stress_scene(kind, n, seed):
    from raytracertest_amd import scenes
    rng = np.random.default_rng(seed)
    if kind == "around_origin":      # triangles all around (and through) the lens: negative t, loose bounds
        c = rng.uniform(-1.5, 1.5, (n, 1, 3))
        t = c + rng.uniform(-0.6, 0.6, (n, 3, 3))
    elif kind == "big_overlapping":  # every tile sees hundreds of candidates -> multi-round lists
        c = np.concatenate([rng.uniform(-0.5, 0.5, (n, 1, 2)), rng.uniform(-9, -2, (n, 1, 1))], axis=2)
        t = c + rng.uniform(-6, 6, (n, 3, 3)) * np.array([1, 1, 0.05])
    elif kind == "grazing":          # nearly edge-on to the view direction: det ~ 0
        c = np.concatenate([rng.uniform(-2, 2, (n, 1, 2)), rng.uniform(-8, -2, (n, 1, 1))], axis=2)
        off = rng.uniform(-1, 1, (n, 3, 3))
        off[:, :, 0] *= 1e-4         # flattened in x: planes contain the z axis direction
        t = c + off
    elif kind == "scales":           # tiny and huge triangles, far and near
        s = 10.0 ** rng.uniform(-4, 3, (n, 1, 1))
        c = rng.uniform(-1, 1, (n, 1, 3)) * s + np.array([0, 0, -3.0])
        t = c + rng.uniform(-1, 1, (n, 3, 3)) * s
    else:
        raise KeyError(kind)
    return scenes._tri_rows(t)


@pytest.mark.parametrize("kind,n", [("around_origin", 400), ("big_overlapping", 700), ("big_overlapping", 3000),
                                    ("grazing", 500), ("scales", 500), ("scales", 5000)])
@pytest.mark.parametrize("mode", [0, 1])
def test_binning_equals_full_scan_stress(rt, kind, n, mode):
    _bin_pair(72, 40, _stress_scene(kind, n, 11), 1, 6, mode=mode, aperture=0.08, focal=3.0)


@pytest.mark.parametrize("cam", [dict(aperture=0.0, focal=3.0), dict(aperture=4.0, focal=10.0),
                                 dict(aperture=0.3, focal=0.5, fov=120.0), dict(aperture=0.05, focal=3.0, angles=(0.4, 2.5)),
                                 dict(aperture=-0.2, focal=-2.0), dict(aperture=0.05, focal=3.0, fov=5.0)])
def test_binning_equals_full_scan_cameras(rt, cam):
    from raytracertest_amd import scenes
    _bin_pair(64, 48, scenes.random_triangles(1500, 99), 1, 5, **cam)
    _bin_pair(40, 24, scene("cornell"), 2, 3, **cam)


def test_macro_level_on_off_and_overflow_fallback(rt, monkeypatch):
    """Large scenes: macro-tile lists on (default) = off = full scan; a macro list that overflows its
    capacity falls back to scanning the scene for that macro tile."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    scn = scenes.random_triangles(6000, 31)
    def run(**kw):
        g = R.RayTracer((200, 136), (0, 0, 0), (0.1, -0.05), 70.0, 3.0, 0.05, seed=8, **kw)
        assert g.UploadScene(scn)
        g.Trace(2, 5, 0); assert g.Wait()
        return g.RenderBuffer().view(np.uint32).copy(), g.RngStates().copy()
    ref = run(no_binning=True)
    on = run()
    off = run(no_macro_bins=True)
    monkeypatch.setenv("RT_MI355X_MACRO_CAP", "40")
    tiny = run()
    monkeypatch.delenv("RT_MI355X_MACRO_CAP")
    for other in (on, off, tiny):
        assert np.array_equal(ref[0], other[0]) and np.array_equal(ref[1], other[1])


def test_large_scene_three_level_classification_equals_full_scan(rt):
    """60 000 triangles: macro tile -> block -> wave tile lists (with multi-round wave lists) = full scan."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    scn = scenes.random_triangles(60000, 4711)
    out = []
    for kw in (dict(), dict(no_binning=True)):
        g = R.RayTracer((160, 96), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=3, **kw)
        assert g.UploadScene(scn)
        g.Trace(1, 5, 0); assert g.Wait()
        out.append((g.RenderBuffer().view(np.uint32).copy(), g.RngStates().copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_binning_with_degenerate_and_nonfinite_triangles(rt):
    from raytracertest_amd import scenes
    scn = scenes.random_triangles(200, 5).copy()
    t = scn.reshape(-1, 3, 4)
    t[3, 1] = t[3, 0]                      # zero-area (two equal vertices)
    t[7, :, :3] = t[7, 0, :3]              # a point
    t[11, 2, 0] = np.nan
    t[13, 1, 2] = np.inf
    t[17, :, :3] *= 1e30
    t[19, :, :3] *= 1e-30
    a = _bin_pair(56, 32, scn, 1, 4)
    # NaN/inf vertices never produce a hit in the reference arithmetic either; image stays finite
    assert np.isfinite(a[0]).all()


def test_binning_candidate_lists_are_short_on_the_bench_scenes(rt):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    g = R.RayTracer((480, 270), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=1)
    g.UploadScene(scenes.cornell32())
    st = g.TraceStats(4)
    waves = (480 // 8) * ((270 + 7) // 8)
    assert st["bin_rounds"] == waves                      # one classification per wave, list fits
    assert st["bin_candidates"] / waves < 16              # of 32 triangles
    g = R.RayTracer((480, 270), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=1)
    g.UploadScene(scenes.random_triangles(10000, 12345))
    st = g.TraceStats(4)
    assert st["bin_rounds"] <= 2 * waves and st["bin_candidates"] / st["bin_rounds"] < 200   # of 10 000


def test_launch_building_block_and_progressive_driver(rt, orc):
    """rt_tracer_launch + dist.progressive_trace on one GPU == rt_tracer_trace == oracle."""
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    from raytracertest_amd.dist import RowBandJob
    cfg = dict(width=48, height=28, iterations=1, samples=2, angles=(0.0, 0.0), fov=70.0, focal=3.0, aperture=0.05, seed=1)
    job = RowBandJob(cfg, scenes.cornell32(), np.zeros((0, 4), np.float32))
    updates, finished = [], []
    ok = job.trace_progressive(7, 2, 3, on_update=lambda f: updates.append(f.copy()),
                               on_finished=lambda f: finished.append(f.copy()))
    assert ok and len(updates) == 2 and len(finished) == 1
    o = orc.OracleTracer(48, 28, (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, nthreads=4)
    o.upload_scene(scenes.cornell32())
    o.trace(7, 2)
    assert np.array_equal(finished[0], o.image) and np.array_equal(job.tracer.RenderBuffer().view(np.uint32), o.render.view(np.uint32))
    stop = {"n": 0}
    ok = job.trace_progressive(50, 1, 2, on_update=lambda f: stop.__setitem__("n", stop["n"] + 1),
                               on_finished=lambda f: finished.append(None), stop_requested=lambda: stop["n"] >= 2)
    assert not ok and len(finished) == 1 and int(job.tracer.SampleCounts().max()) == 5    # launches 0..4, then agreed stop
    job.close()


_INTEROP = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import raytracertest_amd as R
from raytracertest_amd import scenes
from raytracertest_amd.api import BUF_IMAGE
g = R.RayTracer((96, 54), (0, 0, 0), (0, 0), 70.0, 3.0, 0.05, seed=1)
g.UploadScene(scenes.cornell32())
assert g.Stream() != 0
ext = torch.cuda.ExternalStream(g.Stream(), device=torch.device("cuda", 0))
tile = torch.zeros((54, 96), dtype=torch.int32, device="cuda")
ev = torch.cuda.Event()
for _ in range(3):
    g.TraceEnqueue(1, 4)
    g.CopyToDeviceAsync(BUF_IMAGE, tile.data_ptr(), tile.numel() * 4)
    ev.record(ext)
    torch.cuda.current_stream().wait_event(ev)
    doubled = tile * 2                       # consumer on torch's stream
torch.cuda.synchronize()
g.Sync()
img = g.Image()
assert np.array_equal(tile.cpu().numpy().view(np.uint32), img)
assert np.array_equal(doubled.cpu().numpy(), (img.view(np.int32) * 2))
print("INTEROP_OK")
'''


def test_stream_interop_for_the_overlapped_gather(rt):
    """Stream interop for an external driver that orders its OWN device work behind the tracer (rt_tracer_stream):
    the tracer's HIP stream wrapped as a torch ExternalStream, an async copy ordered behind the trace, an
    event making torch's stream wait for it.  (The library's own tile gather does the same with its gather streams.)
    In a process of its own: bringing torch.cuda up on a fresh box can take minutes (the image pages in), which must not
    look like a hung GPU test; if it does not come up within four minutes the test is skipped, not failed."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        out = subprocess.run([sys.executable, "-c", _INTEROP % root], capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.skip("torch.cuda did not come up within 240 s on this box")
    assert out.returncode == 0 and "INTEROP_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_randomised_campaign_default_kernel_equals_plain_full_scan(rt):
    """tools/stress_binning.py: random scenes / scales / cameras / sizes / modes; the default
    kernel (classification + ballot early-outs) must equal the reference-order full scan bit for
    bit.  (18 400 configurations were run once for round 1: 0 mismatches; 250 here.)"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_binning.py"), "250", "31337"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "250 configurations, 0 mismatches" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_randomised_campaign_hip_equals_oracle(rt):
    """tests/stress_oracle.py: random scenes, spheres, cameras, row bands, seeds, both arithmetic
    modes and both hit rules -- HIP vs oracle, bit for bit (21 500 configurations run once for
    round 1: 0 mismatches; 300 here)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "stress_oracle.py"), "300", "424242"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "300 configurations, 0 mismatches" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_two_rank_rehearsal_of_the_multi_gpu_driver(rt):
    """The one-process-per-GPU job of dist.RowBandJob with two processes on this one GPU (tests/dist_rehearsal.py: the
    tiles travel through the test's host-staged exchange, RCCL refuses two ranks per device), then bench.py's N > 1
    line WITHOUT a launcher: one process, the library shards the frame itself (rt_tracer_create_multi)."""
    import subprocess, sys, os, socket, json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(root, "tests", "dist_rehearsal.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "dist_rehearsal ok: world=2" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    n_dev = rt.device_count()
    if n_dev < 2:                  # two bands on one device are a rehearsal, not a scaling run: bench.py refuses unless told so
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2"],
                             capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 2 and "--allow-alias" in out.stderr and not out.stdout.strip(), out.stdout[-2000:] + out.stderr[-2000:]
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--allow-alias",
                          "--full"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == min(2, n_dev) and line["bands"] == 2      # n_gpus = DISTINCT devices that traced
    assert line["scaling"] == "weak" and line["value"] > 0 and "cpu_baseline" not in line
    assert "gather_ms" in line and line["config"]["devices"] == [k % rt.device_count() for k in range(2)]
    c5 = line["c5_strong"]       # BASELINE configs[4] beside the weak headline: one 3840x2160 frame, 256 spp, two row bands
    assert c5["scaling"] == "strong" and c5["value"] > 0 and "2 row bands" in c5["image"] and "gather_ms" in c5
    assert line["roofline"]["frac"] <= 1.0 and line["roofline"]["frac_wall"] <= line["roofline"]["frac"] * 1.5


def test_api_soak_against_a_running_render_thread(rt):
    """Random Trace/Stop/Resize/camera/scene calls while the render thread runs fused launches and
    pipelined update hand-offs: no hang, no recorded error, and a final Trace still matches the oracle."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "soak_api.py"), "400", "11"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "last error ''" in out.stdout and "final parity True" in out.stdout, out.stdout
