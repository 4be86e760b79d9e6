"""Ray queries on the device (RayTracer.Intersect / Pick / FocusAt, rt_tracer_intersect_device): bit for bit against a scan
in upload order with the oracle's HitTriangle and ray-sphere test, under both arithmetic modes, both hit rules, both scene
layouts and every K; pick rays against the oracle's pinhole camera; FocusAt against the oracle's frame; no interference
with a running Trace; the torch path and its ordering against uploads; the C++ class and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

from query_expect import HIT_DTYPE, adversarial_rays, adversarial_scene, edge_rows, expected_hits, same_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytracertest_amd", "lib")
pytestmark = pytest.mark.gpu

SPHERES = np.array([[0.5, 0.3, -6.0, 1.0], [0.5, 0.3, -6.0, 1.0], [-1.5, 1.0, -4.0, 0.7], [0.0, 0.0, 4.0, 1.5]], np.float32)


def _tracer(math_mode=0, nearest=False, K=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, nearest_hit=nearest,
                       samples_in_flight=K, **kw)


def oc(orc, math_mode):
    """The oracle's arithmetic for a tracer's math_mode (RT_MATH_FMA = 0, RT_MATH_STRICT = 1)."""
    return orc.FMA if math_mode == 0 else orc.STRICT


@pytest.mark.parametrize("n_tris", [1, 37, 300])
@pytest.mark.parametrize("spheres", [False, True])
def test_intersect_bit_exact_every_mode_layout_and_K(orc, n_tris, spheres):
    rows = adversarial_scene(n_tris, seed=n_tris)
    rays = adversarial_rays(rows, 160 if n_tris == 300 else 400, seed=n_tris + 1)
    sph = SPHERES if spheres else None
    for mm in (0, 1):
        contract = oc(orc, mm)
        for nearest in (False, True):
            exp = expected_hits(orc, rays, rows, sph, contract, nearest)
            assert (exp["prim"] >= 0).any() and (exp["prim"] < 0).any()
            if not nearest:
                assert (exp["t"][exp["prim"] >= 0] < 0).any() or n_tris < 8     # hits behind the origin are kept
            for edges in (False, True):
                for K in (1, 2, 4):
                    g = _tracer(mm, nearest, K)
                    assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
                    if spheres:
                        g.UploadSpheres(SPHERES)
                    got_all = g.Intersect(rays)
                    for n in (rays.shape[0], 1, 255, 257):             # partial blocks
                        got = got_all if n == rays.shape[0] else g.Intersect(rays[:n])
                        assert got.dtype == HIT_DTYPE
                        assert same_hits(got, exp[:n]), (mm, nearest, edges, K, n,
                                                          np.nonzero(got.view(np.uint32).reshape(-1, 4) != exp[:n].view(np.uint32).reshape(-1, 4))[0][:5])
                    if edges and K == 4:                                # the edge layout's shading of the winner
                        for i in range(0, rays.shape[0], 37):
                            full = orc.radiance(rays[i], edge_rows(rows), sph, contract, int(nearest), layout=1)
                            p = int(got_all[i]["prim"])
                            if 0 <= p < n_tris:
                                one = orc.radiance(rays[i], edge_rows(rows)[3 * p:3 * p + 3], None, contract, int(nearest), layout=1)
                                assert np.array_equal(full, one)
                    g.close()


def test_no_scene_and_empty_batch():
    g = _tracer()
    rays = np.array([[0, 0, 0, 0, 0, -1]] * 5, np.float32)
    h = g.Intersect(rays)
    assert (h["prim"] == -1).all() and (h["t"] == 0).all() and (h["u"] == 0).all() and (h["v"] == 0).all()
    assert g.Intersect(np.zeros((0, 6), np.float32)).shape == (0,)
    assert g.Pick(np.zeros((0, 2), np.uint32)).shape == (0,)


def test_at_scale_K_agree_and_match_radiance(orc):
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    rng = np.random.default_rng(7)
    n = 1 << 20
    org = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    org[:, 2] = rng.uniform(-2, 2, n)
    tgt = rows.reshape(-1, 3, 4)[rng.integers(0, 10000, n), :, :3].mean(axis=1) + rng.normal(0, 0.2, (n, 3)).astype(np.float32)
    rays = np.ascontiguousarray(np.c_[org, tgt - org].astype(np.float32))
    res = []
    for K in (1, 2, 4):
        g = _tracer(0, False, K)
        assert g.UploadScene(rows)
        res.append(g.Intersect(rays))
        g.close()
    assert same_hits(res[0], res[1]) and same_hits(res[0], res[2])
    h = res[0]
    assert (h["prim"] >= 0).mean() > 0.3
    tri = rows.reshape(-1, 3, 4)
    for i in rng.choice(n, 2000, replace=False):
        p = int(h[i]["prim"])
        full = orc.radiance(rays[i], rows, None, orc.FMA, 0)
        if p < 0:
            assert np.array_equal(full, orc.radiance(rays[i], None, None, orc.FMA, 0))
            continue
        assert np.array_equal(full, orc.radiance(rays[i], tri[p].reshape(-1, 4), None, orc.FMA, 0))
        hit, t, u, v = orc.hit_triangle(rays[i], tri[p, 0, :3], tri[p, 1, :3], tri[p, 2, :3], orc.FMA, 0)
        assert hit and same_hits(np.array([(t, u, v, p)], HIT_DTYPE), h[i:i + 1])


def _pinholes(orc, cam, pixels, W, H, contract):
    import ctypes as C
    out = np.zeros((len(pixels), 6), np.float32)
    for i, (x, y) in enumerate(pixels):
        orc.lib().orc_camera_pinhole(C.byref(cam), int(x), int(y), W, H, contract,
                                     out[i].ctypes.data_as(C.POINTER(C.c_float)))
    return out


@pytest.mark.parametrize("math_mode", [0, 1])
def test_pick_rays_match_the_pinhole_camera(orc, math_mode):
    import raytracertest_amd as R
    contract = oc(orc, math_mode)
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    W, H = 96, 64
    rng = np.random.default_rng(3)

    def pixels(W, H, rows_range=None):
        y0, y1 = rows_range or (0, H)
        p = [(0, y0), (W - 1, y0), (0, y1 - 1), (W - 1, y1 - 1), (W // 2, (y0 + y1) // 2)]
        return np.array(p + list(zip(rng.integers(0, W, 40), rng.integers(y0, y1, 40))), np.uint32)

    def check(g, cam, W, H, pix):
        hits, rays = g.Pick(pix, return_rays=True)
        assert np.array_equal(rays.view(np.uint32), _pinholes(orc, cam, pix, W, H, contract).view(np.uint32))
        assert same_hits(hits, expected_hits(orc, rays, rows, None, contract))
        assert same_hits(g.Pick(pix), hits)

    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode)
    assert g.UploadScene(rows)
    check(g, orc.camera((0.0, 0.0), 70.0, 3.0, 0.05), W, H, pixels(W, H))
    g.RotateCamera((0.13, -0.21))
    g.SetCameraParameters(55.0, 4.0, 0.1)
    cam = orc.camera((0.13, -0.21), 55.0, 4.0, 0.1)
    check(g, cam, W, H, pixels(W, H))
    g.Resize((80, 50))
    check(g, cam, 80, 50, pixels(80, 50))
    with pytest.raises(R.RtError, match="outside"):
        g.Pick([(80, 0)])
    with pytest.raises(R.RtError, match="outside"):
        g.Pick([(0, 0), (0, 50)])
    g.close()
    # a band tracer picks any row of the full image, and a two-band handle answers for the whole frame
    b = R.RayTracer((W, 16), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, full_height=H, row_begin=32)
    assert b.UploadScene(rows)
    check(b, orc.camera((0.0, 0.0), 70.0, 3.0, 0.05), W, H, pixels(W, H, (0, 32)))
    with pytest.raises(R.RtError, match="outside"):
        b.Pick([(0, H)])
    b.close()
    m = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, math_mode=math_mode, devices=[0, 0])
    assert m.UploadScene(rows)
    m.RotateCamera((0.05, 0.1))
    check(m, orc.camera((0.05, 0.1), 70.0, 3.0, 0.05), W, H, pixels(W, H))
    m.close()


def _focus_scene():
    """A quad at z = -5 on the left of the view; one triangle in both windings at z = +4 behind the camera, where the pinhole
    rays of the right half meet it at t < 0; the middle columns see neither."""
    quad = [[-9, -9, -5], [-0.5, -9, -5], [-9, 9, -5], [-0.5, -9, -5], [-0.5, 9, -5], [-9, 9, -5]]
    back = [[-1, -30, 4], [-1, 30, 4], [-40, 0, 4], [-1, -30, 4], [-40, 0, 4], [-1, 30, 4]]
    rows = np.zeros((12, 4), np.float32)
    rows[:, :3] = quad + back
    return rows


@pytest.mark.parametrize("math_mode", [0, 1])
def test_focus_at_sets_the_focal_length_the_oracle_renders_with(orc, math_mode):
    import raytracertest_amd as R
    contract = oc(orc, math_mode)
    from raytracertest_amd import scenes
    W, H = 96, 64
    rows = scenes.cornell32()
    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.2, seed=5, math_mode=math_mode)
    assert g.UploadScene(rows)
    f = g.FocusAt(40, 30)
    assert f == g.Pick([(40, 30)])[0]["t"] and 0 < f < 100 and f != np.float32(10.0)
    g.Trace(2, 2, 0)
    assert g.Wait()
    o = orc.OracleTracer(W, H, (0.0, 0.0), 70.0, float(f), 0.2, seed=5, nthreads=4, contract=contract)
    o.upload_scene(rows)
    o.trace(2, 2)
    assert np.array_equal(g.RenderBuffer().view(np.uint32), o.render.view(np.uint32)) and np.array_equal(g.Image(), o.image)


@pytest.mark.parametrize("math_mode", [0, 1])
def test_focus_at_background_or_behind_is_rejected_and_changes_nothing(orc, math_mode):
    import raytracertest_amd as R
    contract = oc(orc, math_mode)
    W, H = 96, 64
    rows = _focus_scene()
    g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.2, seed=5, math_mode=math_mode)
    assert g.UploadScene(rows)
    left, right, top = g.Pick([(5, 32)])[0], g.Pick([(90, 32)])[0], g.Pick([(48, 0)])[0]
    assert left["prim"] in (0, 1) and left["t"] > 0
    assert right["prim"] in (2, 3) and right["t"] < 0            # only a hit behind the camera (the reference rule keeps it)
    cand = np.array([(x, y) for x in range(W) for y in (0, 32, H - 1)], np.uint32)
    bg = [tuple(int(c) for c in xy) for xy, h in zip(cand, g.Pick(cand)) if h["prim"] < 0]
    assert bg, "no background pixel"
    with pytest.raises(R.RtError, match="background"):
        g.FocusAt(*bg[0])
    with pytest.raises(R.RtError, match="not in front"):
        g.FocusAt(90, 32)
    g.Trace(2, 2, 0)
    assert g.Wait()
    o = orc.OracleTracer(W, H, (0.0, 0.0), 70.0, 3.0, 0.2, seed=5, nthreads=4, contract=contract)
    o.upload_scene(rows)
    o.trace(2, 2)
    assert np.array_equal(g.RenderBuffer().view(np.uint32), o.render.view(np.uint32))
    assert g.FocusAt(5, 32) == left["t"]


def test_picks_do_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    pix = np.array([[1000, 500], [17, 3], [1919, 1079]], np.uint32)

    def run(picks):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.Pick(pix)
        got = []
        g.Trace(24, 4, 2)
        for _ in range(picks):
            got.append(g.Pick(pix))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(20)
    assert len(got) == 20 and all(same_hits(x, idle) for x in got)
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_torch_path_and_upload_ordering(orc):
    torch = pytest.importorskip("torch")
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    a_rows = adversarial_scene(37, seed=37)
    b_rows = scenes.cornell32()
    rays = adversarial_rays(a_rows, 3000, seed=9)
    g = _tracer()
    assert g.UploadScene(a_rows)
    want_a = g.Intersect(rays)
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        rt = torch.from_numpy(rays).to("cuda:0", non_blocking=False)
        h = g.Intersect(rt)
        assert h.shape == (rays.shape[0], 4) and h.dtype == torch.float32
    s.synchronize()
    hn = h.cpu().numpy()
    assert np.array_equal(hn.view(np.uint32), want_a.view(np.uint32).reshape(-1, 4))
    assert np.array_equal(h[:, 3].view(torch.int32).cpu().numpy(), want_a["prim"])
    # a query enqueued behind other work on its stream still reads the scene it was enqueued against
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(50_000_000)
        else:
            x = torch.randn(4096, 4096, device="cuda:0")
            for _ in range(20):
                x = x @ x
        h_old = g.Intersect(rt)
    assert g.UploadScene(b_rows)
    with torch.cuda.stream(s):
        h_new = g.Intersect(rt)
    s.synchronize()
    assert np.array_equal(h_old.cpu().numpy().view(np.uint32), want_a.view(np.uint32).reshape(-1, 4))
    want_b = expected_hits(orc, rays[:500], b_rows)
    assert np.array_equal(h_new[:500].cpu().numpy().view(np.uint32), want_b.view(np.uint32).reshape(-1, 4))
    with pytest.raises(ValueError):
        g.Intersect(torch.from_numpy(rays))                       # a host tensor
    with pytest.raises(ValueError):
        g.Intersect(rt.double())


def _build(src, exe):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src,
                    "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-pthread", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("mode", ["fma", "strict"])
def test_cpp_driver_agrees_with_python(tmp_path, mode):
    import raytracertest_amd as R
    exe = _build(os.path.join(ROOT, "tests", "cpp", "query_driver.cpp"), str(tmp_path / "qd"))
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    g = R.RayTracer((64, 48), (0, 0, 0), (0.1, -0.05), 60.0, 10.0, 0.5, seed=3, math_mode=1 if mode == "strict" else 0)
    rows = np.array([[-2, -2, -6, 0], [2, -2, -6, 0], [-2, 2, -6, 0], [2, -2, -6, 0], [2, 2, -6, 0], [-2, 2, -6, 0],
                     [-0.5, -0.5, -3, 0], [0.5, -0.5, -3, 0], [0, 0.5, -3, 0]], np.float32)
    assert g.UploadScene(rows)
    fx = float.fromhex
    picks = re.findall(r"^PICK (\d+) (\d+) (-?\d+) (\S+) (\S+) (\S+)$", out.stdout, re.M)
    rays = re.findall(r"^RAY (\d+) (\d+) (.*)$", out.stdout, re.M)
    assert len(picks) == 6 and len(rays) == 6
    for (x, y, p, t, u, v), (_, _, r) in zip(picks, rays):
        h, ray = g.Pick([(int(x), int(y))], return_rays=True)
        assert int(h[0]["prim"]) == int(p) and (h[0]["t"], h[0]["u"], h[0]["v"]) == (np.float32(fx(t)), np.float32(fx(u)), np.float32(fx(v)))
        assert np.array_equal(ray[0], np.array([fx(c) for c in r.split()], np.float32))
    foc = re.findall(r"^FOCUS (\d+) (\d+) (\d) (\S+)$", out.stdout, re.M)
    assert len(foc) == 2 and foc[0][2] == "1" and np.float32(fx(foc[0][3])) == g.Pick([(32, 24)])[0]["t"]
    assert (foc[1][2] == "1") == bool(g.Pick([(0, 0)])[0]["prim"] >= 0 and g.Pick([(0, 0)])[0]["t"] > 0)
    hits = re.findall(r"^HIT (-?\d+) (\S+) (\S+) (\S+)$", out.stdout, re.M)
    want = g.Intersect(np.array([[0, 0, 0, 0, 0, -1], [1.5, 1.5, 0, 0, 0, -1]], np.float32))
    assert [int(h[0]) for h in hits] == list(want["prim"])
    assert [np.float32(fx(h[1])) for h in hits] == list(want["t"])


def test_cli_focus_renders_what_the_library_renders_with_that_focal_length(tmp_path):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    from raytracertest_amd.bitmap import read_bmp
    scene = str(tmp_path / "c.f4")
    scenes.cornell32().astype("<f4").tofile(scene)
    exe = os.path.join(LIBDIR, "rt_cli")
    bmp = str(tmp_path / "f.bmp")
    out = subprocess.run([exe, "-w", "64", "-h", "40", "-s", "2", "-i", "2", "-u", "0", "--aperture", "0.2", "--scene", scene,
                          "--seed", "4", "--pick", "30,20", "--focus", "30,20", "-o", bmp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"^focus 30 20 focal (\S+)$", out.stdout, re.M)
    p = re.search(r"^pick 30 20 (-?\d+) (\S+) (\S+) (\S+)$", out.stdout, re.M)
    assert m and p
    f = np.float32(float(m.group(1)))
    assert f == np.float32(float(p.group(2))) and int(p.group(1)) >= 0
    g = R.RayTracer((64, 40), (0, 0, 0), (0.0, 0.0), 70.0, float(f), 0.2, seed=4)
    assert g.UploadScene(scenes.cornell32())
    g.Trace(2, 2, 0)
    assert g.Wait()
    assert np.array_equal(read_bmp(bmp), g.Image())
    bad = subprocess.run([exe, "-w", "64", "-h", "40", "--scene", scene, "--focus", "64,0", "-o", str(tmp_path / "x.bmp")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--focus" in bad.stderr
