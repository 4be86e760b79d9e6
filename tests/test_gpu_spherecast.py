"""The swept query on the device (RayTracer.SphereCast / SphereCastContacts / Clearance): the scan and the BVH walk against the
numpy restatement of spherecast_expect, every byte, for both upload layouts, both arithmetic modes (which must not change a
byte), with and without spheres and batches that end in partial waves and blocks; the BVH walk against the scan kernel byte for
byte on 65 536 sweeps, on the lattice and the deep ladder, past its stack and on a refitted tree; identities against ClosestPoint
on the device; empty scenes, spheres alone, n = 0, a running Trace left alone, multi-device forwarding, the torch path and
argument errors."""
import functools
import hashlib

import numpy as np
import pytest

import lattice_cases as lc
import spherecast_expect as se
from query_expect import HIT_DTYPE, edge_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
SPHERES = se.three_spheres()
COUNTS = (1, 63, 64, 65)                                                 # partial waves; 4097 is a partial last block as well


def _tracer(math_mode=0, size=(64, 48), **kw):
    import raytracertest_amd as R
    return R.RayTracer(size, (0, 0, 0), (0.0, 0.0), 70.0, 10.0, 0.5, seed=1, math_mode=math_mode, **kw)


def _assert_hits(got, exp, label):
    assert got.dtype == HIT_DTYPE and got.shape == exp.shape, label
    bad = se.differing(got, exp)
    assert bad.size == 0, (label, bad.size, bad[:5], got[bad[:3]], exp[bad[:3]])


@functools.lru_cache(maxsize=None)
def _reference(n_tris):
    """The scene (slivers; from 5 triangles up a segment, a point and a NaN record), 4097 sweeps of every population in one
    permuted batch, and the restatement's table with SPHERES' columns: one table for all."""
    rows = se.scene(n_tris, seed=100 + n_tris)
    sweeps = se.batch(rows, 4097, 300 + n_tris, spheres=SPHERES)
    tab = se.table(sweeps, rows, spheres=SPHERES)
    for x in (rows, sweeps) + tab:
        x.setflags(write=False)
    return rows, sweeps, tab


def _expected(n_tris, spheres):
    rows, sweeps, tab = _reference(n_tris)
    if not spheres:
        tab = tuple(x[:, :n_tris] for x in tab)
    return se.winners(tab, sweeps)


def test_the_populations_reach_what_they_are_for():
    rows, sweeps, _ = _reference(1100)
    hits, feature = _expected(1100, True)
    tri = (hits["prim"] >= 0) & (hits["prim"] < 1100)
    for f in range(1, 8):
        assert (tri & (feature == f)).any(), se.FEATURES[f]
    valid = se.valid(sweeps)
    assert (tri & (hits["t"] == 0)).any() and (valid & (hits["prim"] < 0)).any() and (hits["prim"] == 1100).any() and (hits["prim"] == 1102).any()
    assert ((hits["prim"] >= 0) & (hits["t"] == sweeps[:, 7])).any() and (hits["prim"] > 1024).any() and (~valid).sum() >= 5
    for slot in range(8):
        assert np.isnan(sweeps[:, slot]).any() and np.isinf(sweeps[:, slot]).any(), slot
    assert (sweeps[:, 6] == 0).any() and (sweeps[:, 6] == 100).any() and (sweeps[:, 3:6] == 0).all(axis=1).any()


@pytest.mark.parametrize("n_tris", [1, 5, 37, 1100])
@pytest.mark.parametrize("spheres", [False, True])
def test_scan_and_bvh_against_the_restatement_every_byte(n_tris, spheres):
    rows, sweeps, _ = _reference(n_tris)
    exp, _ = _expected(n_tris, spheres)
    digests = {}
    for edges in (False, True):
        for mm in (0, 1):
            g = _tracer(mm)
            assert (g.UploadSceneEdges(edge_rows(rows)) if edges else g.UploadScene(rows))
            if spheres:
                g.UploadSpheres(SPHERES)
            blob = hashlib.sha256()
            for accel in (False, True):
                g.SetQueryAcceleration(accel)
                label = "n_tris=%d spheres=%d edges=%d mm=%d accel=%d" % (n_tris, spheres, edges, mm, accel)
                got = g.SphereCast(sweeps)
                _assert_hits(got, exp, label)                            # no case is excluded
                blob.update(got.tobytes())
                for n in COUNTS:
                    _assert_hits(g.SphereCast(sweeps[:n]), exp[:n], label + " n=%d" % n)
                if accel and n_tris >= 5:
                    info = g.QueryAccelInfo()
                    assert info["mode"] == 1 and info["valid"] == 1 and info["always_tested"] == 1
            digests[(edges, mm)] = blob.hexdigest()
            g.close()
    assert len(set(digests.values())) == 1                               # neither the layout nor the arithmetic mode changes a byte


def _mixed(rows, n, seed, rel=False):
    a = se.random_sweeps(rows, n - n // 4, seed, rel=rel)
    b = se.random_sweeps(rows, n // 4, seed + 1, rmin=-1.0, rmax=0.5, rel=rel)
    b[::3, 7] = f32(0.5)                                                 # a third of the wide ones cut at tmax
    return np.concatenate([a, b])


@pytest.mark.parametrize("scene", ["random10000", "rooms", "copies"])
def test_bvh_equals_scan_byte_for_byte(scene):
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345) if scene == "random10000" else lc.rooms() if scene == "rooms" else lc.copies()[0]
    sweeps = _mixed(rows, 65536, 5)
    if scene == "rooms":                                                 # along the lattice's axes and inside its walls' planes
        ax = lc.axis_rays()
        pl = lc.in_plane_rays()
        for k, rays in enumerate((ax, pl)):
            m = min(len(rays), 2000)
            sweeps[k * 2000:k * 2000 + m, :6] = rays[:m, :6]
    g = _tracer()
    assert g.UploadScene(rows)
    scan = g.SphereCast(sweeps)
    assert (scan["prim"] >= 0).sum() > 20000 and (scan["prim"] < 0).sum() > 200 and (scan["t"][scan["prim"] >= 0] == 0).any()
    g.SetQueryAcceleration(True)
    _assert_hits(g.SphereCast(sweeps), scan, scene)
    g.DebugQueryAccelSlack(1000000)                                      # a wider allowance changes nothing
    _assert_hits(g.SphereCast(sweeps[:8192]), scan[:8192], scene + " wide")
    g.DebugQueryAccelSlack(1000)
    g.close()


def test_the_deep_ladder_past_its_stack_and_through_the_restatement():
    import deep_cases as dc
    rows = dc.deep_scene(mirror=True)
    sweeps = _mixed(rows, 4096, 9, rel=True)
    exp = se.expected(sweeps, rows)
    assert (exp["prim"] >= 0).sum() > 1000 and (exp["prim"] < 0).sum() > 100
    g = _tracer()
    assert g.UploadScene(rows)
    _assert_hits(g.SphereCast(sweeps), exp, "deep scan")
    g.SetQueryAcceleration(True)
    try:
        for cap in (None, 0, 1, 3):
            g.DebugQueryStackCap(cap)
            _assert_hits(g.SphereCast(sweeps), exp, "deep cap=%r" % (cap,))
    finally:
        g.DebugQueryStackCap(None)
    g.close()


def test_a_refitted_tree_answers_as_the_scan():
    import raytracertest_amd as R
    import refit_cases as rc
    rows = rc.scenes()["adversarial1100"]
    moved = rc.jitter(rows, 5)
    sweeps = _mixed(moved, 8192, 9)
    g = _tracer()
    g.SetQueryAccelUpdate(R.api.ACCEL_REFIT)
    g.SetQueryAcceleration(True)
    assert g.UploadScene(rows)
    first = g.SphereCast(sweeps)
    assert g.QueryAccelUpdateInfo()["refits"] == 0 and g.QueryAccelInfo()["valid"] == 1
    assert g.UploadScene(moved)
    got = g.SphereCast(sweeps)                                           # refits
    u1 = g.QueryAccelUpdateInfo()
    assert u1["refits"] == 1 and u1["fallbacks"] == 0
    g.SetQueryAcceleration(False)
    _assert_hits(got, g.SphereCast(sweeps), "after the refit")
    assert se.differing(first, got).size > 0                             # the scene did move
    _assert_hits(got[:512], se.expected(sweeps[:512], moved), "the moved scene against the restatement")
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_identities_against_closest_point_on_the_device():
    """Exact by construction and independent of the numpy restatement: a start overlap is ClosestPoint within r; a reported
    contact's centre has something within r + s; Clearance is SphereCast without a contact."""
    rows, sweeps, _ = _reference(1100)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        hits = g.SphereCast(sweeps)
        valid = se.valid(sweeps)
        r = sweeps[:, 6]
        near = g.ClosestPoint(np.c_[sweeps[:, :3], r * r])
        started = (hits["prim"] >= 0) & (hits["t"] == 0)
        assert np.array_equal(started[valid], (near["prim"] >= 0)[valid]) and started.sum() > 50 and not started[~valid].any()
        hit = hits["prim"] >= 0
        c, s = se.centres(sweeps, hits["t"])
        c = np.where(started[:, None], sweeps[:, :3], c)                 # (step 1 evaluates at o itself)
        rs = r + s
        found = g.ClosestPoint(np.c_[c, rs * rs])
        assert (found["prim"][hit] >= 0).all() and hit.sum() > 2000
        # the winner's own record certifies it: its (u, v) are ClosestPoint's at c wherever it is also the nearest
        same = hit & (found["prim"] == hits["prim"]) & ~started
        assert same.sum() > 1000 and np.array_equal(found["u"][same], hits["u"][same]) and np.array_equal(found["v"][same], hits["v"][same])
    fin = valid & np.isfinite(sweeps).all(axis=1)
    a, d = sweeps[fin, :3], sweeps[fin, 3:6]
    b = a + d
    clear = g.Clearance(a, b, sweeps[fin, 6])
    again = np.empty((fin.sum(), 8), f32)
    again[:, :3], again[:, 3:6], again[:, 6], again[:, 7] = a, b - a, sweeps[fin, 6], 1.0
    assert clear.dtype == np.bool_ and np.array_equal(clear, g.SphereCast(again)["prim"] < 0) and clear.any() and (~clear).any()
    # contacts: the centre is o + t*d, the position lies within r + s of it, the normal is a unit vector from the surface to the centre
    h = g.SphereCast(sweeps[fin])
    centre, position, normal = g.SphereCastContacts(sweeps[fin], h)
    moving = (h["prim"] >= 0) & (h["t"] > 0) & (sweeps[fin, 6] > 0.01)
    assert np.isnan(centre[h["prim"] < 0]).all() and np.array_equal(centre[moving], se.centres(sweeps[fin], h["t"])[0][moving])
    gap = np.linalg.norm((centre - position)[moving].astype(np.float64), axis=1)
    _, s = se.centres(sweeps[fin], h["t"])
    assert (gap <= sweeps[fin, 6][moving] + 2 * s[moving]).all()     # (certified: the nearest point of the record is within r + s)
    assert np.allclose(np.linalg.norm(normal[moving].astype(np.float64), axis=1), 1.0, atol=1e-5)
    g.close()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_empty_scenes_spheres_alone_and_no_sweeps():
    _, sweeps, _ = _reference(37)
    for accel in (False, True):
        g = _tracer()
        g.SetQueryAcceleration(accel)
        hits = g.SphereCast(sweeps)                                      # no scene: nothing to touch
        assert (hits["prim"] == -1).all() and not hits["t"].any() and not hits["u"].any() and not hits["v"].any()
        assert g.SphereCast(np.zeros((0, 8), f32)).shape == (0,)
        assert g.Clearance(np.zeros((3, 3)), np.ones((3, 3)), 0.5).all()
        g.UploadSpheres(SPHERES)                                         # spheres alone can answer
        exp = se.expected(sweeps, None, spheres=SPHERES)
        assert (exp["prim"] == 0).any() and (exp["prim"] == 2).any() and not (exp["prim"] == 1).any()
        _assert_hits(g.SphereCast(sweeps), exp, "spheres only accel=%d" % accel)
        g.close()


def test_torch_path_argument_errors_and_misaligned_pointers():
    import torch
    import raytracertest_amd as R
    rows, sweeps, _ = _reference(1100)
    exp, _ = _expected(1100, True)
    g = _tracer()
    assert g.UploadScene(rows)
    g.UploadSpheres(SPHERES)
    L = R.api.load_library()
    t = torch.from_numpy(np.array(sweeps)).to("cuda:0")
    for accel in (False, True):
        g.SetQueryAcceleration(accel)
        th = g.SphereCast(t)
        assert th.dtype == torch.float32 and th.shape == (4097, 4) and th.cpu().numpy().tobytes() == exp.tobytes()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                       # on the caller's current stream, no host synchronisation
            th2 = g.SphereCast(t)
        s.synchronize()
        assert torch.equal(th2.view(torch.int32), th.view(torch.int32))
        assert g.SphereCast(t[:0]).shape == (0, 4)
    for bad in (t.cpu(), t.double(), t[:, :6].contiguous(), t.t(), t.reshape(-1)):
        with pytest.raises(ValueError):
            g.SphereCast(bad)
    for bad in (np.zeros((4, 6), f32), f32(1.0)):
        with pytest.raises(ValueError):
            g.SphereCast(bad)
    flat = t.reshape(-1)
    out = torch.full((8, 4), 77.0, dtype=torch.float32, device="cuda:0")
    P, O = flat.data_ptr(), out.data_ptr()
    for args in ((P + 4, 8, O), (P, 8, O + 4), (P + 8, 8, O)):           # misaligned sweeps, hits
        assert L.rt_tracer_sphere_cast_device(g._h, *args, None) == 1 and "16-byte" in g.LastError()
    for args in ((None, 8, O), (P, 8, None)):
        assert L.rt_tracer_sphere_cast_device(g._h, *args, None) == 1 and "null" in g.LastError()
    host = np.full(8, 77, np.float32)
    assert L.rt_tracer_sphere_cast(g._h, None, 2, host.ctypes.data) == 1 and L.rt_tracer_sphere_cast(g._h, host.ctypes.data, 1, None) == 1
    torch.cuda.synchronize()
    assert (out == 77).all() and (host == 77).all()                      # the outputs are untouched
    assert L.rt_tracer_sphere_cast_device(g._h, None, 0, None, None) == 0 and L.rt_tracer_sphere_cast(g._h, None, 0, None) == 0
    assert L.rt_tracer_sphere_cast_device(g._h, P, 8, O, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == exp[:8].tobytes()
    g.close()


def test_sphere_cast_does_not_disturb_a_running_trace():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.random_triangles(10000, 12345)
    sweeps = _mixed(rows, 4096, 7)

    def run(calls):
        g = R.RayTracer((1920, 1080), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=11)
        assert g.UploadScene(rows)
        idle = g.SphereCast(sweeps)
        got = []
        g.Trace(24, 4, 2)
        for i in range(calls):
            g.SetQueryAcceleration(i % 2 == 1)                           # both modes; the tree is built while the Trace runs
            got.append(g.SphereCast(sweeps))
        assert g.Wait() == 1
        out = (g.RenderBuffer(), g.SampleCounts(), g.RngStates(), g.Image())
        g.close()
        return idle, got, out

    idle, got, out = run(6)
    assert len(got) == 6 and (idle["prim"] >= 0).any()
    for h in got:
        _assert_hits(h, idle, "beside a running Trace")
    _, _, ref = run(0)
    for a, b in zip(out, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_multi_device_handle_answers_as_its_first_band():
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    rows = scenes.cornell32()
    sweeps = _mixed(rows, 2000, 3)
    exp = se.expected(sweeps, rows)
    assert (exp["prim"] >= 0).sum() > 500
    one = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
    assert one.UploadScene(rows)
    _assert_hits(one.SphereCast(sweeps), exp, "one band against the restatement")
    one.close()
    m = R.RayTracer((96, 64), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, devices=[0, 0])
    assert m.UploadScene(rows)
    _assert_hits(m.SphereCast(sweeps), exp, "two bands, scan")
    m.SetQueryAcceleration(True)
    _assert_hits(m.SphereCast(sweeps), exp, "two bands, bvh")
    assert m.QueryAccelInfo()["valid"] == 1
    m.close()
