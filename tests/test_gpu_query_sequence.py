"""Every query in a row on ONE tracer: what the entry points share -- the four staging buffers (QueryState::in[2] and
::out[2], typed at each call: out[0] holds hits, rows of hits, bytes, masks, prims or sides in turn; all grow-only), the one event
behind every launch and the one forward of a sharded handle -- must leave each answer as a fresh tracer that made only that
call gives it, byte for byte: in the scan and the BVH mode, for a smaller batch after a larger one, through the torch tensor
paths on the current stream, and on two bands.  The other suites pin the fresh answers to the oracle and the helpers."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SMALL, K = 70, 5, 3                                                   # one wave and six lanes; a smaller batch behind it
SIZE = (96, 64)
SPHERE = np.array([[0.1, -0.5, -1.6, 0.3]], np.float32)
STEPS = ("Intersect", "ClosestPoint", "SignedDistance", "Occluded", "IntersectAll", "ClosestAll", "ClosestAll after", "ClosestSides",
         "Pick", "Intersect again")
BATCHES = [(accel, n) for accel in (False, True) for n in (N, SMALL)]    # the order one tracer runs them in


def _tracer(**kw):
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    g = R.RayTracer(SIZE, (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, **kw)
    assert g.UploadScene(scenes.cornell32())
    g.UploadSpheres(SPHERE)
    return g


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(70)
    rays = np.zeros((N, 6), np.float32)
    rays[:, :3] = rng.uniform(-0.05, 0.05, (N, 3))
    rays[:, 3:5], rays[:, 5] = rng.uniform(-0.6, 0.6, (N, 2)), -1.0
    segs = np.zeros((N, 8), np.float32)
    segs[:, :6], segs[:, 6], segs[:, 7] = rays, 1e-3, rng.uniform(0.5, 4.0, N)    # some end in front of the room
    pts = rng.uniform((-1.2, -1.2, -3.2), (1.2, 1.2, -0.8), (N, 3)).astype(np.float32)   # three columns: the radius is filled in
    pix = np.stack([(np.arange(N) * 37) % SIZE[0], (np.arange(N) * 11) % SIZE[1]], 1).astype(np.uint32)
    d = {"rays": rays, "segs": segs, "pts": pts, "pix": pix}
    for a in d.values():
        a.setflags(write=False)
    return d


def _call(g, step, d, n, rows, dev=None):
    """Step `step` of the sequence on the first n items -> what the method returned.  rows: ClosestAll's answer of step 5, which
    steps 6 and 7 take their cursor and records from.  dev: the tensor paths (Pick has none)."""
    def arg(name):
        a = d[name][:n]
        if dev is None:
            return a
        import torch
        return torch.from_numpy(np.array(a)).to(dev)
    if step in (0, 9):
        return g.Intersect(arg("rays"))
    if step == 1:
        return g.ClosestPoint(arg("pts"))
    if step == 2:
        return g.SignedDistance(arg("pts"))
    if step == 3:
        return g.Occluded(arg("segs"))
    if step == 4:
        return g.IntersectAll(arg("segs"), K)
    if step == 5:
        return g.ClosestAll(arg("pts"), K)
    if step == 6:
        last = rows[0][:, K - 1]
        return g.ClosestAll(arg("pts"), K, after=np.ascontiguousarray(last) if dev is None else last.contiguous())
    if step == 7:
        return g.ClosestSides(arg("pts"), rows[0])
    return g.Pick(d["pix"][:n], return_rays=True)


def _sequence(g, d, n, dev=None):
    out, rows = [], None
    for step in range(len(STEPS)):
        out.append(_call(g, step, d, n, rows, dev))
        if step == 5:
            rows = out[-1]
    return out


def _blob(answer):
    parts = answer if isinstance(answer, tuple) else (answer,)
    return b"".join((p if isinstance(p, np.ndarray) else p.cpu().numpy()).tobytes() for p in parts)


@functools.lru_cache(maxsize=None)
def _fresh():
    """{(accel, n): the bytes of each step on a tracer of its own that made only that call}."""
    d, out = _inputs(), {}
    for accel, n in BATCHES:
        answers, rows = [], None
        for step in range(len(STEPS)):
            g = _tracer()
            g.SetQueryAcceleration(accel)
            answers.append(_call(g, step, d, n, rows))
            g.close()
            if step == 5:
                rows = answers[-1]
        hits, (all_hits, counts), occ = answers[0], answers[5], answers[3]
        assert (hits["prim"] >= 0).any() and (counts == K).all() and all_hits.shape == (n, K)
        assert answers[6][0].tobytes() != all_hits.tobytes() and (n < N or (occ.any() and not occ.all()))
        out[(accel, n)] = [_blob(a) for a in answers]
    return out


def _assert_sequences(g, dev=None):
    d, got = _inputs(), {}
    for accel, n in BATCHES:
        g.SetQueryAcceleration(accel)
        got[(accel, n)] = _sequence(g, d, n, dev)
    if dev is not None:
        import torch
        torch.cuda.synchronize()                                          # the only one the test makes
    for key, answers in got.items():
        for step, (a, exp) in enumerate(zip(answers, _fresh()[key])):
            assert _blob(a) == exp, (key, STEPS[step])


def test_one_tracer_answers_the_sequence_as_fresh_tracers_answer_each_call():
    g = _tracer()
    _assert_sequences(g)
    g.close()


def test_the_tensor_paths_on_the_current_stream_give_the_same_bytes():
    g = _tracer()
    _assert_sequences(g, dev="cuda:0")
    g.close()


def test_two_bands_answer_the_sequence_as_one_tracer_and_report_a_bad_pick():
    from raytracertest_amd import api
    m = _tracer(devices=[0, 0])
    _assert_sequences(m)
    with pytest.raises(api.RtError):
        m.Pick([[SIZE[0], 0]])                                           # one column to the right of the image
    assert "outside" in m.LastError()
    m.SetQueryAcceleration(False)
    assert _blob(m.Pick(_inputs()["pix"], return_rays=True)) == _fresh()[(False, N)][8]
    m.close()
