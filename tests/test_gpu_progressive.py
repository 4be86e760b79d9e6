"""The images a progressive Trace hands to its update and finished callbacks (tests/progressive_cases.py): every update image,
in order and bit for bit, is the oracle's conversion at that update point; the finished image is the oracle's last one; the
four buffers behind them are the oracle's; the Trace ran as the launches schedule() predicts; and a second Trace on the same
tracer -- the other parity of the two host images, the continued RNG stream -- holds the same.  Then a reader that is slow, a
Stop() from inside an update, and the same through the multi-device handle (rt_multi_api.hpp), whose loop is a second
implementation.

The two multi-device cases (progressive_cases.MULTI) take classic's and every's Trace arguments only: both use every's lens,
aperture 0.3, because classic's 0.05 leaves images of the 64 x 50 frame closer than MIN_DIFFERING."""
import time

import numpy as np
import pytest

import progressive_cases as pc

pytestmark = pytest.mark.gpu
_EXP = {}


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    from raytracertest_amd import api
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return api


def tracer(rt, case, mode=0, nearest=False, **kw):
    g = rt.RayTracer(case["frame"], (0, 0, 0), pc.CAMERA["angles"], pc.CAMERA["fov"], case["focal"], case["aperture"],
                     seed=case["seed"], math_mode=mode, nearest_hit=nearest, **dict(case["options"], **kw))
    assert g.UploadScene(pc.scene_rows(case))
    if case["spheres"]:
        g.UploadSpheres(pc.SPHERE)
    return g


def expected_traces(orc, case, mode=0, nearest=False):
    """expected() of a first Trace of the case, of a second one behind it and (`groups`) of a third, computed once and shared
    (never written to)"""
    key = (case["name"], mode, nearest)
    if key not in _EXP:
        out = [pc.expected(orc, case, mode=mode, nearest=nearest)]
        for _ in range(2 if case["name"] == "groups" else 1):
            out.append(pc.expected(orc, case, o=out[-1]["o"]))
        _EXP[key] = tuple(out)
    return _EXP[key]


class Recorder:
    """both callbacks of a tracer: every call appended as (kind, image copy, size), in the order of the calls"""

    def __init__(self, g, sleep=0.0, stop_at=None):
        self.g, self.events, self.sleep, self.stop_at = g, [], sleep, stop_at
        g.SetUpdateCallback(self.update)
        g.SetFinishedCallback(lambda img, size: self.events.append(("finished", img.copy(), size)))

    def update(self, img, size):
        if self.sleep:
            time.sleep(self.sleep)                                       # the launch enqueued behind this callback finishes meanwhile
        self.events.append(("update", img.copy(), size))
        if self.stop_at is not None and len(self.events) == self.stop_at:
            self.g.Stop()

    def take(self):
        out, self.events = self.events, []
        return out


def same(what, name, got, want):
    d = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    assert got.shape == want.shape and d.size == 0, "%s: %s differs in %d words, first at (row, x, ...) %s" % (what, name, d.shape[0], d[0].tolist())


def check_images(what, events, exp, frame, finished=True):
    """the callbacks' images are expected()'s: the updates in order, then -- after all of them -- the finished one"""
    W, H = frame
    kinds = [k for k, _, _ in events]
    assert kinds == ["update"] * len(exp["updates"]) + ["finished"] * int(finished), (what, kinds, [i for i, _ in exp["updates"]])
    assert all(size == W * H * 4 and img.shape == (H, W) for _, img, size in events), what
    for (kind, img, _), (i, want) in zip(events, exp["updates"]):
        same(what, "update image of iteration %d" % i, img, want)
    if finished:
        same(what, "finished image", events[-1][1], exp["final"])


def check_buffers(what, g, exp, image=True):
    same(what, "render", g.RenderBuffer(), exp["render"])
    same(what, "counts", g.SampleCounts(), exp["counts"])
    same(what, "rng", g.RngStates(), exp["rng"])
    if image:
        same(what, "image", g.Image(), exp["final"])


def trace_and_check(what, g, rec, exp, args, frame, steps=True, settles=False):
    """one Trace(*args) that runs to its end: callbacks, buffers, and the launches it took"""
    n, spp, interval = args
    if steps:
        g.DebugEnqueueCalls()                                            # (reading clears the counters)
    g.Trace(n, spp, interval)
    assert g.Wait(), g.LastError()
    if settles:                                                          # before any read-back pays the debt
        assert g.DebugOwedState()["settles_enqueued"] >= 1, what
    if steps:
        took = g.DebugEnqueueCalls()["steps"]
        launches = pc.schedule(n, spp, interval, True, g.FusedIterations(spp))[1]
        assert took == len(launches), (what, took, launches)
    events = rec.take()
    check_images(what, events, exp, frame)
    same(what, "Image() against the finished image", g.Image(), events[-1][1])
    if n > 1 and interval > 0 and (n - 1) % interval == 0:               # the same image in both callbacks, update first
        same(what, "last update against the finished image", events[-2][1], events[-1][1])
    check_buffers(what, g, exp)
    assert g.LastError() == "", what


VARIANTS = [(c, mode, nearest) for c in pc.CASES for mode, nearest in c["variants"]]


@pytest.mark.parametrize("case,mode,nearest", VARIANTS, ids=["%s-m%d%s" % (c["name"], m, "-nearest" if nh else "") for c, m, nh in VARIANTS])
def test_update_and_finished_images_are_the_oracles(rt, orc, case, mode, nearest):
    first, second = expected_traces(orc, case, mode, nearest)[:2]
    args = (case["n"], case["spp"], case["interval"])
    g = tracer(rt, case, mode, nearest)
    rec = Recorder(g)
    what = "%s mode %d nearest %d" % (case["name"], mode, nearest)
    if case["name"] == "scan" or case["name"] == "nofuse":
        assert g.FusedIterations(case["spp"]) == 1
    if case["name"] == "groups":
        assert g.FusedIterations(case["spp"]) == 64
    trace_and_check(what, g, rec, first, args, case["frame"], settles=case["name"] == "settle")   # (a periodic settle inside the Trace)
    trace_and_check(what + ", second Trace", g, rec, second, args, case["frame"])
    if case["name"] == "groups":                                       # the same pass as split launches, on the lists the unsplit ones kept
        third = expected_traces(orc, case, mode, nearest)[2]
        g.TraceEnqueue(case["n"], case["spp"]); g.Sync()
        check_buffers(what + ", TraceEnqueue behind the Traces", g, third)
        assert rec.take() == []
    g.close()


@pytest.mark.parametrize("name", ["every", "classic"])
def test_slow_reader_still_sees_its_own_image(rt, orc, name):
    """A callback that only copies its image 50 ms after it was called -- long against a launch of these frames (tens of
    microseconds), so the launch enqueued behind the callback has finished writing its own host image -- still copies the
    expected one.  (A shorter sleep weakens the test; it never fails it.)"""
    case = pc.BY_NAME[name]
    first, second = expected_traces(orc, case)
    g = tracer(rt, case)
    rec = Recorder(g, sleep=0.05)
    for what, exp in (("first", first), ("second", second)):
        g.Trace(case["n"], case["spp"], case["interval"])
        assert g.Wait(), g.LastError()
        check_images("%s, slow reader, %s Trace" % (name, what), rec.take(), exp, case["frame"])
    check_buffers(name + ", slow reader", g, second)
    g.close()


def stop_inside_update(rt, orc, case, **kw):
    """Trace(400, ...) of the case, Stop() from inside the 2nd update: no finished callback; the tracer holds exactly m
    iterations, m >= 3; every update point below m was delivered with its image (an update whose iteration ran is always
    delivered); and the next Trace, with classic's arguments, is a complete one."""
    n, k = 400, 2
    spp, interval, frame = case["spp"], case["interval"], case["frame"]
    g = tracer(rt, case, **kw)
    rec = Recorder(g, stop_at=k)
    g.Trace(n, spp, interval)
    assert g.Wait() is False and g.LastError() == ""
    events = rec.take()
    counts = g.SampleCounts()
    m = int(counts[0, 0]) // spp
    assert (counts == spp * m).all() and k * interval + 1 <= m <= n, (m, np.unique(counts))
    exp = pc.expected(orc, case, n=m)
    assert [i for i, _ in exp["updates"]] == [i for i in pc.schedule(n, spp, interval, True, 1)[0] if i < m]
    check_images("stopped after %d iterations" % m, events, exp, frame, finished=False)
    check_buffers("stopped after %d iterations" % m, g, exp, image=False)
    rec.stop_at = None
    args = tuple(pc.BY_NAME["classic"][key] for key in ("n", "spp", "interval"))
    fresh = pc.expected(orc, case, o=exp["o"], n=args[0], spp=args[1], interval=args[2])
    trace_and_check("the Trace behind the stopped one", g, rec, fresh, args, frame, steps=not kw)
    g.close()


def test_stop_from_inside_an_update(rt, orc):
    stop_inside_update(rt, orc, pc.BY_NAME["every"])


# ------------------------------------------------------------------------------------------------------------ the multi-device handle
@pytest.mark.parametrize("case", pc.MULTI, ids=[c["name"] for c in pc.MULTI])
def test_multi_device_updates_are_whole_frames_of_one_iteration(rt, orc, case):
    """rt_tracer_create_multi, three bands on one device: each update is the whole gathered frame of one update point"""
    first, second = expected_traces(orc, case)
    g = tracer(rt, case, devices=[0, 0, 0])
    assert [b["rows"] for b in g.Bands()] == [16, 17, 17]
    rec = Recorder(g)
    args = (case["n"], case["spp"], case["interval"])
    for what, exp in (("first", first), ("second", second)):
        what = "%s, %s Trace" % (case["name"], what)
        trace_and_check(what, g, rec, exp, args, case["frame"], steps=False)
        same(what, "Frame()", g.Frame(), exp["final"])
    g.close()


def test_multi_device_updates_through_the_one_rank_rccl_gather(rt, orc, monkeypatch):
    """RT_MI355X_GATHER_SELF=1: the tiles travel through the send double-buffer and a one-rank communicator on every update"""
    case = pc.MULTI[1]
    first, _ = expected_traces(orc, case)
    monkeypatch.setenv("RT_MI355X_GATHER_SELF", "1")
    g = tracer(rt, case, devices=[0, 0, 0])
    monkeypatch.delenv("RT_MI355X_GATHER_SELF")
    assert g.GroupInfo()["transport"] == "rccl"
    rec = Recorder(g)
    trace_and_check(case["name"] + ", RCCL to self", g, rec, first, (case["n"], case["spp"], case["interval"]), case["frame"], steps=False)
    same(case["name"] + ", RCCL to self", "Frame()", g.Frame(), first["final"])
    g.close()


def test_multi_device_stop_from_inside_an_update(rt, orc):
    stop_inside_update(rt, orc, pc.MULTI[1], devices=[0, 0, 0])
