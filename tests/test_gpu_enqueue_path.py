"""The host's enqueue path of the small-scene trace launches (rt_tracer.hpp: enqueue_trace_launch, TileListRing,
build_tile_lists_ahead; rt_kernels.hip: launch_trace, launch_tile_lists).  The list ring's events are stop events of kernel
launches instead of records of their own -- list_ready on the builder, the list_free pair on the last trace kernel each stream
gets before every fourth build -- and the kernels are launched through cached descriptors.  What could go wrong is ordering: a
build that overwrites a slot under a reader, or a trace kernel that starts before its lists are built, reads the wrong
build's lists and traces a wrong frame.  So the scenarios keep many steps in flight -- nothing is read back before the last
step -- with the lists rebuilt every step, and then compare RngStates(), RenderBuffer(), SampleCounts() and Image() with the
oracle's, FMA and strict.  The RNG states carry every step's draws, so a step that traced the wrong tiles shows at the end.

Frames (tests/test_gpu_owed_rng.py's docstring says what tiles they hold): 256 x 144 and 200 x 136 have >= 128 rows -- split
launches on two streams --, 64 x 24 is one kernel on one stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CAM = dict(angles=(0.0, 0.0), fov=70.0, focal=3.0, aperture=0.05)          # scenes.CONFIGS["C3"]
SPLIT, RAGGED, TINY = (256, 144), (200, 136), (64, 24)
STEPS = 48              # > kFreeEvents x free_stride = 40 builds (a free-event pair is reused) and 6 x the ring's 8 slots
# five cameras (absolute angles) and five lenses (fov, focal, aperture): certain-winner tiles change kind between them
CAMERAS = [(0.0, 0.0), (0.21, -0.13), (-0.3, 0.1), (0.05, 0.4), (-0.12, -0.35)]
LENSES = [(70.0, 3.0, 0.05), (70.0, 3.0, 0.3), (90.0, 2.0, 0.05), (55.0, 4.0, 0.15), (80.0, 3.0, 0.02)]


class Pair:
    """A tracer with list reuse off (every step builds its lists) and the oracle of the same frame, driven in lockstep;
    the oracle only at the end of a scenario has to agree."""

    def __init__(self, R, orc, fma, size, reuse=False, seed=5):
        from raytracertest_amd import scenes
        self.R, self.orc, self.fma, self.seed = R, orc, fma, seed
        self.g = R.RayTracer(size, (0, 0, 0), CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=seed,
                             math_mode=R.MATH_FMA if fma else R.MATH_STRICT)
        self.scene = np.asarray(scenes.cornell32(), np.float32)
        assert self.g.UploadScene(self.scene)
        self.g.SetListReuse(reuse)
        self.angles = (0.0, 0.0)
        self.lens_now = (CAM["fov"], CAM["focal"], CAM["aperture"])
        self._oracle(*size)

    def _oracle(self, W, H):
        orc = self.orc
        self.o = orc.OracleTracer(W, H, (0.0, 0.0), self.lens_now[0], self.lens_now[1], self.lens_now[2], seed=self.seed, nthreads=8,
                                  contract=orc.FMA if self.fma else orc.STRICT)
        self.o.rotate_camera(self.angles)
        assert self.o.upload_scene(self.scene)

    def steps(self, n, samples=4):
        for _ in range(n):
            self.g.TraceEnqueue(1, samples)
            self.o.trace(1, samples)

    def steps_n(self, n, samples=4):                                     # the loop inside the library
        self.g.TraceEnqueueN(1, samples, n)
        for _ in range(n):
            self.o.trace(1, samples)

    def camera(self, angles):
        d = (angles[0] - self.angles[0], angles[1] - self.angles[1])
        self.g.RotateCamera(d)
        self.o.rotate_camera(d)
        self.angles = angles

    def lens(self, fov, focal, aperture):
        self.g.SetCameraParameters(fov, focal, aperture)
        self.o.set_camera_parameters(fov, focal, aperture)
        self.lens_now = (fov, focal, aperture)

    def upload(self, scene):
        self.scene = np.asarray(scene, np.float32)
        assert self.g.UploadScene(self.scene)
        assert self.o.upload_scene(self.scene)

    def resize(self, W, H):
        self.g.Resize((W, H))                                            # new buffers, new states, a new list ring
        self._oracle(W, H)

    def check(self, label):
        g, o = self.g, self.o
        assert np.array_equal(g.RngStates(), o.rng), label + ": RNG states against the oracle"
        assert np.array_equal(g.RenderBuffer().view(np.uint32), o.render.view(np.uint32)), label + ": accumulators against the oracle"
        assert np.array_equal(g.SampleCounts(), o.counts), label + ": sample counts against the oracle"
        assert np.array_equal(g.Image(), o.image), label + ": image against the oracle"


@pytest.fixture(scope="module")
def R():
    import raytracertest_amd as rt
    assert rt.device_count() >= 1
    return rt


MODES = pytest.mark.parametrize("fma", [True, False], ids=["fma", "strict"])


@MODES
def test_48_steps_in_flight(R, orc, fma):
    """Case 1: 48 split steps with a build each, as single calls and as one TraceEnqueueN."""
    p = Pair(R, orc, fma, SPLIT)
    p.steps(STEPS)
    p.check("48 x TraceEnqueue")
    p.steps_n(STEPS)
    p.check("TraceEnqueueN of 48")
    p.g.close()


@MODES
@pytest.mark.parametrize("what", ["camera", "lens", "scene"])
def test_inputs_change_every_fifth_step(R, orc, fma, what):
    """Case 2: the camera, the lens or the scene changes every 5th of 48 steps, nothing read back in between."""
    from raytracertest_amd import scenes
    other = scenes.random_triangles(24, 7)
    p = Pair(R, orc, fma, SPLIT)
    for k in range(STEPS):
        if k % 5 == 0:
            i = (k // 5) % 5
            if what == "camera":
                p.camera(CAMERAS[i])
            elif what == "lens":
                p.lens(*LENSES[i])
            else:
                p.upload(other if (k // 5) % 2 else scenes.cornell32())
        p.steps(1)
    p.check("%s changed every 5th step" % what)
    p.g.close()


@MODES
def test_unsplit_then_resized_to_split(R, orc, fma):
    """Case 3: one kernel on one stream (stream_b has no kernel to carry its free event: it is recorded), then new buffers and
    a new ring for a split frame."""
    p = Pair(R, orc, fma, TINY)
    p.steps(20)
    p.check("64 x 24, 20 steps")
    p.steps(20)
    p.resize(*RAGGED)
    p.steps(20)
    p.check("200 x 136 after the resize")
    p.g.close()


def run_sample_counts(R, orc, fma, size=SPLIT):
    """Case 4: the sample count changes between steps (the sure table, the owed draws per launch)."""
    p = Pair(R, orc, fma, size)
    for rounds in range(6):
        for s in (4, 16, 3, 4):
            p.steps(1, samples=s)
    p.check("sample counts 4, 16, 3, 4")
    p.steps_n(20, samples=3)
    p.check("and 20 steps of 3")
    p.g.close()


@MODES
def test_sample_count_changes(R, orc, fma):
    run_sample_counts(R, orc, fma)


def test_settles_behind_the_trace_kernels():
    """Case 4, with RT_MI355X_OWE_PERIOD=8 in a fresh child process: every 8th owing launch puts settle kernels behind its
    trace kernels, which then are not the last kernels of their streams and may not carry the free events."""
    env = dict(os.environ, RT_MI355X_OWE_PERIOD="8")
    subprocess.run([sys.executable, os.path.abspath(__file__), "owe8"], check=True, env=env, cwd=ROOT, timeout=300)


@MODES
def test_list_reuse_on_then_off(R, orc, fma):
    """Case 5: lists built once and read by 20 steps, then rebuilt by each of 12 more."""
    p = Pair(R, orc, fma, SPLIT, reuse=True)
    p.steps(20)
    p.g.SetListReuse(False)
    p.steps(12)
    p.check("reuse on for 20 steps, off for 12")
    p.g.close()


def test_ring_events_are_not_calls_of_their_own(R, orc):
    """Case 6: the runtime calls per step of split launches with list reuse off, over 32 steps in the steady state.  The
    parent's library has no counter; its enqueue path issues per step a builder launch, a list_ready record, two list_ready
    waits and two trace launches, per fourth step two list_free records and two waits for them, per sixteenth step three
    timing records and two settle launches: 6 + 4 / 4 + 5 / 16 = 7.3 (not measured on its library).  Here neither record may
    appear: both free events of every fourth build are carried by trace kernels, and the figure stays below the parent's."""
    p = Pair(R, orc, True, SPLIT)
    p.steps(16)
    p.g.DebugEnqueueCalls()                                              # (no Sync: it would put the streams' join in between)
    p.steps_n(32)
    c = p.g.DebugEnqueueCalls()
    print("runtime calls over 32 steps:", c)
    assert c["steps"] == 32
    assert c["ready_records"] == 0 and c["free_records"] == 0
    assert c["stop_events"] == 2 * (32 // 4)
    assert c["launches"] >= 3 * 32 and c["waits"] >= 2 * 32
    assert c["calls"] / c["steps"] < 7.3
    p.check("after the counted steps")
    p.g.close()


# The runtime calls of 32 counted steps behind 16 uncounted ones, as the library of the commit before the launch's one body
# issued them (two runs of this sequence with it, selected by RT_MI355X_LIB, agreed in every key).
CALLS_OF_32_STEPS = {
    "one_part": (TINY, None, dict(steps=32, launches=66, records=20, waits=48, ready_records=0, free_records=16, stop_events=8, calls=134)),
    "row_halves": (SPLIT, "0", dict(steps=32, launches=100, records=6, waits=80, ready_records=0, free_records=0, stop_events=16, calls=186)),
    "block_rows": (SPLIT, "1", dict(steps=32, launches=100, records=6, waits=80, ready_records=0, free_records=0, stop_events=16, calls=186)),
}


@pytest.mark.parametrize("shape", list(CALLS_OF_32_STEPS))
def test_every_runtime_call_of_32_steps(R, orc, monkeypatch, shape):
    """Case 7: every counter of DebugEnqueueCalls() for each launch shape enqueue_trace_launch's one body serves -- one part on
    one stream, two row halves, two halves of interleaved block rows -- over 32 steps with list reuse off behind 16 steps
    that are not counted.  The 32 steps hold eight builds that need free events, two timing-sampled launches and two periodic
    settles."""
    size, interleave, expected = CALLS_OF_32_STEPS[shape]
    if interleave is not None:
        monkeypatch.setenv("RT_MI355X_ROW_INTERLEAVE", interleave)
    p = Pair(R, orc, True, size)
    p.steps(16)
    p.g.DebugEnqueueCalls()                                              # (no Sync: it would put the streams' join in between)
    p.steps_n(32)
    c = p.g.DebugEnqueueCalls()
    print("runtime calls over 32 steps, %s:" % shape, c)
    assert c == expected
    p.check("after the counted steps, " + shape)
    p.g.close()


if __name__ == "__main__":                                              # the child of test_settles_behind_the_trace_kernels
    assert sys.argv[1] == "owe8" and os.environ.get("RT_MI355X_OWE_PERIOD") == "8"
    import raytracertest_amd as rt
    from oracle import oracle_py
    oracle_py.lib()
    for mode_fma in (True, False):
        run_sample_counts(rt, oracle_py, mode_fma)
        # One key throughout.  The read after 4 steps pays the debt, so the 8th, 16th, ... owing launch is launch 11, 19, ...:
        # launches whose trace kernels would carry the free events of builds 12, 20, ... were no settle kernels behind them.
        q = Pair(rt, oracle_py, mode_fma, SPLIT)
        q.steps(4)
        q.check("4 steps at period 8")
        q.g.DebugEnqueueCalls()
        q.steps(STEPS - 4)
        calls = q.g.DebugEnqueueCalls()
        assert q.g.DebugOwedState()["settles_enqueued"] >= 10
        # (recorded: build 4, after the read, and builds 12, 20, .. 44; carried: builds 8, 16, .. 48)
        assert calls["free_records"] == 2 * 6 and calls["stop_events"] == 2 * 6, calls
        q.check("48 steps at period 8")
        q.g.close()
