"""Owed RNG draws (rt_tracer.hpp: RngDebt::owed_draws, rt_tracer::settle; rt_rng_settle.hip).  A small-scene launch whose key equals that of the
launch before it leaves the RNG states of its certain-winner tiles alone and the tracer owes them the draws; whoever needs
the states -- a reader, a launch under another key, another kernel, every RT_MI355X_OWE_PERIOD-th owing launch -- has them
advanced first.  Nothing observable may change: after every step of the scenarios below RngStates(), RenderBuffer(),
SampleCounts() and Image() equal the oracle's (FMA and strict arithmetic) and those of the same library under
RT_MI355X_NO_OWE=1 -- run once, in a fresh child process (this file as a script) -- byte for byte.

The frames are the C3 scene and camera in small: 256 x 144 (18 block rows: a split launch), 200 x 136 (ragged right edge,
partial last block column) and 128 x 72 (one kernel).  Each has to have certain-winner tiles, traced tiles with an empty list
and traced tiles with candidates (test_frames_have_every_kind_of_tile), which decided two details.  Probing the tiles' rays
with the oracle (pixels x 9 lens points: tiles whose rays hit nothing / all hit one triangle and no other / anything else):
200 x 136 at C3's 70 degrees has 0 / 211 / 214 -- the box fills the 1.47 : 1 frame -- so that frame looks through a 90 degree
lens, 102 / 101 / 222; 64 x 24, the smallest frame of one kernel, has 6 / 0 / 18 at 70 degrees and 12 / 0 / 12 at 90 and 100 --
a tile is an eighth of its width -- so the one-kernel frame is 128 x 72 (9 block rows, below the 128 rows of a split):
18 / 32 / 94.  256 x 144: 72 / 227 / 277."""
import ctypes as C
import hashlib
import json
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
WIDE = dict(CAM, fov=90.0)
SPLIT, RAGGED, SMALL = (256, 144), (200, 136), (128, 72)
FRAMES = {"split": SPLIT, "ragged": RAGGED, "small": SMALL}
LENS = {SPLIT: CAM, RAGGED: WIDE, SMALL: CAM}                              # the module docstring says why
SPP = 16
ENV_KEYS = ("RT_MI355X_OWE_PERIOD", "RT_MI355X_ROW_INTERLEAVE")


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


class Pair:
    """A tracer -- and, in the test process, the oracle of the same frame driven in lockstep.  snap() records the digests of
    the four buffers under a label and, with an oracle, compares the buffers with the oracle's."""

    def __init__(self, run, size, *, period=None, interleave=None, reuse=None, scene=None, seed=5, **kw):
        from raytracertest_amd import scenes
        cam = LENS[tuple(size)]
        self.run, self.cam, self.seed, self.kw = run, dict(cam), seed, kw
        self.scene = np.asarray(scenes.cornell32() if scene is None else scene, np.float32)
        self.spheres = None
        env = {"RT_MI355X_OWE_PERIOD": period, "RT_MI355X_ROW_INTERLEAVE": interleave}
        for k, v in env.items():                                         # (the library reads its switches when a tracer is created)
            if v is not None:
                os.environ[k] = str(v)
        try:
            self.g = run.R.RayTracer(size, (0, 0, 0), cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=seed,
                                     math_mode=run.R.MATH_FMA if run.fma else run.R.MATH_STRICT, **kw)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert self.g.UploadScene(self.scene)
        if reuse is not None:
            self.g.SetListReuse(reuse)
        self.o = None
        self._oracle(*size)

    def _oracle(self, W, H):
        orc, c = self.run.orc, self.cam
        if orc is None:
            return
        self.o = orc.OracleTracer(W, H, c["angles"], c["fov"], c["focal"], c["aperture"], seed=self.seed, nthreads=8,
                                  contract=orc.FMA if self.run.fma else orc.STRICT, hit_mode=1 if self.kw.get("nearest_hit") else 0)
        assert self.o.upload_scene(self.scene)
        if self.spheres is not None:
            self.o.upload_spheres(self.spheres)

    def snap(self, label, image=True):
        g, o = self.g, self.o
        bufs = {"rng": g.RngStates(), "render": g.RenderBuffer().view(np.uint32), "counts": g.SampleCounts(), "image": g.Image()}
        assert label not in self.run.digests, label
        self.run.digests[label] = {k: digest(v) for k, v in bufs.items()}
        if o is not None:
            assert np.array_equal(bufs["rng"], o.rng), label + ": RNG states against the oracle"
            assert np.array_equal(bufs["render"], o.render.view(np.uint32)), label + ": accumulators against the oracle"
            assert np.array_equal(bufs["counts"], o.counts), label + ": sample counts against the oracle"
            if image:
                assert np.array_equal(bufs["image"], o.image), label + ": image against the oracle"
        return bufs

    # ---- what a caller can do to a tracer, mirrored on the oracle
    def steps(self, n, iterations=1, samples=SPP):
        for _ in range(n):
            self.g.TraceEnqueue(iterations, samples)
            if self.o is not None:
                self.o.trace(iterations, samples)

    def launch(self, samples, clear=False, iterations=1):
        self.g.Launch(samples, clear_first=clear, iterations=iterations)
        if self.o is not None:
            if clear:
                self.run.orc.lib().orc_frame_clear(C.byref(self.o._frame))
            for _ in range(iterations):
                self.o.launch(samples)

    def rotate(self, angles):
        self.g.RotateCamera(angles)
        if self.o is not None:
            self.o.rotate_camera(angles)

    def lens(self, fov, focal, aperture):
        self.g.SetCameraParameters(fov, focal, aperture)
        if self.o is not None:
            self.o.set_camera_parameters(fov, focal, aperture)

    def upload_spheres(self, spheres):
        self.spheres = np.asarray(spheres, np.float32)
        self.g.UploadSpheres(self.spheres)
        if self.o is not None:
            self.o.upload_spheres(self.spheres)

    def upload_scene(self, scene):
        self.scene = np.asarray(scene, np.float32)
        assert self.g.UploadScene(self.scene)
        if self.o is not None:
            assert self.o.upload_scene(self.scene)

    def stats(self, samples):
        self.g.TraceStats(samples)                                       # clears, then one instrumented launch
        if self.o is not None:
            self.run.orc.lib().orc_frame_clear(C.byref(self.o._frame))
            self.o.launch(samples)

    def resize(self, W, H):
        self.g.Resize((W, H))                                            # new buffers, new states
        self._oracle(W, H)

    def reseed(self, seed):
        self.g.SetSeed(seed)
        self.seed = seed
        if self.o is not None:
            self.run.orc.lib().orc_frame_rng_init(C.byref(self.o._frame), seed, 8)


class Run:
    def __init__(self, R, orc, fma):
        self.R, self.orc, self.fma, self.digests = R, orc, fma, {}

    def pair(self, size, **kw):
        return Pair(self, size, **kw)


# ---- the scenarios: name -> function(run); every snap label is unique within a scenario ------------------------------------

def sc_period(run):
    """(a) owing across the period: period 3, seven steps -- the first owes nothing, the fourth and the seventh settle on
    their way -- and an eighth, whose draws are left to the reader."""
    for name, size in FRAMES.items():
        for reuse in (False, True):
            p = run.pair(size, period=3, reuse=reuse)
            p.steps(7)
            p.snap("%s reuse=%d, 7 steps" % (name, reuse))
            p.steps(1)
            p.snap("%s reuse=%d, 8 steps" % (name, reuse))
            p.steps(5)                                                   # one periodic settle, two launches left
            p.snap("%s reuse=%d, 13 steps" % (name, reuse))
            p.g.close()


def sc_table(run):
    """(b) the read-back settles through a table (draws above the stepping threshold of 96) and by stepping."""
    for name, size in FRAMES.items():
        p = run.pair(size, period=1000)
        p.steps(6)                                                       # five owing launches x 48 draws
        p.snap(name + " table 240")
        p.steps(3)                                                       # (the launches after a read owe again)
        p.snap(name + " table 144")
        p.steps(2)
        p.snap(name + " stepped 96")
        p.launch(1)
        p.launch(1)
        p.snap(name + " stepped 6", image=False)
        p.g.close()


def sc_camera(run):
    """(c) a certain tile becomes a traced tile: the camera or the lens moves after five owing steps."""
    for name, size in FRAMES.items():
        p = run.pair(size, period=4)
        p.steps(6)
        p.rotate((0.21, -0.13))
        p.steps(2)
        p.snap(name + " rotated")
        p.steps(5)
        p.lens(p.cam["fov"], 3.0, 0.3)
        p.steps(2)
        p.snap(name + " aperture")
        p.g.close()


def sc_consumer(run):
    """(d) after three owing steps somebody else handles the states."""
    from raytracertest_amd import scenes
    for name, size in (("split", SPLIT), ("small", SMALL)):
        p = run.pair(size, period=1000)
        p.steps(4)
        p.upload_spheres([[0.2, -0.1, -2.0, 0.4]])
        p.steps(1)
        p.snap(name + " spheres")
        p.upload_spheres(np.zeros((0, 4), np.float32))
        p.steps(4)
        p.upload_scene(scenes.random_triangles(4096, 99))                # the dense-scene kernels
        p.steps(1, samples=2)
        p.snap(name + " dense")
        p.upload_scene(scenes.cornell32())
        p.steps(4)
        p.stats(3)
        p.snap(name + " stats", image=False)
        p.steps(4)
        p.resize(96, 40)
        p.steps(2)
        p.resize(*size)
        p.steps(4)
        p.snap(name + " resized")
        p.reseed(11)
        p.snap(name + " reseeded")
        p.steps(3)
        p.snap(name + " after reseed")
        p.g.close()
        for flag in ("no_sure_hit", "no_binning"):                       # tracers that never owe
            q = run.pair(size, period=1000, **{flag: True})
            q.steps(4)
            q.snap("%s %s" % (name, flag))
            q.g.close()


def sc_samples(run):
    """(e) sample counts and fused iterations mixed within one key."""
    for name, size in FRAMES.items():
        p = run.pair(size, period=5)
        assert p.g.FusedIterations(2) >= 3
        p.launch(16, clear=True)
        for k, s in enumerate((1, 2, 3, 16, 3, 1)):
            p.launch(s)
            if k % 2:
                p.snap("%s launch %d of %d" % (name, k, s), image=False)
        p.launch(2, iterations=3)
        p.launch(3)
        p.launch(1, iterations=3)
        p.snap(name + " fused", image=False)
        p.launch(2, clear=True, iterations=3)
        p.launch(0)
        p.launch(16)
        p.snap(name + " fused, cleared", image=False)
        p.g.close()


def sc_bands(run):
    """(g) three row bands in one process on one device after five steps, (h) both kinds of halves of a split launch."""
    p = run.pair(SPLIT, period=3, devices=[0, 0, 0])
    p.steps(5)
    p.snap("three bands")
    p.g.close()
    for il in ("0", "1"):
        q = run.pair(SPLIT, period=3, interleave=il)
        q.steps(5)
        q.snap("interleave " + il)
        q.steps(3)
        q.snap("interleave " + il + ", 8 steps")
        q.g.close()


SCENARIOS = {"period": sc_period, "table": sc_table, "camera": sc_camera, "consumer": sc_consumer, "samples": sc_samples,
             "bands": sc_bands}


def run_scenario(R, orc, name, fma):
    run = Run(R, orc, fma)
    SCENARIOS[name](run)
    return run.digests


# ---- the tests --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def R():
    import raytracertest_amd as rt
    assert rt.device_count() >= 1
    return rt


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """Every scenario under RT_MI355X_NO_OWE=1, in a fresh child process: {scenario/mode: {label: digests}}."""
    out = tmp_path_factory.mktemp("owed") / "reference.json"
    env = dict(os.environ, RT_MI355X_NO_OWE="1")
    for k in ENV_KEYS:
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], check=True, env=env, cwd=ROOT, timeout=600)
    with open(out) as f:
        return json.load(f)


def test_frames_have_every_kind_of_tile(R):
    for name, size in FRAMES.items():
        cam = LENS[size]
        g = R.RayTracer(size, (0, 0, 0), cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=5)
        from raytracertest_amd import scenes
        assert g.UploadScene(scenes.cornell32())
        g.TraceEnqueue(1, SPP)
        count, _, certain = g.DebugTileLists()
        tx = (size[0] + 7) // 8                                          # tiles that hold pixels (the last block may be partial)
        count, certain = count[:, :tx], certain[:, :tx]
        kinds = (int(certain.sum()), int((~certain & (count == 0)).sum()), int((~certain & (count > 0)).sum()))
        print(name, size, "certain / traced and empty / traced with candidates:", kinds)
        assert min(kinds) >= 1, (name, kinds)
        g.close()


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "strict"])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(R, orc, reference, name, fma):
    got = run_scenario(R, orc, name, fma)                                # (asserts against the oracle on the way)
    want = reference["%s/%s" % (name, "fma" if fma else "strict")]
    assert sorted(got) == sorted(want)
    for label in got:
        assert got[label] == want[label], "%s: differs from the same library under RT_MI355X_NO_OWE=1" % label


def test_debt_is_owed_and_paid(R, monkeypatch):
    """The mechanism itself: launches under one key owe 3 x samples draws each, the period-th pays on the way, a read pays
    the rest, and a second read enqueues nothing."""
    from raytracertest_amd import scenes
    monkeypatch.setenv("RT_MI355X_OWE_PERIOD", "4")
    g = R.RayTracer(SPLIT, (0, 0, 0), CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=5)
    monkeypatch.delenv("RT_MI355X_OWE_PERIOD")
    assert g.UploadScene(scenes.cornell32())
    g.TraceEnqueue(1, SPP)                                               # the first launch under a key runs as ever
    assert g.DebugOwedState()["owed_draws"] == 0
    g.TraceEnqueue(1, SPP); g.TraceEnqueue(1, 2)
    s = g.DebugOwedState()
    assert (s["owed_draws"], s["owing_launches"], s["settles_enqueued"]) == (3 * SPP + 3 * 2, 2, 0)
    g.TraceEnqueue(1, SPP); g.TraceEnqueue(1, SPP)                       # the fourth owing launch: one settle per half
    s = g.DebugOwedState()
    assert (s["owed_draws"], s["owing_launches"], s["settles_enqueued"]) == (0, 0, 2)
    g.TraceEnqueue(1, SPP)
    assert g.DebugOwedState()["owed_draws"] == 3 * SPP
    g.RngStates()
    s = g.DebugOwedState()
    assert (s["owed_draws"], s["settles_enqueued"]) == (0, 3)
    g.RngStates(); g.SampleCounts(); g.RenderBuffer(); g.Image()
    assert g.DebugOwedState()["settles_enqueued"] == 3                   # nothing owed: no kernel
    g.RotateCamera((0.1, 0.0))                                           # interactive use never owes
    for _ in range(3):
        g.TraceEnqueue(1, SPP)
        g.RotateCamera((0.01, 0.0))
    s = g.DebugOwedState()
    assert (s["owed_draws"], s["settles_enqueued"]) == (0, 3)
    g.close()


def _hip():
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise AssertionError("the HIP runtime the library is linked against is not loadable by its soname")


def test_read_back_paths(R, orc):
    """(f) DevicePointer(RT_BUF_RNG) and CopyToDeviceAsync directly after owing steps hand out the settled planes."""
    import torch
    from raytracertest_amd import scenes
    from raytracertest_amd.api import BUF_RNG
    W, H = SPLIT
    o = orc.OracleTracer(W, H, CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=5, nthreads=8)
    assert o.upload_scene(scenes.cornell32())
    g = R.RayTracer(SPLIT, (0, 0, 0), CAM["angles"], CAM["fov"], CAM["focal"], CAM["aperture"], seed=5)
    assert g.UploadScene(scenes.cornell32())
    for _ in range(4):
        g.TraceEnqueue(1, SPP); o.trace(1, SPP)
    assert g.DebugOwedState()["owed_draws"] == 3 * 3 * SPP
    dst = torch.zeros((6, H, W), dtype=torch.int32, device="cuda")
    g.CopyToDeviceAsync(BUF_RNG, dst.data_ptr(), dst.numel() * 4)
    assert g.DebugOwedState()["owed_draws"] == 0
    g.Sync(); torch.cuda.synchronize()
    assert np.array_equal(np.moveaxis(dst.cpu().numpy().view(np.uint32), 0, -1), o.rng)
    for _ in range(3):
        g.TraceEnqueue(1, SPP); o.trace(1, SPP)
    settles = g.DebugOwedState()["settles_enqueued"]
    ptr = g.DevicePointer(BUF_RNG)
    s = g.DebugOwedState()
    assert ptr and (s["owed_draws"], s["settles_enqueued"]) == (0, settles + 1)
    g.Sync()
    host = np.zeros((6, H, W), np.uint32)
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    assert np.array_equal(np.moveaxis(host, 0, -1), o.rng)
    assert g.DevicePointer(BUF_RNG) == ptr and g.DebugOwedState()["settles_enqueued"] == settles + 1   # a second hand-out: no kernel
    assert np.array_equal(g.RngStates(), o.rng) and np.array_equal(g.RenderBuffer().view(np.uint32), o.render.view(np.uint32))
    g.close()


if __name__ == "__main__":                                              # the reference arm: python tests/test_gpu_owed_rng.py OUT.json
    assert os.environ.get("RT_MI355X_NO_OWE") == "1"
    import raytracertest_amd as rt
    res = {}
    for sc_name in sorted(SCENARIOS):
        for mode_fma in (True, False):
            res["%s/%s" % (sc_name, "fma" if mode_fma else "strict")] = run_scenario(rt, None, sc_name, mode_fma)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
