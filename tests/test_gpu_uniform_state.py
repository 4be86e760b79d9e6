"""The XORWOW Weyl word and the sample count are the same for every pixel of a tracer (tests/test_uniform_state_premise.py),
so the launches carry them as scalars and the tracer fills plane 0 of RT_BUF_RNG and RT_BUF_COUNTS only when somebody reads
them (rt_tracer.hpp: UniformWords::take, rt_tracer::materialise).  Here: after every step of sequences that go through every way the
state advances or resets, RngStates() (all six planes), SampleCounts() and the accumulators equal the oracle's bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAM = dict(angles=(0.0, 0.0), fov=70.0, focal=3.0, aperture=0.05)
DENSE_CAM = dict(angles=(0.1, -0.05), fov=70.0, focal=3.0, aperture=0.05)


@pytest.fixture(scope="module")
def R():
    import raytracertest_amd as rt
    assert rt.device_count() >= 1
    return rt


class Pair:
    """A tracer and the oracle of the same frame, driven in lockstep."""

    def __init__(self, R, orc, W, H, scene, cam=CAM, seed=5, **kw):
        self.R, self.orc, self.cam, self.scene, self.seed = R, orc, cam, np.asarray(scene, np.float32), seed
        self.g = R.RayTracer((W, H), (0, 0, 0), cam["angles"], cam["fov"], cam["focal"], cam["aperture"], seed=seed, **kw)
        assert self.g.UploadScene(self.scene)
        self._oracle(W, H)

    def _oracle(self, W, H):
        c = self.cam
        self.o = self.orc.OracleTracer(W, H, c["angles"], c["fov"], c["focal"], c["aperture"], seed=self.seed, nthreads=8)
        assert self.o.upload_scene(self.scene)

    def check(self, what, image=False):
        g, o = self.g, self.o
        rng, counts = g.RngStates(), g.SampleCounts()
        assert np.array_equal(rng[..., 0], o.rng[..., 0]), what + ": Weyl word (plane 0 of the RNG states)"
        assert np.array_equal(rng, o.rng), what + ": RNG states"
        assert np.array_equal(counts, o.counts), what + ": sample counts"
        assert np.array_equal(g.RenderBuffer().view(np.uint32), o.render.view(np.uint32)), what + ": accumulators"
        if image:
            assert np.array_equal(g.Image(), o.image), what + ": image"
        # a second read without a launch in between takes the planes as they are
        assert np.array_equal(g.SampleCounts(), counts) and np.array_equal(g.RngStates(), rng), what + ": re-read"

    # ---- the ways the state advances or resets
    def launch(self, samples, clear=False, iterations=1):
        self.g.Launch(samples, clear_first=clear, iterations=iterations)
        if clear:
            self.orc.lib().orc_frame_clear(C.byref(self.o._frame))
        for _ in range(iterations):
            self.o.launch(samples)
        self.check("Launch(%d, clear=%s, iterations=%d)" % (samples, clear, iterations))

    def trace(self, iterations, samples, interval=0):
        updates = []
        self.g.SetUpdateCallback((lambda img, size: updates.append(size)) if interval else None)
        self.g.Trace(iterations, samples, interval)
        assert self.g.Wait()
        if interval:
            assert len(updates) == (iterations - 1) // interval
        self.o.trace(iterations, samples)
        self.check("Trace(%d, %d, %d)" % (iterations, samples, interval), image=True)

    def trace_enqueue(self, iterations, samples):
        self.g.TraceEnqueue(iterations, samples)
        self.o.trace(iterations, samples)
        self.check("TraceEnqueue(%d, %d)" % (iterations, samples), image=True)

    def stats(self, samples):
        self.g.TraceStats(samples)                           # clears, then one instrumented launch
        self.orc.lib().orc_frame_clear(C.byref(self.o._frame))
        self.o.launch(samples)
        self.check("TraceStats(%d)" % samples)

    def reseed(self, seed):
        self.g.SetSeed(seed)                                 # new states; accumulators and counts stay
        self.seed = seed
        self.orc.lib().orc_frame_rng_init(C.byref(self.o._frame), seed, 8)
        self.check("SetSeed(%d)" % seed)

    def resize(self, W, H):
        self.g.Resize((W, H))                                # new buffers, new states
        self._oracle(W, H)
        self.check("Resize(%d, %d)" % (W, H))

    def copies_equal_reads(self):
        import torch
        from raytracertest_amd.api import BUF_COUNTS, BUF_RNG
        g = self.g
        rng = torch.zeros((6, g.rows, g.width), dtype=torch.int32, device="cuda")
        counts = torch.zeros((g.rows, g.width), dtype=torch.int32, device="cuda")
        g.CopyToDevice(BUF_RNG, rng.data_ptr(), rng.numel() * 4)
        g.CopyToDevice(BUF_COUNTS, counts.data_ptr(), counts.numel() * 4)
        torch.cuda.synchronize()
        assert np.array_equal(np.moveaxis(rng.cpu().numpy().view(np.uint32), 0, -1), g.RngStates())
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), g.SampleCounts())
        assert np.array_equal(g.RngStates(), self.o.rng) and np.array_equal(g.SampleCounts(), self.o.counts)


def test_small_frame_every_way_the_state_moves(R, orc):
    """96 x 72 (below 128 rows: every launch is one kernel), the Cornell box (SmallLists)."""
    from raytracertest_amd import scenes
    p = Pair(R, orc, 96, 72, scenes.cornell32())
    p.check("fresh tracer")
    p.launch(16, clear=True)
    p.launch(3)
    p.launch(0)                                              # a real launch of no samples
    p.launch(1)
    fuse = p.g.FusedIterations(2)
    assert fuse >= 3
    p.launch(2, iterations=3)                                # fused, accumulating
    p.launch(2, clear=True, iterations=3)                    # fused, clearing
    p.trace(4, 2)                                            # one fused launch
    p.trace(7, 1, 2)                                         # launches cut at the update points
    p.trace(0, 4)                                            # no iteration: clear + convert
    p.launch(5)
    p.stats(3)
    p.launch(2)
    p.trace_enqueue(2, 3)
    p.reseed(11)
    p.launch(4)
    p.resize(80, 40)
    p.launch(2, clear=True)
    p.launch(3)
    p.copies_equal_reads()
    p.g.close()


@pytest.mark.parametrize("interleave", ["0", "1"], ids=["row_halves", "block_rows"])
def test_split_launches(R, orc, monkeypatch, interleave):
    """64 x 160: Launch and TraceEnqueue run two half-frame kernels -- the band's upper and lower rows, or its even and odd
    block rows -- which both get the launch's words (the state advances once per launch, not once per half)."""
    from raytracertest_amd import scenes
    monkeypatch.setenv("RT_MI355X_ROW_INTERLEAVE", interleave)
    p = Pair(R, orc, 64, 160, scenes.cornell32())
    monkeypatch.delenv("RT_MI355X_ROW_INTERLEAVE")
    p.check("fresh tracer")
    p.launch(4, clear=True)
    p.launch(3)
    p.launch(0)
    p.launch(2, iterations=2)
    p.trace_enqueue(3, 2)
    p.trace(5, 1, 2)                                         # (Trace launches are never split)
    p.launch(1)
    p.stats(2)
    p.reseed(3)
    p.launch(2)
    p.copies_equal_reads()
    p.g.close()


def test_dense_scene(R, orc):
    """4 096 random triangles on 128 x 48: the DenseLists kernels (lists and forms from HBM)."""
    from raytracertest_amd import scenes
    p = Pair(R, orc, 128, 48, scenes.random_triangles(4096, 99), cam=DENSE_CAM)
    p.check("fresh tracer")
    p.launch(3, clear=True)
    p.launch(1)
    p.launch(0)
    p.trace(3, 1)                                            # fused
    p.launch(7)
    p.stats(2)                                               # (instrumented launches classify inside the kernel)
    p.copies_equal_reads()
    p.g.close()


def test_two_bands_on_one_device(R, orc):
    """rt_tracer_create_multi with both bands on device 0: each band tracer keeps its own pair of words, the whole-frame
    read assembles the bands' planes."""
    from raytracertest_amd import scenes
    p = Pair(R, orc, 96, 72, scenes.cornell32(), devices=[0, 0])
    assert len(p.g.Bands()) == 2
    p.check("fresh tracer")
    p.launch(4, clear=True)
    p.launch(3)
    p.launch(0)
    p.trace(4, 2)
    p.trace(5, 1, 2)
    p.launch(1)
    p.reseed(9)
    p.launch(2)
    p.resize(64, 50)
    p.trace_enqueue(2, 2)
    p.launch(3)
    p.g.close()
