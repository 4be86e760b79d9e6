"""bench.py --dump-outputs on a CPU stand-in for the tracer: the last step's buffers, whole when they fit, else the same
seeded pixel sample of every buffer, exact values, at most 64 MB, identical from run to run."""
import os

import numpy as np

import bench


class StandInTracer:
    def __init__(self, width, rows, seed=0):
        r = np.random.default_rng(seed)
        self.width, self.rows = width, rows
        self.image = r.integers(0, 2 ** 32, (rows, width), dtype=np.uint32)
        self.render = r.random((rows, width, 4), dtype=np.float32)
        self.counts = r.integers(0, 257, (rows, width), dtype=np.uint32)
        self.rng = r.integers(0, 2 ** 32, (rows, width, 6), dtype=np.uint32)

    def Image(self):
        return self.image

    def Frame(self):
        return self.image

    def RenderBuffer(self):
        return self.render

    def SampleCounts(self):
        return self.counts

    def RngStates(self):
        return self.rng


class StandInJob:
    world = 1

    def __init__(self, tracer):
        self.tracer = tracer


def sources(t):
    n = t.rows * t.width
    return {"image": t.image.view(np.uint8).reshape(n, 4), "render": t.render.reshape(n, 4), "counts": t.counts.reshape(n),
            "rng": t.rng.reshape(n, 6)}


def written_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_frame_is_written_whole_and_exact(tmp_path):
    t = StandInTracer(64, 32)
    rec = bench.dump_outputs(str(tmp_path), StandInJob(t), 1, 0)
    assert not rec["sampled"] and sorted(os.listdir(tmp_path)) == ["counts.npy", "image.npy", "render.npy", "rng.npy"]
    for name, src in sources(t).items():
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape[:2] == (32, 64)
        assert np.array_equal(a.reshape(src.shape), src.astype(np.float64)), name
    assert np.load(os.path.join(tmp_path, "rng.npy")).dtype == np.float64       # uint32 words need float64


def test_headline_frame_is_a_seeded_sample_within_64_mb(tmp_path):
    t = StandInTracer(1920, 1080)
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    rec = bench.dump_outputs(a_dir, StandInJob(t), 1, 0)
    bench.dump_outputs(b_dir, StandInJob(t), 1, 0)
    assert rec["sampled"] and written_bytes(a_dir) <= 64e6 and rec["bytes"] <= bench.DUMP_BYTES
    idx = np.load(os.path.join(a_dir, "image_pixels.npy"))
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx.size > 0.2 * 1920 * 1080
    for name, src in sources(t).items():
        assert np.array_equal(np.load(os.path.join(a_dir, name + "_pixels.npy")), idx), name      # one pixel set for all
        a = np.load(os.path.join(a_dir, name + ".npy"))
        assert np.array_equal(a, src[idx.astype(np.int64)].astype(np.float64)), name
        assert np.array_equal(a, np.load(os.path.join(b_dir, name + ".npy"))), name              # same sample every run


def test_only_rank_0_writes(tmp_path):
    class Exchange:
        def frame(self, job):
            return None

    job = StandInJob(StandInTracer(8, 8))
    job.world, job.exchange = 2, Exchange()
    assert bench.dump_outputs(str(tmp_path / "r1"), job, 2, 1) is None and not os.path.exists(tmp_path / "r1")
