"""The strict HIP kernels against the reference's own kernels.

tests/golden/reference_*.json / .npz hold what the COMPILED reference computed on the cases and probes of
tests/reference_cases.py (see tests/test_reference_parity.py, which holds the oracle to the same records on the CPU).  Here
RayTracer(..., math_mode=MATH_STRICT) goes through each case's calls and must end with the recorded reference's render buffer,
sample counts and RNG states bit for bit, and with its image on the pixels where the reference defines one -- on the default
path, as the plain full scan (no_binning), and for the 236 x 134 frames as two row bands (devices=[0, 0]); and
rt_dbg_hit_triangle and rt_dbg_get_ray must give the recorded answers on the probes.  Reads tests/golden/ only."""
import json
import os

import numpy as np
import pytest

import reference_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "reference_frames.json")) as _f:
    FRAMES = json.load(_f)
CROPS = np.load(os.path.join(GOLDEN, "reference_crops.npz"))
PROBES = np.load(os.path.join(GOLDEN, "reference_probes.npz"))
PATHS = {"default": {}, "full_scan": {"no_binning": True}, "two_bands": {"devices": [0, 0]}}
RUNS = [(c["name"], p) for c in rc.CASES for p in ("default", "full_scan")] + \
       [(c["name"], "two_bands") for c in rc.CASES if (c["W"], c["H"]) == (236, 134)]


@pytest.fixture(scope="module")
def R():
    import raytracertest_amd as rt
    assert rt.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return rt


@pytest.mark.parametrize("name,path", RUNS)
def test_strict_kernels_equal_the_recorded_reference(R, name, path):
    c = rc.case(name)
    run = rc.HipRun(R, c, **PATHS[path])
    render, counts, rng, image = rc.play(run, c)
    key = name + "/built_in"
    assert rc.differences(FRAMES[key], CROPS[key.replace("/", "__")], render, counts, rng, image) == []
    assert float(rc.image_mask(render).mean()) >= c["min_share"]
    if path == "two_bands":
        assert len(run.g.Bands()) == 2
    run.g.close()


def test_hit_triangle_on_the_device_equals_the_recorded_probes(R):
    from raytracertest_amd import api
    rays, tris, group = rc.hit_probes()
    assert [rc.crc(rays), rc.crc(tris)] == PROBES["hit_inputs_crc32"].tolist(), "the probes are not the recorded ones"
    want_hit, want = PROBES["hit"].astype(bool), PROBES["tuv"].view(np.float32)
    hit, tuv, _, _ = api.dbg_hit_triangle(rays, tris, math_mode=api.MATH_STRICT)
    assert np.array_equal(hit, want_hit), (np.flatnonzero(hit != want_hit)[:8], group[hit != want_hit][:8])
    bad = np.flatnonzero(~rc.same_bits(tuv, want).all(axis=1) & want_hit)
    assert bad.size == 0, (bad[:8], group[bad[:8]], tuv[bad[:2]], want[bad[:2]])


def test_get_ray_on_the_device_equals_the_recorded_probes(R, orc):
    for k, ((pix, states), (size, angles, fov, focal, aperture)) in enumerate(zip(rc.ray_probes(orc), rc.RAY_CAMERAS)):
        assert [rc.crc(pix), rc.crc(states)] == PROBES["ray_inputs_crc32_%d" % k].tolist(), "the probes are not the recorded ones"
        g = R.RayTracer(size, (0, 0, 0), angles, fov, focal, aperture, seed=1, math_mode=R.MATH_STRICT)
        rays, st = g.DebugGetRay(pix, states)
        g.close()
        bad = np.flatnonzero((rays.view(np.uint32) != PROBES["rays%d" % k]).any(axis=1))
        assert bad.size == 0, (k, bad[:8], rays[bad[:2]], PROBES["rays%d" % k][bad[:2]].view(np.float32))
        assert np.array_equal(st, PROBES["states%d" % k])
