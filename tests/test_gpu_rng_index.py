"""RNG state creation and band renders at large pixel indices, up to the last one the library accepts (tests/rng_index_cases.py;
test_rng_index_cases.py proves the table without a device).  rng_init_kernel builds the state of pixel p = x + y * W from the set
bits of p: the frames of the other tests set none above bit 22 against the oracle, so the jump matrices 23..31, the carry of
p0 + base into them, the register path J^stride of a wave's later chunks at such a p0 and the 64-bit seed were checked by nobody.
Every comparison is byte for byte with the oracle's band of the same geometry and seed."""
import numpy as np
import pytest

import rng_index_cases as T
from rng_index_cases import check_render_preconditions, oracle_band, oracle_render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracertest_amd as R
    assert R.device_count() >= 1, "no HIP device: the GPU tests need the real extension"
    return R


def band_tracer(R, case, **kw):
    return R.RayTracer((case.W, case.rows), (0, 0, 0), (0.0, 0.0), seed=case.seed, full_height=case.full_height,
                       row_begin=case.row_begin, **kw)


def assert_states_equal(got, want, case, what="RNG states"):
    """all six words of every pixel; a failure names the first differing pixel by its global index and where the launch put it"""
    assert got.shape == want.shape == (case.rows, case.W, 6), (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=2).reshape(-1))
    if bad.size:
        p = T.pixel_range(case)[0] + int(bad[0])
        blocks, stride, chunk = T.locate(case, p)
        i = int(bad[0])
        pytest.fail("%s of %s: %d of %d pixels differ, the first at global index 0x%x (pixel %d of the band: blocks = %d, stride = %d, "
                    "chunk %d of its wave, lane %d): %s, the oracle has %s" % (what, case.name, bad.size, T.npix(case), p, i, blocks, stride,
                                                                              chunk, i % 64, got.reshape(-1, 6)[i], want.reshape(-1, 6)[i]))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_created_states_equal_the_oracle(rt, orc, case):
    with band_tracer(rt, case) as g:
        assert_states_equal(g.RngStates(), oracle_band(orc, case), case)


def test_the_8k_frame_states_equal_the_oracle_on_its_last_rows(rt, orc):
    """ties test_dense_scene_at_8k_equals_the_full_scan -- the library against itself, same states on both sides -- to the oracle at
    the frame's highest indices without rendering 33 M pixels"""
    case = T.EIGHT_K
    with band_tracer(rt, case) as g:
        assert_states_equal(g.RngStates(), oracle_band(orc, case), case)


def test_set_band_resize_and_set_seed_recreate_the_states_of_the_new_range(rt, orc):
    """One tracer through SetBand, Resize and SetSeed: each has to create the states of the NEW range (p0 = row_begin * W of the
    new geometry) under the seed then in force.  The frame is the crossings' width and high enough for its last row to end above
    0xFFFF0000, as the top band does."""
    W = T.CROSSING_W
    H = (2**32 - 1) // W
    top = T.Case("moved_top", "moved", W, H, H - 2, 2, 11)
    assert T.pixel_range(top)[1] > 0xFFFF0000 and W * H <= 2**32 - 1
    x31 = T.BY_NAME["crossing_bit31"]
    assert x31.W == W and x31.row_begin + x31.rows <= H
    with band_tracer(rt, top) as g:
        assert_states_equal(g.RngStates(), oracle_band(orc, top), top, "states as created")
        step = x31._replace(name="moved_to_bit31", full_height=H, seed=top.seed)
        g.SetBand(step.row_begin, step.rows)
        lo, hi = T.pixel_range(step)
        assert lo < 2**31 < hi
        assert_states_equal(g.RngStates(), oracle_band(orc, step), step, "states after SetBand")
        # another odd width and row count; the band keeps its first row, so p0 moves to row_begin * W'
        W2, rows2 = 4001, 3
        step = step._replace(name="resized", W=W2, rows=rows2)
        assert step.row_begin + rows2 <= H and W2 * H <= 2**32 - 1 and T.pixel_range(step)[0] % 64 != 0
        g.Resize((W2, rows2))
        assert_states_equal(g.RngStates(), oracle_band(orc, step), step, "states after Resize")
        step = step._replace(name="reseeded", seed=2**64 - 1)
        g.SetSeed(step.seed)
        assert_states_equal(g.RngStates(), oracle_band(orc, step), step, "states after SetSeed")


def frame_mismatch(g, o):
    """None, or what differs first between the tracer's four buffers and the oracle's (tests/test_gpu_parity.assert_frame_equal)"""
    for name, got, want in (("SampleCounts", g.SampleCounts(), o.counts), ("RngStates", g.RngStates(), o.rng),
                            ("RenderBuffer", g.RenderBuffer().view(np.uint32), o.render.view(np.uint32)), ("Image", g.Image(), o.image)):
        if got.shape != want.shape:
            return "%s: shape %s vs %s" % (name, got.shape, want.shape)
        bad = np.argwhere(got != want)
        if bad.size:
            return "%s: %d values differ, the first at (row, x, ...) = %s: %s vs the oracle's %s" % (
                name, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return None


@pytest.mark.parametrize("mode", [0, 1], ids=["fma", "strict"])
@pytest.mark.parametrize("rc", T.RENDERS, ids=lambda r: r.name)
def test_bands_at_the_top_of_the_index_range_render_as_the_oracle(rt, orc, rc, mode):
    """Ray generation, tile classification and the certain-winner / owed-draw path where the pixel coordinates and x + y * W are
    as large as they get: Trace(2, 2, 0) of the Cornell box on the last rows of the 65535 x 65537 frame, with the default launch
    and as a full scan, four buffers bit for bit against the oracle.  (The second launch of a Trace owes its certain-winner tiles
    their draws, and a settle runs before the read.)"""
    from raytracertest_amd import scenes
    b, cam = rc.band, T.CAMERA
    o = oracle_render(orc, rc, contract=1 - mode)                        # RT_MATH_FMA = 0 <-> the oracle's contract = 1
    check_render_preconditions(rc, o)
    found = {}
    for label, kw in (("default", {}), ("no_binning", dict(no_binning=True))):
        with rt.RayTracer((b.W, b.rows), (0, 0, 0), rc.angles, cam["fov"], cam["focal"], cam["aperture"], seed=b.seed, math_mode=mode,
                          full_height=b.full_height, row_begin=b.row_begin, **kw) as g:
            assert g.UploadScene(scenes.cornell32())
            g.Trace(T.ITERATIONS, T.SAMPLES, 0)
            assert g.Wait()
            if label == "default":
                count, _, certain = g.DebugTileLists()
                tx = (b.W + 7) // 8                                      # the tiles that hold pixels
                count, certain = count[:, :tx], certain[:, :tx]
                kinds = (int(certain.sum()), int((~certain & (count > 0)).sum()))
                print(rc.name, "certain-winner tiles / traced tiles with candidates:", kinds, "of", count.size)
                assert min(kinds) >= 1, "%s does not test what it says: %s" % (rc.name, kinds)
            found[label] = frame_mismatch(g, o)
    if found["default"] and not found["no_binning"]:
        pytest.fail("%s: the default launch differs from the oracle where the full scan equals it -- the classification: %s"
                    % (rc.name, found["default"]))
    assert found == {"default": None, "no_binning": None}, (rc.name, found)
