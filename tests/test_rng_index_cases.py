"""The bands of tests/rng_index_cases.py hold what they promise, without a device: the index range, the bits they cross, the
launcher's grid and chunk counts; the oracle that tests/test_gpu_rng_index.py compares the device with gives the same states by
its two routes (one jump per row start and one J step per pixel, against one jump per pixel) at the pixels that matter; the
host restatement of the jump table (rth::build_jump_table, the table rng_init_kernel reads) agrees with the oracle matrix by
matrix; and the oracle's frames of the render cases show what the cases say they show."""
import numpy as np
import pytest

import rng_index_cases as T
from rng_index_cases import check_render_preconditions, oracle_band, oracle_render


def family(name):
    return [c for c in T.CASES if c.family == name]


# ------------------------------------------------------------------------------------------------------- the table's properties
def test_the_restated_launch_geometry():
    """launch_rng_init by hand: one block per 512 pixels, rounded down to a power of two, at most 512"""
    G = T.launch_geometry
    assert [G(n) for n in (1, 512, 513, 1024, 1025, 1535, 1537)] == [(1, 512, 1), (1, 512, 1), (2, 1024, 1), (2, 1024, 1),
                                                                        (2, 1024, 2), (2, 1024, 2), (4, 2048, 1)]
    assert G(8198) == (16, 8192, 2) and G(262_144) == (512, 262_144, 1) and G(262_145) == (512, 262_144, 2)
    assert G(819_800) == (512, 262_144, 4) and G(1920 * 1080) == (512, 262_144, 8)


def test_every_case_is_a_band_the_library_accepts_and_is_small():
    assert {c.family for c in T.CASES} == {"top", "crossing", "cap", "grid", "seeds"}
    for c in T.CASES + [T.EIGHT_K]:
        lo, hi = T.pixel_range(c)
        assert c.W * c.full_height <= 2**32 - 1 and c.row_begin + c.rows <= c.full_height and c.rows >= 1, c.name
        assert 0 <= lo < hi <= 2**32 - 1 and hi - lo == T.npix(c) <= T.MAX_PIXELS <= 900_000, c.name
        assert 0 <= c.seed < 2**64, c.name


def test_the_top_bands_end_at_the_last_pixel_the_library_accepts():
    a, b = family("top")
    assert (a.W, a.full_height, a.row_begin, a.rows, a.seed) == (65535, 65537, 65536, 1, 2**64 - 1)
    assert T.pixel_range(a) == (0xFFFF0000, 0xFFFFFFFF)                 # the last pixel: 0xFFFFFFFE
    assert (b.W, b.full_height, b.row_begin, b.rows) == (65535, 65537, 65528, 9)
    assert T.pixel_range(b)[1] == 0xFFFFFFFF and b.rows % 8 == 1         # a partial second tile row
    assert T.geometry(b)[2] >= 2
    assert [c.seed for c in family("seeds")] == [0, 2**32, 0x0123456789ABCDEF]
    assert all(c[2:6] == a[2:6] for c in family("seeds"))


def test_every_bit_from_23_to_31_is_crossed_inside_a_band_that_starts_off_a_multiple_of_64():
    cases = family("crossing")
    assert [T.crossing_bit(c) for c in cases] == list(range(23, 32))
    for c in cases:
        k = T.crossing_bit(c)
        lo, hi = T.pixel_range(c)
        # p0 off a multiple of 64: no wave starts on 2^k, bit k is set by the carry of p0 + base and inside a wave's lanes
        assert lo < 2**k < hi - 1 and lo % 64 != 0 and c.W % 2 == 1, c.name
        assert c.row_begin == 2**k // c.W and c.full_height == c.row_begin + 2, c.name
        after = (2**k - lo) // 64 * 64 + 64                                # the first wave past 2^k: its A has bit k by the carry alone
        assert after < hi - lo and (lo + after) >> k == 1 and (lo | after) != lo + after, c.name
        blocks, stride, chunks = T.geometry(c)
        assert (blocks, chunks, T.npix(c) - stride) == (16, 2, 30), c.name   # the second chunk: one wave, half empty
    # together with the top band, every jump matrix is read with its bit set and clear around the crossing
    for k in range(23, 32):
        lo, hi = T.pixel_range(cases[k - 23])
        assert (lo >> k) & 1 == 0 and ((hi - 1) >> k) & 1 == 1


def test_the_cap_bands_take_four_chunks_per_wave_across_their_bit():
    cases = family("cap")
    assert sorted(T.crossing_bit(c) for c in cases) == [24, 31]
    for c in cases:
        k = T.crossing_bit(c)
        lo, hi = T.pixel_range(c)
        blocks, stride, chunks = T.geometry(c)
        assert T.npix(c) > 2 * 262_144 and blocks == 512 and chunks >= 4, c.name
        assert lo + stride < 2**k < hi - stride and lo % 64 != 0, c.name    # in the interior: not in the first or last chunk


def test_the_grid_bands_sit_on_the_launchers_seams_at_the_end_of_the_index_range():
    cases = family("grid")
    assert {1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1535, 1537} <= {T.npix(c) for c in cases}
    second = {}
    for c in cases:
        n = T.npix(c)
        lo, hi = T.pixel_range(c)
        assert c.rows == 1 and c.W == n and c.row_begin == c.full_height - 1 == (2**32 - 1) // n - 1, c.name
        assert hi > 2**32 - 1 - n and lo >= 2**31, c.name               # the last whole row of n pixels below 2^32 - 1
        blocks, stride, chunks = T.geometry(c)
        assert chunks <= 2
        if chunks == 2:
            second[n] = n - stride
    assert second == T.GRID_SECOND_CHUNK and {1, 511, 513} <= set(second.values())
    for n in second:                                                    # `blocks` a power of two where ceil(npix / 512) is none
        want = -(-n // 512)
        assert want & (want - 1) and T.launch_geometry(n)[0] < want, n
    assert T.launch_geometry(1537) == (4, 2048, 1)                      # ... and is one again: four blocks, one chunk


def test_the_8k_band_is_the_last_rows_of_the_frame_the_self_comparison_renders():
    c = T.EIGHT_K
    assert (c.W, c.full_height, c.row_begin + c.rows) == (7680, 4320, 4320) and 2**24 < T.pixel_range(c)[0] < T.pixel_range(c)[1] < 2**25


# ------------------------------------------------------------------------------------------------------- the oracle's two routes
def _pixels_to_compare(case):
    lo, hi = T.pixel_range(case)
    want = {lo, hi - 1} | {p for k in range(33) for p in (2**k - 1, 2**k, 2**k + 1) if lo <= p < hi}
    _, stride, chunks = T.geometry(case)
    want |= {lo + j * stride + d for j in range(1, chunks) for d in (-1, 0) if lo + j * stride + d < hi}   # chunk seams
    r = np.random.default_rng(lo % 2**31 + T.npix(case))
    want |= {lo + int(i) for i in r.integers(0, hi - lo, 32)}
    return sorted(want)


@pytest.mark.parametrize("case", T.CASES + [T.EIGHT_K], ids=lambda c: c.name)
def test_the_oracles_frame_route_and_its_per_pixel_route_agree(orc, case):
    band = oracle_band(orc, case).reshape(-1, 6)
    lo, _ = T.pixel_range(case)
    for p in _pixels_to_compare(case):
        want = orc.rng_init(case.seed, p)
        assert np.array_equal(band[p - lo], want), "%s: pixel 0x%x: %s (frame) vs %s (per pixel)" % (case.name, p, band[p - lo], want)


# ------------------------------------------------------------------------------------------------------- the host's jump table
@pytest.mark.parametrize("seed", [1, 0xFEDCBA9876543210])
def test_the_host_restatement_agrees_with_the_oracle_matrix_by_matrix(orc, seed):
    """subsequence 2^k reads jump matrix k alone, 2^k - 1 every matrix below it, 2^32 - 2^k every one from k up: a wrong column
    of any one matrix of rth::build_jump_table shows in a vector that no other matrix can mend"""
    from raytracertest_amd import api
    for k in range(32):
        for s in (2**k, 2**k - 1, 2**32 - 2**k):
            got, want = api.dbg_rng_init_host(seed, s), orc.rng_init(seed, s)
            assert np.array_equal(got, want), "seed 0x%x, subsequence 0x%x (k = %d): %s vs %s" % (seed, s, k, got, want)


# ------------------------------------------------------------------------------------------------------- the render cases
def test_the_render_cases_are_the_top_bands_ahead_and_rotated():
    assert [(r.band.name, r.angles) for r in T.RENDERS] == [("top_last_row", (0.0, 0.0)), ("top_last_row", T.ROTATED),
                                                            ("top_last_9_rows", (0.0, 0.0)), ("top_last_9_rows", T.ROTATED)]
    assert (T.ITERATIONS, T.SAMPLES) == (2, 2) and T.MIN_PRIMITIVES >= 4 and T.MIN_COLOURS >= 4


@pytest.mark.parametrize("rc", T.RENDERS, ids=lambda r: r.name)
def test_the_oracles_frame_of_a_render_case_shows_what_the_case_says(orc, rc):
    check_render_preconditions(rc, oracle_render(orc, rc))
