"""Row bands that put RNG STATE CREATION (csrc/rt_rng_init.hip) and the render path on large pixel indices, up to the last one
the library accepts, 2^32 - 2.  A helper, not a test: test_rng_index_cases.py proves without a device that every case holds
what it promises, test_gpu_rng_index.py runs them.  Plain data and integer arithmetic; needs no device and no oracle.

A pixel's XORWOW state is curand_init(seed, subsequence = x + y * W, 0).  rng_init_kernel builds it from A = p0 + base
(p0 = row_begin * W, base = the wave's first pixel of the band): a cooperative product by J^(2^k) for every set bit k < 32 of A,
a per-lane window-table product for the low six bits, and ONE fixed jump J^stride from a wave's chunk to its next.  Frames of a
few thousand rows set no bit above 22, so the families here are

  top        the last rows of a 65535 x 65537 frame: indices up to 0xFFFFFFFE, every jump matrix at once, seed 2^64 - 1
  crossing   for every k in 23..31 a two-row band of odd width that holds pixel 2^k strictly inside and starts off a multiple of
             64 (the carry of p0 + base runs into bit k); 8222 pixels = 16 blocks and a second chunk of 30 pixels
  cap        more than 2 x 262 144 pixels (the grid's cap of 512 blocks: 4 chunks per wave) across 2^31 and across 2^24
  grid       one-row bands of W = npix pixels at the very end of the index range, for the pixel counts at which the launcher's grid
             changes: one lane, a partial wave, a block, and `blocks` staying a power of two while ceil(npix / 512) is none
  seeds      the top row again under seeds 0, 2^32 and a 64-bit pattern (the scramble is host code fed through rt_options)

Every case keeps W * full_height <= 2^32 - 1 and at most MAX_PIXELS pixels: far below the 2^32 - 2^19 pixels per tracer at
which the kernel's 32-bit chunk loop would wrap (the library refuses those: test_abi.py), and a fraction of a second on
either side."""
from collections import namedtuple

Case = namedtuple("Case", "name family W full_height row_begin rows seed")

MAX_INDEX = 2**32 - 1                            # W * full_height may not exceed it: the last pixel index is 2^32 - 2
MAX_PIXELS = 900_000
THREADS = 512                                    # of a block of rng_init_kernel: 8 waves, a chunk of 64 pixels each
MAX_BLOCKS = 512
ODD_W = 4099
# the crossings' width: with 4099 (and 4097 ... 4109) the bands of bits 30 and 31 start ON a multiple of 64 -- 2^k mod W is one
# then -- and no carry runs into the bit; 4111 leaves p0 mod 64 = 8, 31, 62, 60, 56, 48, 47, 45, 41 for k = 23 .. 31
CROSSING_W = 4111
CROSSING_BITS = tuple(range(23, 32))
GRID_NPIX = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2561)
# the grid sizes with a second chunk -> its pixels.  (1537 has none: ceil(1537 / 512) = 4 is a power of two again, 4 blocks.)
GRID_SECOND_CHUNK = {1025: 1, 1535: 511, 1536: 512, 2561: 513}


def launch_geometry(npix):
    """(blocks, stride, chunks per wave) as launch_rng_init chooses them: one block per 512 pixels, rounded DOWN to a power of
    two and capped at 512 blocks; a wave's chunks lie stride = 512 * blocks pixels apart"""
    want = -(-npix // THREADS)
    blocks = 1
    while blocks < MAX_BLOCKS and blocks * 2 <= want:
        blocks *= 2
    stride = THREADS * blocks
    return blocks, stride, -(-npix // stride)


def pixel_range(case):
    """(lo, hi): the global indices lo <= p < hi of the band's pixels"""
    lo = case.row_begin * case.W
    return lo, lo + case.rows * case.W


def npix(case):
    return case.rows * case.W


def geometry(case):
    return launch_geometry(npix(case))


def locate(case, p):
    """(blocks, stride, chunk): the launch of the case and which chunk of its wave wrote global pixel p"""
    blocks, stride, _ = geometry(case)
    return blocks, stride, (p - pixel_range(case)[0]) // stride


def _crossing(k, W=CROSSING_W, rows=2):
    row0 = 2**k // W
    return Case("crossing_bit%d" % k, "crossing", W, row0 + rows, row0, rows, 1000 + k)


def _cap(k, W=ODD_W, rows=200):
    row0 = (2**k - 400_000) // W
    return Case("cap_across_bit%d" % k, "cap", W, row0 + rows, row0, rows, 77 + k)


def _grid(n):
    H = MAX_INDEX // n
    return Case("grid_npix%d" % n, "grid", n, H, H - 1, 1, 5)


TOP_ROW = Case("top_last_row", "top", 65535, 65537, 65536, 1, 2**64 - 1)
TOP_ROWS = Case("top_last_9_rows", "top", 65535, 65537, 65528, 9, 7)
SEEDS = (0, 2**32, 0x0123456789ABCDEF)

CASES = ([TOP_ROW, TOP_ROWS] + [_crossing(k) for k in CROSSING_BITS] + [_cap(31), _cap(24)] + [_grid(n) for n in GRID_NPIX] +
         [TOP_ROW._replace(name="seed_%x" % s, family="seeds", seed=s) for s in SEEDS])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def crossing_bit(case):
    return int(case.name.rsplit("bit", 1)[1])


# the last rows of the 8K frame whose default launch test_gpu_round4 compares with its own full scan: indices just under 2^25
EIGHT_K = Case("8k_last_rows", "8k", 7680, 4320, 4312, 8, 1)

# ---- renders at the top of the index range -------------------------------------------------------------------------------------
# scenes.cornell32() through the C3 camera.  Unrotated, the last rows of the square frame look 35 degrees down: the floor's two
# triangles and, in the 9 rows, a strip of the left wall.  ROTATED was chosen with the oracle's tile probe: the band then shows
# the back wall, both triangles of the left wall, the floor and the background (test_rng_index_cases.py counts them).
CAMERA = dict(fov=70.0, focal=3.0, aperture=0.05)
ITERATIONS, SAMPLES = 2, 2                       # Trace(2, 2, 0): the second launch owes its certain-winner tiles' draws
ROTATED = (0.3, 0.3)
MIN_PRIMITIVES, MIN_COLOURS = 4, 4
RenderCase = namedtuple("RenderCase", "name band angles")
RENDERS = tuple(RenderCase(b.name + tag, b, a) for b in (TOP_ROW, TOP_ROWS) for tag, a in (("_ahead", (0.0, 0.0)), ("_rotated", ROTATED)))

# ---- the oracle's side, made once per session and shared by both test modules (orc: the `orc` fixture) -------------------------
_BANDS, _FRAMES = {}, {}


def oracle_band(orc, case):
    """the oracle's states of the band (rows, W, 6), read-only"""
    if case not in _BANDS:
        o = orc.OracleTracer(case.W, case.full_height, row0=case.row_begin, rows=case.rows, seed=case.seed, nthreads=8)
        o.rng.setflags(write=False)
        _BANDS[case] = o.rng
    return _BANDS[case]


def oracle_render(orc, rc, contract=1):
    """the oracle's tracer of a render case after Trace(ITERATIONS, SAMPLES), its buffers read-only"""
    if (rc, contract) not in _FRAMES:
        from raytracertest_amd import scenes
        b = rc.band
        o = orc.OracleTracer(b.W, b.full_height, rc.angles, CAMERA["fov"], CAMERA["focal"], CAMERA["aperture"], seed=b.seed,
                             row0=b.row_begin, rows=b.rows, contract=contract, nthreads=8)
        assert o.upload_scene(scenes.cornell32())
        o.trace(ITERATIONS, SAMPLES)
        for a in (o.render, o.counts, o.rng, o.image):
            a.setflags(write=False)
        _FRAMES[rc, contract] = o
    return _FRAMES[rc, contract]


def check_render_preconditions(rc, o):
    """On the oracle's output alone: every pixel sampled, no NaN, at least MIN_COLOURS colours (the background is a gradient,
    so colours alone say little), and for the rotated cases MIN_PRIMITIVES triangles that win rays of the band's first and last
    row through the lens centre, beside rays that meet nothing."""
    import numpy as np
    assert not np.isnan(o.render).any(), rc.name
    assert np.all(o.counts == ITERATIONS * SAMPLES), rc.name
    colours = np.unique(o.image)
    assert colours.size >= MIN_COLOURS, (rc.name, colours.size)
    if rc.angles != (0.0, 0.0):
        b = rc.band
        pixels = [(x, y) for y in sorted({b.row_begin, b.row_begin + b.rows - 1}) for x in range(0, b.W, 31)]
        probe, nohit = o.tile_probe(pixels, [(0.0, 0.0)])
        winners = np.flatnonzero(probe["wins"])
        print(rc.name, "colours", colours.size, "winning primitives", winners.tolist(), "rays on the background", nohit)
        assert winners.size >= MIN_PRIMITIVES and nohit > 0, (rc.name, winners.tolist(), nohit)
