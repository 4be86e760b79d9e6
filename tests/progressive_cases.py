"""What a progressive Trace(iterationCount, samples, updateInterval) hands to its callbacks, from the oracle alone:
test_progressive_cases.py checks this helper without a device, test_gpu_progressive.py and test_cpp_api.py compare the images the
update and finished callbacks receive with it.  A helper, not a test.  Everything is deterministic and needs no device.

schedule() restates the loop of RayTracerImpl.cu:246-273 -- which iterations are update points -- and how the library cuts that
loop into launches (rt_tracer::trace_funct, multi_trace_funct): a launch ends at the next update point, at the end of its fuse
group, or at the last iteration.  expected() is the reference's loop itself, one oracle launch per iteration, with the oracle's
converted image kept at every update point and after the last iteration.

CASES are the smallest shapes that still reach each seam of the host loop: ragged tiles, the two host images alternating on
every launch, a fuse group that ends between update points on a frame that TraceEnqueue would split, a periodic settle of owed
RNG draws inside the Trace, every kernel path, and the Traces without any update."""
import ctypes

import numpy as np

CAMERA = dict(angles=(0.0, 0.0), fov=70.0, focal=3.0)
SPHERE = np.array([[0.0, 0.0, -2.5, 0.4]], np.float32)
MIN_DIFFERING = 0.02                             # any two images of one case differ in at least this fraction of the pixels


def _case(name, frame, scene, n, spp, interval, aperture=0.3, focal=None, options=None, variants=((0, False),), seed=1, spheres=False,
          rotate=None, lens=None):
    """variants: (math_mode, nearest_hit) pairs the case runs under.  rotate / lens: RotateCamera and SetCameraParameters
    calls made once after the upload (the C++ driver's configuration)."""
    return dict(name=name, frame=frame, scene=scene, n=n, spp=spp, interval=interval, aperture=aperture,
                focal=CAMERA["focal"] if focal is None else focal, options=dict(options or {}), variants=tuple(variants), seed=seed,
                spheres=spheres, rotate=rotate, lens=lens)


BOTH = ((0, False), (1, False))
CASES = [
    _case("classic", (70, 37), "cornell32", 10, 1, 3, aperture=0.05, variants=BOTH + ((0, True),), seed=11),
    _case("every", (70, 37), "cornell32", 7, 2, 1, variants=BOTH, seed=12),
    _case("groups", (96, 136), "cornell32", 150, 1, 100, seed=13),
    _case("settle", (96, 136), "cornell32", 40, 1, 2, seed=14),
    _case("classify", (70, 37), ("random", 300, 777), 9, 3, 4, variants=BOTH, seed=15),
    _case("dense", (70, 37), ("random", 4096, 99), 6, 2, 2, variants=BOTH, seed=16),
    _case("scan", (70, 37), "cornell32", 6, 2, 2, options=dict(no_binning=True), seed=17),
    _case("wide", (38, 21), "demo3", 10, 1, 3, aperture=4.0, focal=10.0, seed=18),
    _case("nofuse", (70, 37), "cornell32", 5, 70, 2, seed=19),
    _case("one", (70, 37), "cornell32", 1, 4, 1, seed=20),
    _case("none", (70, 37), "cornell32", 0, 4, 1, seed=21),
    _case("spheres", (70, 37), "cornell32", 7, 2, 3, spheres=True, seed=22),
]
BY_NAME = {c["name"]: c for c in CASES}
# tests/cpp/mainframe_like.cpp: the reference's caller, its demo scene seen by a rotated camera
CPP = _case("cpp_driver", (38, 21), "demo3", 100, 1, 10, aperture=4.0, focal=10.0, seed=5, rotate=(0.0, 3.0), lens=(70.0, 10.0, 0.5))
# the multi-device handle: classic's and every's arguments on a frame of three bands (16, 17, 17 rows: two of them no whole
# number of tiles).  Only (n, spp, interval) are classic's: its narrow lens leaves images of this frame closer than
# MIN_DIFFERING, so both cases get every's aperture, and their names say so
MULTI = [dict(BY_NAME[name], name=name + "_args_bands_ap0.3", frame=(64, 50), aperture=0.3, variants=((0, False),)) for name in ("classic", "every")]
_SCENES = {}


def scene_rows(case):
    from raytracertest_amd import scenes
    key = case["scene"]
    if key not in _SCENES:
        _SCENES[key] = scenes.random_triangles(key[1], key[2]) if isinstance(key, tuple) else getattr(scenes, key)()
    return _SCENES[key]


def fuse_of(case):
    """rt_tracer::fused_iterations for the case, without a device: at most 64 samples per pixel and launch; the full scan never
    fuses.  (The GPU tests take the number from the tracer.)"""
    return 1 if case["options"].get("no_binning") or case["spp"] == 0 else max(1, 64 // case["spp"])


# ------------------------------------------------------------------------------------------------------------ the loop
def schedule(n, spp, interval, has_update_cb, fuse):
    """(update points, launches).  Update points: the iterations i of RayTracerImpl.cu:256 after which the reference converts
    and calls back.  Launches: (first, last, emit, update) -- the library runs iterations first..last as one launch; `update`:
    last is an update point; `emit`: the launch writes the BGRA8 image (an update or the end of the Trace).  spp does not enter:
    the caller's `fuse` holds what it decides."""
    del spp
    points = [i for i in range(n) if has_update_cb and i > 0 and interval > 0 and i % interval == 0]
    is_update = set(points)
    launches, first = [], 0
    while first < n:
        last_allowed = min(n - 1, first + max(1, fuse) - 1)
        last = first
        while last < last_allowed and last not in is_update:
            last += 1
        update = last in is_update
        launches.append((first, last, update or last + 1 == n, update))
        first = last + 1
    return points, launches


# ------------------------------------------------------------------------------------------------------------ the oracle
def oracle_tracer(orc, case, mode=0, nearest=False):
    W, H = case["frame"]
    o = orc.OracleTracer(W, H, CAMERA["angles"], CAMERA["fov"], case["focal"], case["aperture"], seed=case["seed"], contract=1 - mode,
                         nthreads=8, hit_mode=int(nearest))
    assert o.upload_scene(scene_rows(case))
    if case["spheres"]:
        o.upload_spheres(SPHERE)
    if case["rotate"] is not None:
        o.rotate_camera(case["rotate"])
    if case["lens"] is not None:
        o.set_camera_parameters(*case["lens"])
    return o


def expected(orc, case, o=None, mode=0, nearest=False, n=None, spp=None, interval=None):
    """One Trace(n, spp, interval) of the case with both callbacks set, on the oracle tracer `o` (a new one of the case when
    None; an earlier Trace's continues its RNG stream as the device's does): dict with
      updates   [(i, image)] at every update point, in order
      final     the image after the last iteration (what the finished callback gets and Image() reads)
      render, counts, rng   the oracle's buffers at the end
      o         the oracle tracer, for a Trace behind this one
    n, spp, interval override the case's: n = m gives the state a Trace stopped after m iterations leaves."""
    n = case["n"] if n is None else n
    spp = case["spp"] if spp is None else spp
    interval = case["interval"] if interval is None else interval
    if o is None:
        o = oracle_tracer(orc, case, mode, nearest)
    L = orc.lib()
    points, _ = schedule(n, spp, interval, True, 1)
    L.orc_frame_clear(ctypes.byref(o._frame))                            # RayTracerImpl.cu:242-243
    updates = []
    for i in range(n):                                                   # :246
        o.launch(spp)                                                    # :249
        if i in points:                                                  # :256
            L.orc_convert(ctypes.byref(o._frame))                        # :265
            updates.append((i, o.image.copy()))                          # :272
    L.orc_convert(ctypes.byref(o._frame))                                # :295
    return dict(updates=updates, final=o.image.copy(), render=o.render.copy(), counts=o.counts.copy(), rng=o.rng.copy(), o=o)


def images_of(exp):
    """every image of one expected(): the updates, then the final one unless the last update already is it"""
    out = [("update %d" % i, img) for i, img in exp["updates"]]
    if not out or not np.array_equal(out[-1][1], exp["final"]):
        out.append(("final", exp["final"]))
    return out


def differing(a, b):
    return float(np.mean(a != b))


def fnv1a(image):
    """FNV-1a over the image's pixels as 32-bit words, as tests/cpp/mainframe_like.cpp hashes them"""
    h = 1469598103934665603
    for px in np.asarray(image).ravel():
        h = ((h ^ int(px)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
