"""The frames and probes on which the project is pinned to the reference's own kernels.  A helper, not a test.

oracle/_ref/libref.so is the reference's RayTracer/Kernels.cuh and the headers it includes, compiled unmodified for the CPU
(oracle/ref_driver.cpp).  tests/golden/make_reference_golden.py runs it over CASES and the two probe sets below and records
what it computes (tests/golden/reference_*.json / .npz); tests/test_reference_parity.py holds the strict oracle -- and the
freshly built library, where there is one -- to those records on the CPU, tests/test_gpu_reference_parity.py the strict HIP
kernels on the device.  Everything here is deterministic and needs neither the library nor the reference.

A case is a frame, a scene, a camera and a sequence of calls on ONE tracer:
  ("trace", iterations, samples)   Trace, which clears the accumulators first (RayTracerImpl.cu:242-249)
  ("rotate", (ax, ay))             RotateCamera
  ("params", fov, focal, aperture) SetCameraParameters
  ("resize", W, H)                 Resize: new buffers, new RNG states from the same seed
and the record is taken after the last call.

The image is compared only where the reference defines it.  Where a ray misses everything the colour is
background * 0.8 + direction * 0.2 (Kernels.cuh:103), negative in a channel for directions that point away from that axis;
the converter hands 255 * mean to a uint8_t parameter (Kernels.cuh:166-168, DeviceUtils.cuh:20), which is undefined for a
negative float in a host compile (gcc wraps: -8 becomes 0xF8) and saturates to 0 on the GPU the reference was written
for.  The project clamps to 0.  So the image mask of a frame is: all three accumulators of the pixel
are >= 0 in the REFERENCE's render buffer.  `min_share` is the least share of the frame that mask must cover, per case, and
is asserted: a mask must not quietly shrink to nothing.  Cases with min_share 1.0 compare every pixel.
"""
import hashlib
import zlib

import numpy as np

SEQ_ONE = lambda it, spp: (("trace", it, spp),)

_C = ("name", "W", "H", "scene", "angles", "fov", "focal", "aperture", "seed", "seq", "min_share", "libm")
CASES = [dict(zip(_C, row)) for row in (
    # 40 x 24: smaller than one 32 x 32 block in y, two blocks in x
    ("c40_cornell_turned", 40, 24, "cornell", (0.1, -0.05), 70.0, 3.0, 0.05, 5, SEQ_ONE(2, 3), 0.84, True),
    ("c40_cornell_closed_fov40", 40, 24, "cornell", (0.0, 0.0), 40.0, 3.0, 0.05, 6, SEQ_ONE(1, 7), 1.0, False),
    ("c40_degenerate_resize_53x37", 40, 24, "five_degenerate", (0.0, 0.0), 70.0, 3.0, 0.05, 7,
     (("trace", 1, 1), ("resize", 53, 37), ("trace", 2, 3)), 0.43, False),
    # 96 x 54: __graft_entry__.smoke()'s frame
    ("c96_cornell", 96, 54, "cornell", (0.0, 0.0), 70.0, 3.0, 0.05, 1, SEQ_ONE(2, 3), 0.79, True),
    ("c96_five_backwards", 96, 54, "five", (0.1, 3.0), 70.0, 3.0, 0.05, 8, SEQ_ONE(1, 3), 0.72, False),
    ("c96_adversarial_two_traces", 96, 54, "adversarial37", (0.1, -0.05), 70.0, 10.0, 0.3, 9,
     (("trace", 1, 3), ("trace", 2, 1)), 0.03, False),
    ("c96_twins_aperture0", 96, 54, "twins", (0.0, 0.0), 40.0, 3.0, 0.0, 10, SEQ_ONE(1, 3), 1.0, False),
    ("c96_cornell_turn_params_trace", 96, 54, "cornell", (0.0, 0.0), 70.0, 3.0, 0.05, 11,
     (("trace", 1, 3), ("rotate", (0.1, 3.0)), ("params", 112.0, 2.5, 0.0), ("trace", 1, 7)), 0.51, True),
    # 236 x 134: small_cases.py's ragged frame -- no multiple of 32 or 8 in x, none of 8 in y; two row bands as devices=[0, 0]
    ("c236_cornell_spp7", 236, 134, "cornell", (0.0, 0.31), 70.0, 3.0, 0.05, 12, SEQ_ONE(1, 7), 0.70, True),
    ("c236_cornell_fov112", 236, 134, "cornell", (0.0, 0.09), 112.0, 3.0, 0.05, 13, SEQ_ONE(2, 1), 0.40, False),
    ("c236_adversarial_turn_params_trace", 236, 134, "adversarial37", (0.1, -0.05), 70.0, 10.0, 0.3, 14,
     (("trace", 1, 1), ("rotate", (0.2, -0.3)), ("params", 40.0, 6.0, 0.4), ("trace", 1, 3)), 0.07, False),
    ("c236_twins_lens", 236, 134, "twins", (0.0, 0.0), 40.0, 3.0, 0.05, 15, SEQ_ONE(2, 3), 1.0, False),
)]
LIBM_FULL = "c40_cornell_turned"        # the libm case whose render buffer is recorded in full (small enough)


def case(name):
    return next(c for c in CASES if c["name"] == name)


def samples_of(c):
    """samples per pixel in the accumulators when the sequence ends: those of the last trace"""
    last = [op for op in c["seq"] if op[0] == "trace"][-1]
    return last[1] * last[2]


def final_size(c):
    W, H = c["W"], c["H"]
    for op in c["seq"]:
        if op[0] == "resize":
            W, H = op[1], op[2]
    return W, H


# ---------------------------------------------------------------------------------------------------------------- scenes
def _rows(tris):
    r = np.zeros((len(tris), 3, 4), np.float32)
    r[:, :, :3] = np.asarray(tris, np.float32)
    return r.reshape(-1, 4)


def twins():
    """A slanted back plane that fills the view of a 40-degree camera at the origin, four times over, and a small triangle in
    front of it.  All coordinates are small dyadic numbers, so every edge is exact.
      0  the plane's triangle A = (v0, v0 + e1, v0 + e2)
      1  A again, bit for bit: ties with 0 at every ray, and draws with it
      2  A with both edges tripled, (v0, v0 + 3 e1, v0 + 3 e2): the same plane, so its t is A's up to the rounding of 9 det
         and 1 / (9 det) -- equal to A's on some rays, an ulp off on others -- and its normalised normal differs from A's in
         the last bit of some channel.  Where t ties, `distance < t` (Kernels.cuh:84) keeps the earlier triangle; a kernel that
         scanned in another order or compared with <= would show the other normal's bits
      3  A with the other winding: culled at every ray (det < 0, Kernels.cuh:42)
      4  a small triangle in front of the plane: what the nearest-hit rule sees instead of the plane"""
    v0 = np.array([-16.0, -12.0, -9.5])
    e1 = np.array([48.0, 1.0, 2.5])
    e2 = np.array([3.0, 44.0, -1.75])
    a = [v0, v0 + e1, v0 + e2]
    tripled = [v0, v0 + 3.0 * e1, v0 + 3.0 * e2]
    front = [np.array([-0.5, -0.375, -4.0]), np.array([0.625, -0.25, -4.5]), np.array([0.0, 0.5, -3.75])]
    return _rows([a, a, tripled, [a[0], a[2], a[1]], front])


def five_degenerate():
    """small_cases.FIVE of the Cornell box and four triangles without area: two equal vertices, three equal vertices, three
    vertices on a line, and three on a line through the view's middle -- det is 0 or rounding noise for every ray"""
    import small_cases
    from raytracertest_amd import scenes
    box = scenes.cornell32().reshape(32, 3, 4)[list(small_cases.FIVE), :, :3]
    p, q = np.array([0.25, -0.5, -2.0]), np.array([-0.75, 0.375, -1.5])
    flat = [[p, p, q], [q, q, q], [p, (p + q) / 2.0, q], [np.array([-0.3, -0.2, -2.0]), np.array([0.0, 0.0, -2.0]), np.array([0.6, 0.4, -2.0])]]
    return np.concatenate([_rows(box), _rows(flat)])


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        import small_cases
        from query_expect import adversarial_scene
        from raytracertest_amd import scenes
        _SCENES[name] = {
            "cornell": scenes.cornell32,
            "five": lambda: scenes.cornell32().reshape(32, 3, 4)[list(small_cases.FIVE)].reshape(-1, 4),
            "adversarial37": lambda: adversarial_scene(37, 3),
            "twins": twins,
            "five_degenerate": five_degenerate,
        }[name]()
        _SCENES[name] = np.ascontiguousarray(_SCENES[name], np.float32)
        _SCENES[name].setflags(write=False)
    return _SCENES[name]


# ---------------------------------------------------------------------------------------------------------------- runs
class OracleRun:
    """the oracle behind the calls of a case (a resize makes a new OracleTracer that keeps camera and scene)"""

    def __init__(self, orc, c, contract=0, hit_mode=0, scene_rows=None):
        self.orc, self.kw = orc, dict(seed=c["seed"], contract=contract, nthreads=4, hit_mode=hit_mode)
        self.o = orc.OracleTracer(c["W"], c["H"], c["angles"], c["fov"], c["focal"], c["aperture"], **self.kw)
        assert self.o.upload_scene(scene(c["scene"]) if scene_rows is None else scene_rows)

    def trace(self, it, spp):
        self.o.trace(it, spp)

    def rotate(self, angles):
        self.o.rotate_camera(angles)

    def params(self, fov, focal, aperture):
        self.o.set_camera_parameters(fov, focal, aperture)

    def resize(self, W, H):
        old = self.o
        self.o = self.orc.OracleTracer(W, H, **self.kw)
        self.o.cam, self.o.tris = old.cam, old.tris

    def buffers(self):
        return self.o.render, self.o.counts, self.o.rng, self.o.image


class RefRun:
    """the compiled reference behind the calls of a case"""

    def __init__(self, ref, c):
        self.r = ref.RefTracer(c["W"], c["H"], c["angles"], c["fov"], c["focal"], c["aperture"], seed=c["seed"])
        assert self.r.upload_scene(scene(c["scene"]))

    def trace(self, it, spp):
        self.r.trace(it, spp)

    def rotate(self, angles):
        self.r.rotate_camera(angles)

    def params(self, fov, focal, aperture):
        self.r.set_camera_parameters(fov, focal, aperture)

    def resize(self, W, H):
        self.r.resize(W, H)

    def buffers(self):
        return self.r.render, self.r.counts, self.r.rng, self.r.image


class HipRun:
    """a RayTracer in strict arithmetic behind the calls of a case; kw: no_binning, devices, ..."""

    def __init__(self, R, c, **kw):
        self.g = R.RayTracer((c["W"], c["H"]), (0, 0, 0), c["angles"], c["fov"], c["focal"], c["aperture"], seed=c["seed"],
                             math_mode=R.MATH_STRICT, **kw)
        assert self.g.UploadScene(scene(c["scene"]))

    def trace(self, it, spp):
        self.g.Trace(it, spp, 0)
        assert self.g.Wait()

    def rotate(self, angles):
        self.g.RotateCamera(angles)

    def params(self, fov, focal, aperture):
        self.g.SetCameraParameters(fov, focal, aperture)

    def resize(self, W, H):
        self.g.Resize((W, H))

    def buffers(self):
        return self.g.RenderBuffer(), self.g.SampleCounts(), self.g.RngStates(), self.g.Image()


def play(run, c):
    """the case's calls on `run`; returns its four buffers"""
    for op in c["seq"]:
        getattr(run, op[0])(*op[1:])
    return run.buffers()


# ---------------------------------------------------------------------------------------------------------------- records
def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def digest(a):
    """a second, independent hash of a buffer's bytes (64 bits of BLAKE2b)"""
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).hexdigest()


def image_mask(render):
    """where the reference defines the image: all three accumulators >= 0 (a NaN is not)"""
    return (np.asarray(render)[..., :3] >= 0.0).all(axis=2)


def crop_of(render):
    """16 x 16 pixels around the frame's middle, as bit patterns, and their origin"""
    H, W = render.shape[:2]
    r0, c0 = max(0, H // 2 - 8), max(0, W // 2 - 8)
    return np.ascontiguousarray(render[r0:r0 + 16, c0:c0 + 16]).view(np.uint32).copy(), [r0, c0]


def record_of(render, counts, rng, image):
    """what is kept of a frame (the crop goes into the .npz)"""
    mask = image_mask(render)
    return {"size": [int(render.shape[1]), int(render.shape[0])],
            "render_crc32": crc(render), "render_digest": digest(render),
            "counts_crc32": crc(counts), "counts_digest": digest(counts),
            "rng_crc32": crc(rng), "rng_digest": digest(rng),
            "mask_crc32": crc(mask.astype(np.uint8)), "mask_share": float(mask.mean()),
            "image_on_mask_crc32": crc(np.where(mask, image, 0).astype(np.uint32)),
            "image_on_mask_digest": digest(np.where(mask, image, 0).astype(np.uint32)),
            "crop_origin": crop_of(render)[1],
            "render_sum": [float(np.asarray(render)[..., k].astype(np.float64).sum()) for k in range(3)]}


def differences(rec, crop, render, counts, rng, image):
    """the names of what differs between a record and four buffers ([] = the buffers are the recorded reference's)"""
    bad = []
    if [int(render.shape[1]), int(render.shape[0])] != rec["size"]:
        return ["size"]
    got = record_of(render, counts, rng, image)
    r0, c0 = rec["crop_origin"]
    if not np.array_equal(np.ascontiguousarray(render[r0:r0 + 16, c0:c0 + 16]).view(np.uint32), crop):
        bad.append("render crop")
    for k in ("render", "counts", "rng", "image_on_mask"):
        if got[k + "_crc32"] != rec[k + "_crc32"] or got[k + "_digest"] != rec[k + "_digest"]:
            bad.append(k)
    if got["mask_crc32"] != rec["mask_crc32"]:
        bad.append("mask")
    return bad


# ---------------------------------------------------------------------------------------------------------------- probes
def _u(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _step(x, k):
    """the float32 k ulps above x (x > 0)"""
    return (np.array([x], np.float32).view(np.uint32) + np.uint32(k)).view(np.float32)[0] if k >= 0 else \
        (np.array([x], np.float32).view(np.uint32) - np.uint32(-k)).view(np.float32)[0]


def hit_probes():
    """(rays (n, 6), triangles (n, 9), group names (n,)): ray i = rt::Ray(origin, direction) against triangle i.
      queries   query_expect.adversarial_rays over adversarial_scene(37, 3): through vertices, edge midpoints and centroids (at
                1e30 and 1e-30 times the length too), nearly in the plane, NaN / inf, a zero direction, random rays
      exact_uv  a unit right triangle in z = -2 under the ray (0, 0, 0) -> (0, 0, -1), shifted so that u and v are EXACTLY the
                listed values: 0, 1, 1/2, a denormal, an ulp outside, and pairs with u + v exactly 1 and an ulp beyond
      det       the same triangle scaled so that det = s * s lies within a few ulp of the culling epsilon 1e-10 on both sides
      tilt      a triangle that holds the ray's line up to a tilt: det from -1e-9 through 0 to 1e-9
      tiny      the exact_uv triangle scaled to denormal coordinates (1e-40 .. 1e-44)
      huge      the same at 2^60, origin and vertices: t overflows where the ray hits
      aimed     tests/adversarial.py: triangles built around the family rays of a camera, each against the ray of the pixel
                and lens point it was aimed at or a neighbour"""
    from query_expect import adversarial_rays, adversarial_scene
    rays, tris, group = [], [], []

    def add(g, ray, tri):
        rays.append(np.asarray(ray, np.float32).reshape(6))
        tris.append(np.asarray(tri, np.float32).reshape(9))
        group.append(g)

    rows = adversarial_scene(37, 3)
    t37 = rows.reshape(-1, 3, 4)[:, :, :3]
    q = adversarial_rays(rows, 300, 4)
    rng = np.random.default_rng(2024)
    per = 7 * 4 + 5                                   # adversarial_rays makes 33 rays per triangle for the first 24
    for i, r in enumerate(q):
        j = i // per if i < 24 * per else int(rng.integers(0, 37))
        add("queries", r, t37[j])
    down = [0, 0, 0, 0, 0, -1]
    one, eps, den = np.float32(1.0), np.float32(2.0 ** -23), _u(1)
    vals = [0.0, -0.0, float(den), -float(den), float(_u(0x00400000)), 0.5, float(_step(one, -1)), 1.0, float(_step(one, 1)), -float(eps),
            0.25, 0.75]
    for a in vals:
        for b in vals:
            if abs(a) <= 1.5 and abs(b) <= 1.5:
                add("exact_uv", down, [[-a, -b, -2], [1 - a, -b, -2], [-a, 1 - b, -2]])
    for a, b in ((0.5, 0.5), (0.25, 0.75), (0.5, float(_step(np.float32(0.5), 1))), (float(_step(np.float32(0.5), -1)), 0.5),
                 (0.75, float(_step(np.float32(0.25), 1))), (1.0, float(den)), (float(den), 1.0), (1.0, 0.0), (0.0, 1.0)):
        add("exact_uv", down, [[-a, -b, -2], [1 - a, -b, -2], [-a, 1 - b, -2]])
    s0 = np.float32(np.sqrt(np.float32(1e-10)))
    for k in range(-6, 7):
        s = float(_step(s0, k))
        add("det", down, [[-0.25 * s, -0.25 * s, -2], [0.75 * s, -0.25 * s, -2], [-0.25 * s, 0.75 * s, -2]])
    for k in range(-3, 4):                            # det = sx * sy with sx fixed: a finer ladder across the epsilon
        sx, sy = 1.0 / 1024.0, float(_step(np.float32(1e-10 * 1024.0), k))
        add("det", down, [[-0.25 * sx, -0.25 * sy, -2], [0.75 * sx, -0.25 * sy, -2], [-0.25 * sx, 0.75 * sy, -2]])
    for tilt in (-1e-9, -1e-10, -9e-11, -1e-12, 0.0, 1e-12, 9e-11, 1e-10, 1.1e-10, 1e-9):
        add("tilt", down, [[-1, tilt, -1], [1, tilt, -1], [0, -tilt, -3]])
        add("tilt", down, [[-1, tilt, -1], [0, -tilt, -3], [1, tilt, -1]])
    for scale in (1e-40, 1e-42, 1e-44):
        for a, b in ((0.25, 0.25), (0.0, 0.5), (1.0, 0.0)):
            tri = np.array([[-a, -b, -2], [1 - a, -b, -2], [-a, 1 - b, -2]], np.float64) * scale
            add("tiny", down, tri)
            add("tiny", [0, 0, 0, 0, 0, -scale], tri)
    big = 2.0 ** 60
    for a, b in ((0.25, 0.25), (0.0, 0.5), (0.5, 0.5), (2.0, 0.25)):
        tri = np.array([[-a, -b, -2], [1 - a, -b, -2], [-a, 1 - b, -2]], np.float64) * big
        add("huge", down, tri)
        add("huge", [0, 0, big, 0, 0, -big], tri)
        add("huge", [big, -big, big, -1, 1, -3], tri)
    import adversarial
    cam = dict(angles=(0.1, -0.05), fov=70.0, focal=3.0, aperture=0.05)
    W, H = 96, 54
    r2 = np.random.default_rng(77)
    aimed = adversarial.adversarial_triangles(r2, cam, W, H, 240, 3.0)
    for tri in aimed:
        px, py = int(r2.integers(0, W)), int(r2.integers(0, H))
        th = r2.uniform(0, 2 * np.pi)
        o, d, _ = adversarial.family_ray(cam, W, H, px, py, (np.cos(th), np.sin(th)))
        add("aimed", np.r_[o, d], tri)
        c = tri.astype(np.float64).mean(axis=0)            # and a ray at the triangle itself, from a lens point
        add("aimed", np.r_[o, c - o], tri)
    return (np.ascontiguousarray(np.array(rays, np.float32)), np.ascontiguousarray(np.array(tris, np.float32)),
            np.array(group))


RAY_CAMERAS = (   # frame, angles, fov, focal, aperture: an unturned camera, the backwards-looking one, aperture 0 at a wide fov
    ((321, 123), (0.0, 0.0), 70.0, 3.0, 0.05),
    ((236, 134), (0.1, 3.0), 40.0, 10.0, 4.0),
    ((40, 24), (-0.7, 2.9), 112.0, 0.5, 0.0),
)
RAYS_PER_CAMERA = 120


def ray_probes(orc):
    """per camera of RAY_CAMERAS: (pixels (n, 2), RNG states (n, 6)) for ThinLensCamera::GetRay -- the frame's corners, its last
    column and row, and random pixels, with states of seed 7 at random subsequences (oracle_py.rng_init, which
    tests/golden/rocrand_xorwow_kats.json pins to rocRAND)"""
    out = []
    for k, ((W, H), _, _, _, _) in enumerate(RAY_CAMERAS):
        rng = np.random.default_rng(100 + k)
        pix = np.stack([rng.integers(0, W, RAYS_PER_CAMERA), rng.integers(0, H, RAYS_PER_CAMERA)], axis=1).astype(np.uint32)
        pix[:4] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        states = np.stack([orc.rng_init(7, int(p)) for p in rng.integers(0, 2 ** 31, RAYS_PER_CAMERA)])
        out.append((pix, states))
    return out


def same_bits(a, b):
    """elementwise: the same float32 bit pattern, or NaN on both sides (x86 and gfx950 give different NaN payloads)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
