"""ctypes binding of the compiled reference (oracle/_ref/libref.so: the reference's own kernel headers built for the
CPU by `make -C oracle ref`, see oracle/ref_driver.cpp).

TEST INFRASTRUCTURE: only tests/ and tests/golden/make_reference_golden.py load it.  The library exists only where the
build found a reference checkout (or where a build's oracle/_ref/ was carried along); available() tells.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(_HERE, "_ref", "libref.so")
STAMP = os.path.join(_HERE, "_ref", "libref.stamp")
SINCOS = C.CFUNCTYPE(None, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float))

_lib = None


def build():
    """`make ref`: builds the library where there is a reference checkout, keeps what is there otherwise; never raises for a
    missing reference."""
    subprocess.run(["make", "-s", "-C", _HERE, "ref"], check=True)
    return SO if os.path.exists(SO) else None


def available():
    return os.path.exists(SO)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO)
        f32p, u32p, i32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p
        L.ref_set_trig.argtypes = [vp]
        L.ref_create.argtypes = [C.c_uint32, C.c_uint32, f32p, f32p, C.c_float, C.c_float, C.c_float, C.c_uint64]
        L.ref_create.restype = vp
        L.ref_destroy.argtypes = [vp]
        L.ref_upload.argtypes = [vp, f32p, C.c_uint32]
        L.ref_upload.restype = C.c_int
        L.ref_trace.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.ref_rotate.argtypes = [vp, f32p]
        L.ref_set_camera_parameters.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        L.ref_resize.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.ref_size.argtypes = [vp, u32p]
        L.ref_read_render.argtypes = [vp, f32p]
        L.ref_read_counts.argtypes = [vp, u32p]
        L.ref_read_image.argtypes = [vp, u32p]
        L.ref_read_states.argtypes = [vp, u32p]
        L.ref_hit_triangle.argtypes = [C.c_uint32, f32p, f32p, i32p, f32p, f32p, f32p]
        L.ref_get_ray.argtypes = [vp, C.c_uint32, u32p, u32p, f32p]
        for f in (L.ref_set_trig, L.ref_destroy, L.ref_trace, L.ref_rotate, L.ref_set_camera_parameters, L.ref_resize,
                  L.ref_size, L.ref_read_render, L.ref_read_counts, L.ref_read_image, L.ref_read_states, L.ref_hit_triangle,
                  L.ref_get_ray):
            f.restype = None
        _lib = L
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def set_trig(trig):
    """What stands behind glm::sin / glm::cos / glm::tan in the compiled reference, for everything it computes from now on:
    "libm" -- sinf, cosf, tanf; "oracle" -- the project's build-owned sincos (liboracle's orc_sincos; tan = sin / cos)."""
    if trig == "libm":
        lib().ref_set_trig(None)
    elif trig == "oracle":
        from oracle import oracle_py
        lib().ref_set_trig(C.cast(oracle_py.lib().orc_sincos, C.c_void_p))
    else:
        raise ValueError(trig)


def hit_triangle(rays, tris):
    """rt::HitTriangle of rt::Ray(rays[i, :3], rays[i, 3:]) against the triangle tris[i] (v0, v1, v2): hit (bool), t, u, v."""
    r = _f32(rays).reshape(-1, 6)
    t9 = _f32(tris).reshape(-1, 9)
    n = r.shape[0]
    assert t9.shape[0] == n
    hit = np.zeros(n, np.int32)
    t, u, v = (np.zeros(n, np.float32) for _ in range(3))
    lib().ref_hit_triangle(n, _fp(r), _fp(t9), hit.ctypes.data_as(C.POINTER(C.c_int32)), _fp(t), _fp(u), _fp(v))
    return hit.astype(bool), t, u, v


class RefTracer:
    """The reference's RayTracerImpl as far as it can be compiled: its camera object and its two kernels over the four buffers
    (ref_driver.cpp says which lines the driver supplies)."""

    def __init__(self, width, height, angles=(0.0, 0.0), fov_deg=70.0, focal=10.0, aperture=4.0, seed=1, position=(0.0, 0.0, 0.0)):
        self._h = lib().ref_create(int(width), int(height), _fp(_f32(position)), _fp(_f32(angles)), fov_deg, focal, aperture, seed)
        assert self._h

    def close(self):
        if self._h:
            lib().ref_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def size(self):
        wh = np.zeros(2, np.uint32)
        lib().ref_size(self._h, _up(wh))
        return int(wh[0]), int(wh[1])

    def upload_scene(self, float4s):
        a = _f32(float4s).reshape(-1, 4)
        return bool(lib().ref_upload(self._h, _fp(a), a.shape[0]))

    def trace(self, iterations, samples_per_iteration):
        lib().ref_trace(self._h, iterations, samples_per_iteration)

    def rotate_camera(self, dangles):
        lib().ref_rotate(self._h, _fp(_f32(dangles)))

    def set_camera_parameters(self, fov_deg, focal, aperture):
        lib().ref_set_camera_parameters(self._h, fov_deg, focal, aperture)

    def resize(self, width, height):
        lib().ref_resize(self._h, int(width), int(height))

    @property
    def render(self):
        W, H = self.size
        out = np.zeros((H, W, 4), np.float32)
        lib().ref_read_render(self._h, _fp(out))
        return out

    @property
    def counts(self):
        W, H = self.size
        out = np.zeros((H, W), np.uint32)
        lib().ref_read_counts(self._h, _up(out))
        return out

    @property
    def image(self):
        W, H = self.size
        out = np.zeros((H, W), np.uint32)
        lib().ref_read_image(self._h, _up(out))
        return out

    @property
    def rng(self):
        W, H = self.size
        out = np.zeros((H, W, 6), np.uint32)
        lib().ref_read_states(self._h, _up(out))
        return out

    def get_ray(self, pixels, states):
        """ThinLensCamera::GetRay for pixels (n, 2) with states (n, 6): (rays (n, 6), the advanced states)."""
        pix = np.ascontiguousarray(pixels, np.uint32).reshape(-1, 2)
        st = np.ascontiguousarray(states, np.uint32).reshape(-1, 6).copy()
        rays = np.zeros((pix.shape[0], 6), np.float32)
        lib().ref_get_ray(self._h, pix.shape[0], _up(pix), _up(st), _fp(rays))
        return rays, st
