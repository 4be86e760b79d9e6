"""CPU-side checks of the product boundary: the C-ABI library loads, exports every symbol
include/rt_mi355x.h declares, and fails loudly (no fallback) when no HIP device exists.
No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", txt)) - {"rt_callback_fn"})


def test_library_loads_and_exports_every_declared_symbol():
    from raytracertest_amd import api
    lib = api.load_library()
    decl = declared_symbols()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(lib, name), "missing export " + name
    assert sorted(api.ABI_SYMBOLS) == decl, "api.ABI_SYMBOLS out of sync with the header"
    assert b"gfx950" in lib.rt_version()


def test_gfx950_code_object_is_embedded():
    from raytracertest_amd import api
    blob = open(api.library_path(), "rb").read()
    assert b"gfx950" in blob and b"trace_kernel" in blob


def test_no_cpu_fallback_without_device():
    import raytracertest_amd as R
    if R.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(R.RtError, match="no HIP device|no CPU fallback"):
        R.RayTracer((8, 8), seed=1)


def test_a_tracer_of_more_pixels_than_rng_init_can_index_is_refused_before_any_device_is_asked():
    """More than 2^32 - 2^19 pixels in ONE tracer: rng_init_kernel's 32-bit chunk loop would wrap (csrc/rt_kernels.hpp).  The
    refusal is an argument check: RT_ERR_INVALID, with or without a device, before anything is allocated.  The same frame is
    accepted in row bands -- that half needs a device: tests/test_gpu_rng_index.py creates its last rows."""
    import numpy as np
    import raytracertest_amd as R
    from raytracertest_amd import api
    limit = 2**32 - 2**19
    assert 65535 * 65537 == 2**32 - 1 > limit                            # a frame create_states used to accept whole
    with pytest.raises(R.RtError, match=r"at most 2\^32 - 2\^19 = %d pixels.*row bands" % limit):
        R.RayTracer((65535, 65537), seed=1)
    lib = api.load_library()
    for size, full_height, row_begin in (((65535, 65537), 0, 0), ((65535, 65536), 65537, 1), ((65535, 65530), 65537, 0)):
        opt = api.Options(struct_size=ctypes.sizeof(api.Options), full_height=full_height, row_begin=row_begin, seed=1)
        handle = ctypes.c_void_p()
        s, pos, ang = np.array(size, np.uint32), np.zeros(3, np.float32), np.zeros(2, np.float32)
        as_p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
        rc = lib.rt_tracer_create_ex(as_p(s, ctypes.c_uint32), as_p(pos, ctypes.c_float), as_p(ang, ctypes.c_float), 70.0, 3.0, 0.05,
                                     ctypes.byref(opt), ctypes.byref(handle))
        assert rc == 1 and not handle, (size, rc)                        # RT_ERR_INVALID
        assert b"at most 2^32 - 2^19" in lib.rt_last_error()
    # a frame above 2^32 - 1 pixels stays refused, band or not (the pixel index is a 32-bit word)
    with pytest.raises(R.RtError, match=r"\(1\).*frames above 2\^32 - 1 pixels"):
        R.RayTracer((65536, 8), seed=1, full_height=65536, row_begin=0)


def test_options_struct_layout_matches_header():
    from raytracertest_amd import api
    assert ctypes.sizeof(api.Options) == 56                  # (48 up to round 2: `transport` was appended; struct_size versions it)
    assert api.Options.seed.offset == 24 and api.Options.flags.offset == 32 and api.Options.transport.offset == 48


def test_product_does_not_touch_the_oracle():
    """The oracle is test infrastructure: nothing under raytracertest_amd/ or include/ may
    import, include or link it."""
    bad = []
    for base in ("raytracertest_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", "Makefile")):
                    txt = open(os.path.join(dirpath, f), errors="ignore").read()
                    if re.search(r"oracle", txt, re.I):
                        bad.append(os.path.join(dirpath, f))
    assert bad == []


def test_header_is_plain_c99(tmp_path):
    """The boundary must be bindable from C: include/rt_mi355x.h compiles as pedantic C99."""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include "rt_mi355x.h"\nint main(void) { rt_options o; o.struct_size = sizeof o; '
                   'return rt_device_count() < 0 ? (int)o.struct_size : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "abi.o")], check=True)
