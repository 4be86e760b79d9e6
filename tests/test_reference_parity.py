"""The strict oracle against the reference's own kernels, on the CPU.

tests/golden/reference_*.json / .npz hold what the COMPILED reference computed (oracle/_ref/libref.so, the reference's
RayTracer/Kernels.cuh built for the CPU behind oracle/ref_driver.cpp; recorded by tests/golden/make_reference_golden.py) on
the cases and probes of tests/reference_cases.py.  Here:
  - the strict oracle reproduces every record: render buffer, sample counts and RNG states bit for bit, the image on the
    pixels where the reference defines it (reference_cases' docstring), HitTriangle and GetRay on the probes;
  - where the library is there, a fresh run of it reproduces the records too (skipped, with the reason, where it is not);
  - teeth: the fma oracle, the nearest-hit rule, another scan order of the twins and libm's sin / cos each miss a record;
  - libm's sin / cos against the build-owned sincos: same RNG states, render buffers within the project's cross-mode bound."""
import json
import os

import numpy as np
import pytest

import reference_cases as rc
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "reference_frames.json")) as _f:
    FRAMES = json.load(_f)
CROPS = np.load(os.path.join(GOLDEN, "reference_crops.npz"))
PROBES = np.load(os.path.join(GOLDEN, "reference_probes.npz"))
NAMES = [c["name"] for c in rc.CASES]
LIBM_NAMES = [c["name"] for c in rc.CASES if c["libm"]]
TOLERANCE = 2e-6          # per sample and channel: tests/test_gpu_parity.py: test_mode_tolerance, DESIGN.md section 2


def rec(name, trig="built_in"):
    key = "%s/%s" % (name, trig)
    return FRAMES[key], CROPS[key.replace("/", "__")]


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_py
    if not ref_py.available():
        pytest.skip("oracle/_ref/libref.so is not built: no reference checkout was found when build() ran")
    yield ref_py
    ref_py.set_trig("libm")


_ORACLE = {}


def oracle_buffers(orc, name):
    """the strict oracle's four buffers of a case, computed once and shared (read-only)"""
    if name not in _ORACLE:
        c = rc.case(name)
        _ORACLE[name] = tuple(np.array(b) for b in rc.play(rc.OracleRun(orc, c), c))
        for b in _ORACLE[name]:
            b.setflags(write=False)
    return _ORACLE[name]


# ---------------------------------------------------------------------------------------------------------------- the table
def test_case_table_covers_what_it_is_there_for():
    sizes = {(c["W"], c["H"]) for c in rc.CASES}
    assert sizes == {(40, 24), (96, 54), (236, 134)}
    assert {c["scene"] for c in rc.CASES} == {"cornell", "five", "adversarial37", "twins", "five_degenerate"}
    angles = {c["angles"] for c in rc.CASES}
    assert {(0.0, 0.0), (0.1, -0.05), (0.1, 3.0)} <= angles
    assert any(c["aperture"] == 0.0 for c in rc.CASES) and {40.0, 112.0} <= {c["fov"] for c in rc.CASES}
    spp = {op[2] for c in rc.CASES for op in c["seq"] if op[0] == "trace"}
    assert {1, 3, 7} <= spp
    kinds = [tuple(op[0] for op in c["seq"]) for c in rc.CASES]
    assert ("trace",) in kinds and ("trace", "trace") in kinds and ("trace", "rotate", "params", "trace") in kinds
    resized = [rc.final_size(c) for c in rc.CASES if any(op[0] == "resize" for op in c["seq"])]
    assert resized and all(W % 8 and H % 8 for W, H in resized)
    assert len(LIBM_NAMES) >= 3 and rc.LIBM_FULL in LIBM_NAMES
    assert set(FRAMES) - {"_stamp"} == {"%s/built_in" % n for n in NAMES} | {"%s/libm" % n for n in LIBM_NAMES}


def test_scenes_are_what_the_cases_are_named_after():
    for c in rc.CASES:                                            # the records belong to these very rows
        assert rc.crc(rc.scene(c["scene"])) == rec(c["name"])[0]["scene_crc32"], c["scene"]
    t = rc.scene("twins").reshape(-1, 3, 4)[:, :, :3]
    assert np.array_equal(t[0], t[1]) and np.array_equal(t[3], t[0][[0, 2, 1]])
    assert np.array_equal(t[2][1] - t[2][0], 3 * (t[0][1] - t[0][0])) and np.array_equal(t[2][2] - t[2][0], 3 * (t[0][2] - t[0][0]))
    d = rc.scene("five_degenerate").reshape(-1, 3, 4)[5:, :, :3].astype(np.float64)
    assert d.shape[0] == 4 and np.allclose(np.cross(d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]), 0.0, atol=1e-7)


def test_image_mask_is_a_condition_not_a_loophole():
    """Every case compares at least its min_share of the image, by the reference's own render buffer; two cases at least compare
    every pixel; and the mask leaves out nothing but pixels with a negative accumulator."""
    whole = 0
    for c in rc.CASES:
        for trig in ("built_in", "libm") if c["libm"] else ("built_in",):
            share = rec(c["name"], trig)[0]["mask_share"]
            assert share >= c["min_share"], (c["name"], trig, share)
        whole += rec(c["name"])[0]["mask_share"] == 1.0 and c["min_share"] == 1.0
    assert whole >= 2
    r = np.zeros((2, 3, 4), np.float32)
    r[0, 1, 2] = -1e-30
    r[1, 2, 0] = np.nan
    r[1, 0, 3] = -5.0                                             # alpha is never written and takes no part
    assert rc.image_mask(r).tolist() == [[True, False, True], [True, True, False]]


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", NAMES)
def test_strict_oracle_equals_the_recorded_reference(orc, name):
    c = rc.case(name)
    render, counts, rng, image = oracle_buffers(orc, name)
    r, crop = rec(name)
    assert rc.differences(r, crop, render, counts, rng, image) == []
    assert (counts == rc.samples_of(c)).all() and render.shape[:2][::-1] == rc.final_size(c)
    assert float(rc.image_mask(render).mean()) >= c["min_share"]


@pytest.mark.parametrize("name", NAMES)
def test_fresh_reference_equals_the_fixtures(ref, name):
    c = rc.case(name)
    for trig in ("built_in", "libm") if c["libm"] else ("built_in",):
        ref.set_trig({"built_in": "oracle", "libm": "libm"}[trig])
        r, crop = rec(name, trig)
        assert rc.differences(r, crop, *rc.play(rc.RefRun(ref, c), c)) == [], trig


def test_fresh_reference_is_built_from_the_recorded_files(ref):
    """the SHA-256 of the reference files the library was compiled from are the ones the records were made from"""
    stamp = open(ref.STAMP).read().splitlines()
    head = stamp[:next(i for i, line in enumerate(stamp) if line.startswith("built from"))]
    sums = lambda lines: [line.split() for line in lines if len(line.split()) == 2 and len(line.split()[0]) == 64]
    assert len(sums(head)) == 8 and sums(head) == sums(FRAMES["_stamp"])
    assert any("-ffp-contract=off" in line and "-fno-fast-math" in line for line in stamp)


def test_oracle_hit_triangle_equals_the_recorded_probes(orc):
    rays, tris, group = rc.hit_probes()
    assert [rc.crc(rays), rc.crc(tris)] == PROBES["hit_inputs_crc32"].tolist(), "the probes are not the recorded ones"
    hit, tuv = PROBES["hit"].astype(bool), PROBES["tuv"].view(np.float32)
    got_hit = np.zeros(len(rays), bool)
    got = np.zeros((len(rays), 3), np.float32)
    for i in range(len(rays)):
        ray = orc.ray_make(rays[i, :3], rays[i, 3:], True, orc.STRICT)
        got_hit[i], got[i, 0], got[i, 1], got[i, 2] = orc.hit_triangle(ray, tris[i, 0:3], tris[i, 3:6], tris[i, 6:9], orc.STRICT, 0)
    assert np.array_equal(got_hit, hit), np.flatnonzero(got_hit != hit)[:8]
    bad = np.flatnonzero(~rc.same_bits(got, tuv).all(axis=1) & hit)
    assert bad.size == 0, (bad[:8], got[bad[:2]], tuv[bad[:2]])


def test_hit_probes_sit_on_the_edges_they_are_named_after():
    """By the REFERENCE's recorded answers: det on both sides of the culling epsilon, u, v and u + v at 0 and 1 exactly, hits and
    misses among the denormal and the 2^60-sized triangles, and an overflowing t."""
    rays, tris, group = rc.hit_probes()
    hit, tuv = PROBES["hit"].astype(bool), PROBES["tuv"].view(np.float32)
    for g in ("det", "tilt", "tiny", "huge", "exact_uv", "aimed", "queries"):
        sel = group == g
        assert hit[sel].any() and not hit[sel].all(), g
    det = np.flatnonzero(group == "det")                  # a ladder of scales: the hits are exactly its upper end
    first = det[:13]
    assert not hit[first[0]] and hit[first[-1]] and (np.diff(hit[first].astype(int)) >= 0).all()
    u, v = tuv[(group == "exact_uv") & hit, 1], tuv[(group == "exact_uv") & hit, 2]
    assert (u == 0).any() and (u == 1).any() and (v == 0).any() and (v == 1).any() and ((u + v == 1) & (u > 0) & (v > 0)).any()
    assert (np.abs(tris[group == "tiny"]).max(axis=1) < 1.2e-38).all() and (np.abs(tris[group == "huge"]).max(axis=1) >= 2.0 ** 60).all()
    assert np.isinf(tuv[(group == "huge") & hit, 0]).any()


def test_oracle_get_ray_equals_the_recorded_probes(orc):
    import ctypes as C
    L = orc.lib()
    for k, ((pix, states), (size, angles, fov, focal, aperture)) in enumerate(zip(rc.ray_probes(orc), rc.RAY_CAMERAS)):
        assert [rc.crc(pix), rc.crc(states)] == PROBES["ray_inputs_crc32_%d" % k].tolist(), "the probes are not the recorded ones"
        want, want_states = PROBES["rays%d" % k], PROBES["states%d" % k]
        cam = orc.camera(angles, fov, focal, aperture)
        for i in range(pix.shape[0]):
            s, out = states[i].copy(), np.zeros(6, np.float32)
            L.orc_camera_get_ray(C.byref(cam), int(pix[i, 0]), int(pix[i, 1]), size[0], size[1], orc._up(s), orc.STRICT, orc._fp(out))
            assert np.array_equal(out.view(np.uint32), want[i]), (k, i, out, want[i].view(np.float32))
            assert np.array_equal(s, want_states[i]) and not np.array_equal(s, states[i]), (k, i)


def test_fresh_reference_equals_the_recorded_probes(ref):
    from oracle import oracle_py as orc
    rays, tris, _ = rc.hit_probes()
    hit, t, u, v = ref.hit_triangle(rays, tris)
    assert np.array_equal(hit, PROBES["hit"].astype(bool))
    assert np.array_equal(np.stack([t, u, v], axis=1).view(np.uint32), PROBES["tuv"])
    ref.set_trig("oracle")
    for k, ((pix, states), (size, angles, fov, focal, aperture)) in enumerate(zip(rc.ray_probes(orc), rc.RAY_CAMERAS)):
        got, st = ref.RefTracer(size[0], size[1], angles, fov, focal, aperture, seed=1).get_ray(pix, states)
        assert np.array_equal(got.view(np.uint32), PROBES["rays%d" % k]) and np.array_equal(st, PROBES["states%d" % k])


# ---------------------------------------------------------------------------------------------------------------- teeth
def test_teeth_fma_oracle_misses_the_record(orc):
    for name in ("c40_cornell_turned", "c236_cornell_spp7"):
        c = rc.case(name)
        bad = rc.differences(*rec(name), *rc.play(rc.OracleRun(orc, c, contract=orc.FMA), c))
        assert "render" in bad and "rng" not in bad and "counts" not in bad, (name, bad)


def test_teeth_nearest_hit_misses_the_record_on_the_twins(orc):
    c = rc.case("c96_twins_aperture0")
    bad = rc.differences(*rec(c["name"]), *rc.play(rc.OracleRun(orc, c, hit_mode=1), c))
    assert "render" in bad and "image_on_mask" in bad and "rng" not in bad, bad


def test_teeth_the_tie_between_the_twins_decides_bits(orc):
    """`distance < t` keeps the first of two triangles with the same t (Kernels.cuh:84).  The tripled twin ties with the plane's
    triangle on some rays and has another normal in the last bit: scanned before it, it changes those pixels and no others."""
    for name in ("c96_twins_aperture0", "c236_twins_lens"):
        c = rc.case(name)
        rows = rc.scene("twins").reshape(-1, 3, 4)
        swapped = np.ascontiguousarray(rows[[2, 1, 0, 3, 4]].reshape(-1, 4))
        render, counts, rng, image = rc.play(rc.OracleRun(orc, c, scene_rows=swapped), c)
        base = oracle_buffers(orc, name)
        changed = (render.view(np.uint32) != base[0].view(np.uint32)).any(axis=2)
        assert "render" in rc.differences(*rec(name), render, counts, rng, image), name
        assert 0.02 < changed.mean() < 0.98, (name, changed.mean())            # ties on some rays, an ulp apart on others
        assert np.abs(render - base[0]).max() <= 4e-7 * rc.samples_of(c)        # and nothing but last bits
        assert np.array_equal(rng, base[2])


def test_teeth_libm_record_differs_in_the_render_buffer_only():
    for name in LIBM_NAMES:
        a, b = rec(name, "built_in")[0], rec(name, "libm")[0]
        assert a["rng_crc32"] == b["rng_crc32"] and a["rng_digest"] == b["rng_digest"] and a["counts_crc32"] == b["counts_crc32"], name
    turned = [n for n in LIBM_NAMES if rc.case(n)["angles"] != (0.0, 0.0) or any(op[0] == "rotate" for op in rc.case(n)["seq"])]
    assert len(turned) >= 2
    for name in turned:
        assert rec(name, "built_in")[0]["render_crc32"] != rec(name, "libm")[0]["render_crc32"], name


# ---------------------------------------------------------------------------------------------------------------- libm
def _cross_trig(name, a, b):
    """|a - b| of two render buffers of a case against the cross-mode bound; returns (max |a - b|, share within the bound)"""
    n = rc.samples_of(rc.case(name))
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)).max(axis=2)
    return float(d.max()), float((d <= TOLERANCE * n).mean())


def test_libm_trig_stays_within_the_cross_mode_bound_recorded_frame(orc):
    """The reference with libm's sinf / cosf / tanf behind glm against the build-owned sincos (= the strict oracle, by the test
    above), on the frame whose libm render buffer is recorded in full: |a - b| <= 2e-6 * samples per channel on >= 99.5 % of
    the pixels.  Measured: max |a - b| = 2.4e-7 at 6 samples, every pixel within the bound."""
    name = rc.LIBM_FULL
    libm = CROPS["full__%s__libm" % name].view(np.float32)
    assert rc.crc(libm) == rec(name, "libm")[0]["render_crc32"]
    worst, share = _cross_trig(name, libm, oracle_buffers(orc, name)[0])
    print("libm against the build-owned sincos, %s: max |a - b| = %.3g at %d samples, %.4f of the pixels within %.1e per sample"
          % (name, worst, rc.samples_of(rc.case(name)), share, TOLERANCE))
    assert 0.0 < worst and share >= 0.995


@pytest.mark.parametrize("name", LIBM_NAMES)
def test_libm_trig_stays_within_the_cross_mode_bound(ref, orc, name):
    c = rc.case(name)
    ref.set_trig("libm")
    render, counts, rng, image = rc.play(rc.RefRun(ref, c), c)
    base = oracle_buffers(orc, name)
    assert np.array_equal(rng, base[2]) and np.array_equal(counts, base[1])
    worst, share = _cross_trig(name, render, base[0])
    print("libm against the build-owned sincos, %s: max |a - b| = %.3g at %d samples, %.4f of the pixels within %.1e per sample"
          % (name, worst, rc.samples_of(c), share, TOLERANCE))
    assert share >= 0.995
