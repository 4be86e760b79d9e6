#!/usr/bin/env python3
"""Records what the COMPILED REFERENCE computes (oracle/_ref/libref.so: the reference's own kernel headers built for the
CPU, oracle/ref_driver.cpp) on the cases and probes of tests/reference_cases.py:

    python -c "import __graft_entry__ as g; g.build()"      # builds oracle/_ref/libref.so where the reference is checked out
    python tests/golden/make_reference_golden.py

It needs the library and refuses to run without it; the oracle takes no part in what is written, except as the supplier
of orc_sincos, which is installed behind glm::sin / cos / tan for the records called "built_in" (the
transcendentals are the build-owned piece of `strict`).  The cases marked libm are recorded with libm behind them as well.

Outputs (data written by the compiled reference while it runs):
  reference_frames.json   per case and trig: CRC32 and a BLAKE2b digest of the render buffer, the sample counts and the RNG
                          states in full, of the image on the pixels whose three accumulators are all >= 0 and of that mask;
                          the mask's share of the frame; the CRC32 of the scene rows the case was run on
  reference_crops.npz     16 x 16 pixel crops of the render buffers (bit patterns); the whole libm render buffer of
                          reference_cases.LIBM_FULL
  reference_probes.npz    rt::HitTriangle on reference_cases.hit_probes(): hit, t, u, v; ThinLensCamera::GetRay on
                          reference_cases.ray_probes(): rays and advanced states; CRC32s of the probes' inputs
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import oracle_py as orc     # noqa: E402
from oracle import ref_py as ref        # noqa: E402
import reference_cases as rc            # noqa: E402

TRIGS = {"built_in": "oracle", "libm": "libm"}


def frames():
    meta, crops = {}, {}
    for c in rc.CASES:
        for trig in ("built_in", "libm") if c["libm"] else ("built_in",):
            ref.set_trig(TRIGS[trig])
            render, counts, rng, image = rc.play(rc.RefRun(ref, c), c)
            key = "%s/%s" % (c["name"], trig)
            meta[key] = rc.record_of(render, counts, rng, image)
            meta[key]["scene_crc32"] = rc.crc(rc.scene(c["scene"]))
            crops[key.replace("/", "__")] = rc.crop_of(render)[0]
            if trig == "libm" and c["name"] == rc.LIBM_FULL:
                crops["full__" + key.replace("/", "__")] = render.view(np.uint32).copy()
            print("%-48s render %08x  image mask %.4f of the frame (the case asks for >= %.2f)"
                  % (key, meta[key]["render_crc32"], meta[key]["mask_share"], c["min_share"]), flush=True)
    ref.set_trig("libm")
    return meta, crops


def probes():
    out = {}
    rays, tris, group = rc.hit_probes()
    for trig in ("built_in",):                     # HitTriangle calls no transcendental
        ref.set_trig(TRIGS[trig])
        hit, t, u, v = ref.hit_triangle(rays, tris)
    out["hit"] = hit.astype(np.uint8)
    out["tuv"] = np.stack([t, u, v], axis=1).view(np.uint32)
    out["hit_inputs_crc32"] = np.array([rc.crc(rays), rc.crc(tris)], np.uint32)
    for g in sorted(set(group)):
        sel = group == g
        print("HitTriangle %-9s %4d probes, %4d hits" % (g, int(sel.sum()), int(hit[sel].sum())), flush=True)
    ref.set_trig("oracle")
    for k, ((pix, states), (size, angles, fov, focal, aperture)) in enumerate(zip(rc.ray_probes(orc), rc.RAY_CAMERAS)):
        r = ref.RefTracer(size[0], size[1], angles, fov, focal, aperture, seed=1)
        got, st = r.get_ray(pix, states)
        out["rays%d" % k] = got.view(np.uint32)
        out["states%d" % k] = st
        out["ray_inputs_crc32_%d" % k] = np.array([rc.crc(pix), rc.crc(states)], np.uint32)
    ref.set_trig("libm")
    return out


def main():
    if not ref.available():
        sys.exit("oracle/_ref/libref.so is missing: run __graft_entry__.build() where the reference is checked out")
    meta, crops = frames()
    stamp = open(ref.STAMP).read().splitlines()          # compiler, flags and the SHA-256 of the reference files read
    meta["_stamp"] = stamp[:next(i for i, line in enumerate(stamp) if line.startswith("built from"))]
    json.dump(meta, open(os.path.join(HERE, "reference_frames.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "reference_crops.npz"), **crops)
    np.savez_compressed(os.path.join(HERE, "reference_probes.npz"), **probes())
    for f in ("reference_frames.json", "reference_crops.npz", "reference_probes.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
