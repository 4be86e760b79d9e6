#!/usr/bin/env python3
"""How far inside its allowance the query BVH's box test runs: the device comparison of
tests/test_gpu_query_accel.py -- scan against BVH on the same tracer, three ray populations of 2^18 rays and the pinhole rays
of a 512x288 frame, on C4's scene and on 200 000 random triangles -- repeated with the inflation rho multiplied by
slack_milli / 1000 = 1, 0.3, 0.1, 0.03, 0.01 and 0 (rt_dbg_query_accel_slack).  Reports per slack how many rays with a
well-conditioned scan winner get another answer, the largest slack at which one does, and the ratio allowance / reach.
At slack 0 the boxes are bare: differences there are expected (wrong answers, not faults).
Usage: bvh_margin.py [--out FILE.json] [--rays LOG2]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLACKS = (1000, 300, 100, 30, 10, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rays", type=int, default=18)
    a = ap.parse_args()
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    from query_accel_expect import WELL_CONDITIONED, conditioning, populations

    W, H = 512, 288
    xs, ys = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
    pix = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], 1))
    res = {"version": R.api.load_library().rt_version().decode(), "rho": 2.0 ** -8, "slacks": list(SLACKS), "scenes": {}}
    first_fail = 0
    for name, rows in (("c4_10k", scenes.random_triangles(10000, 12345)), ("random_200k", scenes.random_triangles(200000, 77))):
        g = R.RayTracer((W, H), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
        assert g.UploadScene(rows)
        pops = populations(rows, 1 << a.rays, seed=21)
        _, pops["pinhole"] = g.Pick(pix, return_rays=True)
        scan = {k: g.Intersect(r) for k, r in pops.items()}
        ratio = {k: conditioning(r, rows, scan[k]["prim"]) for k, r in pops.items()}
        g.SetQueryAcceleration(True)
        out = {}
        for slack in SLACKS:
            g.DebugQueryAccelSlack(slack)
            per = {}
            for k, r in pops.items():
                got = g.Intersect(r)
                differ = (got.view(np.uint32).reshape(-1, 4) != scan[k].view(np.uint32).reshape(-1, 4)).any(axis=1)
                well = differ & ~(ratio[k] < WELL_CONDITIONED)
                per[k] = {"rays": int(r.shape[0]), "differ": int(differ.sum()), "differ_well_conditioned": int(well.sum())}
                if well.any():
                    first_fail = max(first_fail, slack)
            out[str(slack)] = per
        out["smallest_winner_ratio"] = {k: float(np.min(v[np.isfinite(v)], initial=np.inf)) for k, v in ratio.items()}
        res["scenes"][name] = out
        g.close()
    res["largest_slack_milli_with_a_well_conditioned_difference"] = first_fail
    res["allowance_over_reach"] = (">= %g (no difference above slack 0)" % (1000.0 / SLACKS[-2])) if first_fail == 0 else 1000.0 / first_fail
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
