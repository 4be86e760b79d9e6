#!/usr/bin/env python3
"""How far inside its allowance the query BVH's box test runs: the device comparison of
tests/test_gpu_query_accel.py -- scan against BVH on the same tracer, three ray populations of 2^18 rays and the pinhole rays
of a 512x288 frame, on C4's scene and on 200 000 random triangles -- repeated with the inflation rho multiplied by
slack_milli / 1000 = 1, 0.3, 0.1, 0.03, 0.01 and 0 (rt_dbg_query_accel_slack).  Reports per slack how many rays with a
well-conditioned scan winner get another answer, the largest slack at which one does, and the ratio allowance / reach.
At slack 0 the boxes are bare: differences there are expected (wrong answers, not faults).
--closest: the same sweep for the point query, whose allowance rho_c the same slack scales: ClosestPoint, scan
against BVH, on 2^LOG2 points of tests/closest_expect.points_for and on the lattice points, C4's scene and the lattice scene;
there is no conditioning clause, so every differing row counts.  Reports the smallest slack at which BVH still equals scan.
--nearest: the --closest sweep for the k-nearest query, which prunes with the same allowance against the
list's last entry: ClosestAll with max_hits 4 and 16, rows and counts, scan against BVH, same points and scenes.
--spherecast: the same sweep for the swept query, whose allowance beyond r (4 * RT_SWEEP_SLACK * (cmax + r) +
rho_s * (max|o| + cmax + r)) the same slack scales: SphereCast, scan against BVH, on 2^LOG2 sweeps of
tests/spherecast_expect.random_sweeps (narrow and wide radii, a share cut at tmax) on C4's scene and the lattice scene.
--tridistance: the --closest sweep for the triangle distance query, which prunes with the point query's allowance
rho_c against the query triangle's bounding box: TriangleDistance, hits and witnesses, scan against BVH, on 2^LOG2 queries of
tests/tridistance_expect.mixed_queries (and the lattice's tie queries), unbounded and within the median distance, C4's scene and
the lattice scene.
--graze: the sweep on the grazing populations of tests/graze_cases.py (`above` on the general, flat and sliver scenes of 2 000
triangles, `rivals` on the pairs), whose targeted hits sit at a conditioning of 2^-10 .. 2^-6: Intersect under both hit rules,
Occluded, IntersectAll (max_hits 4) and Exposure with a world-space table, scan against BVH on the same tracer, with two more
slacks (0.003, 0.001: rt_dbg_query_accel_slack counts in thousandths).  Per query and
slack the rows that differ and, of them, the rows the contract does not let differ: the scan winner is well conditioned
(Intersect, also by distance class), or a well-conditioned in-interval hit of the scan's own first 16 was lost (the others).
Usage: bvh_margin.py [--closest | --nearest | --spherecast | --tridistance | --graze] [--out FILE.json] [--rays LOG2]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLACKS = (1000, 300, 100, 30, 10, 0)
GRAZE_SLACKS = (1000, 300, 100, 30, 10, 3, 1, 0)        # --graze goes on to the smallest non-zero slack there is


def closest_margin(R, scenes, log2_points):
    import closest_expect as ce
    import lattice_cases as lc
    res = {"version": R.api.load_library().rt_version().decode(), "rho_c": 2.0 ** -18, "derived_budget": 19 * 2.0 ** -24,
           "slacks": list(SLACKS), "scenes": {}}
    smallest_equal = {}
    for name, rows in (("c4_10k", scenes.random_triangles(10000, 12345)), ("lattice_rooms", lc.rooms())):
        g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
        assert g.UploadScene(rows)
        pts = ce.points_for(rows, 1 << log2_points, seed=81, spread=4.0)
        if name == "lattice_rooms":
            pts = np.concatenate([ce.lattice_points(), pts])
        scan = g.ClosestPoint(pts)
        batches = {"unbounded": ce.with_radius(pts, np.inf), "half": ce.with_radius(pts, np.float32(np.median(scan["t"])))}
        scan = {k: g.ClosestPoint(p) for k, p in batches.items()}
        g.SetQueryAcceleration(True)
        out, equal = {}, []
        for slack in SLACKS:
            g.DebugQueryAccelSlack(slack)
            per = {}
            for k, p in batches.items():
                got = g.ClosestPoint(p)
                differ = (got.view(np.uint32).reshape(-1, 4) != scan[k].view(np.uint32).reshape(-1, 4)).any(axis=1)
                per[k] = {"points": int(p.shape[0]), "differ": int(differ.sum())}
            out[str(slack)] = per
            if all(v["differ"] == 0 for v in per.values()):
                equal.append(slack)
        smallest_equal[name] = min(equal) if equal else None
        res["scenes"][name] = out
        g.close()
    res["smallest_slack_milli_at_which_bvh_equals_scan"] = smallest_equal
    return res


def nearest_margin(R, scenes, log2_points):
    import closest_expect as ce
    import lattice_cases as lc
    res = {"version": R.api.load_library().rt_version().decode(), "rho_c": 2.0 ** -18, "derived_budget": 19 * 2.0 ** -24,
           "slacks": list(SLACKS), "max_hits": [4, 16], "scenes": {}}
    smallest_equal = {}
    for name, rows in (("c4_10k", scenes.random_triangles(10000, 12345)), ("lattice_rooms", lc.rooms())):
        g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
        assert g.UploadScene(rows)
        pts = ce.points_for(rows, 1 << log2_points, seed=81, spread=4.0)
        if name == "lattice_rooms":
            pts = np.concatenate([ce.lattice_points(), pts])
        median = np.float32(np.median(g.ClosestPoint(pts)["t"]))
        batches = {"unbounded": ce.with_radius(pts, np.inf), "median": ce.with_radius(pts, median)}
        scan = {(k, m): g.ClosestAll(p, m) for k, p in batches.items() for m in (4, 16)}
        g.SetQueryAcceleration(True)
        out, equal = {}, []
        for slack in SLACKS:
            g.DebugQueryAccelSlack(slack)
            per = {}
            for (k, m), (hits, counts) in scan.items():
                got, got_counts = g.ClosestAll(batches[k], m)
                differ = (got.view(np.uint32).reshape(-1, 4 * m) != hits.view(np.uint32).reshape(-1, 4 * m)).any(axis=1)
                per["%s_%d" % (k, m)] = {"points": int(hits.shape[0]), "rows_differ": int(differ.sum()),
                                         "counts_differ": int((got_counts != counts).sum())}
            out[str(slack)] = per
            if all(v["rows_differ"] == 0 and v["counts_differ"] == 0 for v in per.values()):
                equal.append(slack)
        smallest_equal[name] = min(equal) if equal else None
        res["scenes"][name] = out
        g.close()
    res["smallest_slack_milli_at_which_bvh_equals_scan"] = smallest_equal
    return res


def tridistance_margin(R, scenes, log2_queries):
    import lattice_cases as lc
    import tridistance_expect as td
    res = {"version": R.api.load_library().rt_version().decode(), "rho_c": 2.0 ** -18, "slacks": list(SLACKS), "scenes": {}}
    smallest_equal = {}
    for name, rows in (("c4_10k", scenes.random_triangles(10000, 12345)), ("lattice_rooms", lc.rooms())):
        g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
        assert g.UploadScene(rows)
        q = td.mixed_queries(rows, 1 << log2_queries, 85)
        if name == "lattice_rooms":
            q = np.concatenate([td.lattice_queries(), q])
        first = g.TriangleDistance(q)[0]
        median = np.float32(np.median(first["t"][first["prim"] >= 0]))
        batches = {"unbounded": q, "median": td.with_radius(q, median)}
        scan = {k: g.TriangleDistance(b) for k, b in batches.items()}
        g.SetQueryAcceleration(True)
        out, equal = {}, []
        for slack in SLACKS:
            g.DebugQueryAccelSlack(slack)
            per = {}
            for k, b in batches.items():
                differ = td.differing(g.TriangleDistance(b), scan[k])
                per[k] = {"queries": int(b.shape[0]), "answers": int((scan[k][0]["prim"] >= 0).sum()), "differ": int(differ.size)}
            out[str(slack)] = per
            if all(v["differ"] == 0 for v in per.values()):
                equal.append(slack)
        smallest_equal[name] = min(equal) if equal else None
        res["scenes"][name] = out
        g.DebugQueryAccelSlack(1000)
        g.close()
    res["smallest_slack_milli_at_which_bvh_equals_scan"] = smallest_equal
    return res


def spherecast_margin(R, scenes, log2_sweeps):
    import lattice_cases as lc
    import spherecast_expect as se
    res = {"version": R.api.load_library().rt_version().decode(), "sweep_slack": float(se.SLACK), "rho_s": float(se.RHO_S),
           "slacks": list(SLACKS), "scenes": {}}
    smallest_equal = {}
    n = 1 << log2_sweeps
    for name, rows in (("c4_10k", scenes.random_triangles(10000, 12345)), ("lattice_rooms", lc.rooms())):
        g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1)
        assert g.UploadScene(rows)
        wide = se.random_sweeps(rows, n, 83, rmin=-1.0, rmax=0.5)
        wide[::3, 7] = 0.5
        batches = {"narrow": se.random_sweeps(rows, n, 82), "wide": wide, "far": se.random_sweeps(rows, n, 84, far=100.0)}
        scan = {k: g.SphereCast(b) for k, b in batches.items()}
        g.SetQueryAcceleration(True)
        out, equal = {}, []
        for slack in SLACKS:
            g.DebugQueryAccelSlack(slack)
            per = {}
            for k, b in batches.items():
                got = g.SphereCast(b)
                differ = (got.view(np.uint32).reshape(-1, 4) != scan[k].view(np.uint32).reshape(-1, 4)).any(axis=1)
                per[k] = {"sweeps": int(b.shape[0]), "contacts": int((scan[k]["prim"] >= 0).sum()), "differ": int(differ.sum())}
            out[str(slack)] = per
            if all(v["differ"] == 0 for v in per.values()):
                equal.append(slack)
        smallest_equal[name] = min(equal) if equal else None
        res["scenes"][name] = out
        g.DebugQueryAccelSlack(1000)
        g.close()
    res["smallest_slack_milli_at_which_bvh_equals_scan"] = smallest_equal
    return res


def graze_margin(R, log2_rays):
    import exposure_expect as ee
    import graze_cases as gc
    from query_accel_expect import WELL_CONDITIONED, conditioning
    n = min(1 << log2_rays, 1 << 16) // 81 * 81
    res = {"version": R.api.load_library().rt_version().decode(), "rho": 2.0 ** -8, "slacks": list(GRAZE_SLACKS), "rays": n, "scenes": {}}
    first_fail = {}

    def well_of(scan, segs, rows):
        """(n, k) bool: the entries of the scan's lists that are well-conditioned triangle hits."""
        sh, sc = scan
        k = sh.shape[1]
        ratio = np.stack([conditioning(segs[:, :6], rows, sh["prim"][:, j]) for j in range(k)], 1)
        return (np.arange(k)[None, :] < sc[:, None]) & (ratio >= WELL_CONDITIONED) & np.isfinite(ratio)

    def lists_lost(scan, got, segs, rows, m):
        """Rows whose tree list lacks a well-conditioned hit of the scan's list that sorts before its end."""
        sh, sc = scan
        gh, gcnt = got
        well = well_of(scan, segs, rows)
        held = (sh["prim"][:, :, None] == gh["prim"][:, None, :m]).any(axis=2)
        last = np.clip(gcnt.astype(np.int64) - 1, 0, None)
        lt, lp = gh["t"][np.arange(len(last)), last], gh["prim"][np.arange(len(last)), last]
        room = (gcnt < m)[:, None] | (sh["t"] < lt[:, None]) | ((sh["t"] == lt[:, None]) & (sh["prim"] < lp[:, None]))
        return (well & ~held & room).any(axis=1)

    for name in ("general", "flat", "slivers", "pairs"):
        if name == "pairs":
            rows, pop = gc.pairs(999)
        else:
            rows = gc.slivers(2000) if name == "slivers" else gc.SCENES[name](2000, size=0.6)
            pop = gc.rays(rows, "above", n, seed=51)
        rays, segs = pop["rays"], gc.segments(pop)
        groups = gc.exposure_groups(pop, 12)
        xsegs = np.concatenate([ee.exposure_segments(p, d, world=True) for p, d in groups])
        out = {str(s): {} for s in GRAZE_SLACKS}
        for nearest in (False, True):
            g = R.RayTracer((64, 48), (0, 0, 0), (0.0, 0.0), 70.0, 3.0, 0.05, seed=1, nearest_hit=nearest)
            assert g.UploadScene(rows)
            scan = g.Intersect(rays)
            well = conditioning(rays, rows, scan["prim"]) >= WELL_CONDITIONED
            if not nearest:
                occ, lists, xocc, xlists = g.Occluded(segs), g.IntersectAll(segs, 16), g.Occluded(xsegs), g.IntersectAll(xsegs, 16)
                lists4 = (np.ascontiguousarray(lists[0][:, :4]), np.minimum(lists[1], 4))
                owell, xwell = well_of(lists, segs, rows).any(axis=1), well_of(xlists, xsegs, rows).any(axis=1)
            g.SetQueryAcceleration(True)
            for slack in GRAZE_SLACKS:
                g.DebugQueryAccelSlack(slack)
                per = out[str(slack)]
                got = g.Intersect(rays)
                differ = (got.view(np.uint32).reshape(-1, 4) != scan.view(np.uint32).reshape(-1, 4)).any(axis=1)
                key = "intersect_nearest" if nearest else "intersect_farthest"
                per[key] = {"rows": int(rays.shape[0]), "differ": int(differ.sum()), "differ_well_conditioned": int((differ & well).sum()),
                            "by_distance_class": [int((differ & well & (pop["L"] == c)).sum()) for c in range(len(gc.L_CLASSES))]}
                if not nearest:
                    o = g.Occluded(segs)
                    per["occluded"] = {"rows": int(segs.shape[0]), "differ": int((o != occ).sum()), "invented": int((o & ~occ).sum()),
                                       "differ_well_conditioned": int((owell & occ & ~o).sum())}
                    a = g.IntersectAll(segs, 4)
                    d4 = (a[0].view(np.uint32).reshape(-1, 16) != lists4[0].view(np.uint32).reshape(-1, 16)).any(axis=1) | (a[1] != lists4[1])
                    per["intersect_all_4"] = {"rows": int(segs.shape[0]), "differ": int(d4.sum()),
                                              "differ_well_conditioned": int(lists_lost(lists4, a, segs, rows, 4).sum())}
                    masks = np.concatenate([g.Exposure(p, d, world=True) for p, d in groups])
                    xo = ~ee.unpack_masks(masks).reshape(-1)
                    per["exposure"] = {"rows": int(xsegs.shape[0]), "differ": int((xo != xocc).sum()), "invented": int((xo & ~xocc).sum()),
                                       "differ_well_conditioned": int((xwell & xocc & ~xo).sum())}
            g.DebugQueryAccelSlack(1000)
            g.close()
        res["scenes"][name] = out
        for slack in GRAZE_SLACKS:
            for q, v in out[str(slack)].items():
                if v["differ_well_conditioned"]:
                    first_fail[q] = max(first_fail.get(q, -1), slack)
    # per query the largest slack at which a row the contract protects differed (absent: at none, not even bare boxes)
    res["largest_slack_milli_with_a_well_conditioned_difference"] = first_fail
    worst = max(first_fail.values(), default=-1)
    clean = min(s for s in GRAZE_SLACKS if s > worst)                     # the smallest probed slack above it: still the scan
    res["smallest_clean_slack_milli"] = clean
    res["allowance_over_reach"] = {"at_least": 1000.0 / clean, "below": (1000.0 / worst) if worst > 0 else None,
                                   "bare_boxes_differ": worst >= 0}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rays", type=int, default=18)
    ap.add_argument("--closest", action="store_true")
    ap.add_argument("--nearest", action="store_true")
    ap.add_argument("--spherecast", action="store_true")
    ap.add_argument("--tridistance", action="store_true")
    ap.add_argument("--graze", action="store_true")
    a = ap.parse_args()
    import raytracertest_amd as R
    from raytracertest_amd import scenes
    if a.graze:
        txt = json.dumps(graze_margin(R, a.rays), indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    if a.closest or a.nearest or a.spherecast or a.tridistance:
        margin = tridistance_margin if a.tridistance else spherecast_margin if a.spherecast else nearest_margin if a.nearest else closest_margin
        txt = json.dumps(margin(R, scenes, a.rays), indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
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
