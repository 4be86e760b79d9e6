#!/usr/bin/env python3
"""The accuracy of rt_tracer_section_segments' endpoints, measured without a device: the residual
|n.X - d| / (|n| max|corner|) in float64 of the fp32 endpoints of tests/section_expect.cuts -- the kernel's arithmetic operation
by operation -- over the families of section_expect.margin_families, against a float64 run of the same rule on the same fp32
inputs (a pair enters when both find the same case).  Writes profiles/section_margin_<kernel hash>.json, the record
tests/test_section_expect.py compares its own measurement with.
Usage: section_margin.py [--out FILE.json]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import section_expect as se                                              # noqa: E402
from raytracertest_amd import api                                        # noqa: E402

version = api.load_library().rt_version().decode()
khash = re.search(r"kernels=([0-9a-f]+)", version).group(1)
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "section_margin_%s.json" % khash)
doc = {"library": version, "unit": "|n.X - d| / (|n| max|corner|), float64", "families": {}}
worst = 0.0
for name, (rows, planes) in se.margin_families().items():
    w, entered, left_out, total = se.margin(rows, planes)
    doc["families"][name] = {"largest_residual": w, "in_ulps_of_1": w * 2.0 ** 24, "entered": entered, "left_out": left_out, "pairs": total}
    worst = max(worst, w)
    print("%-10s %.4e  entered %d, left out %d of %d" % (name, w, entered, left_out, total))
doc["largest_residual"] = worst
doc["cut_slack"] = se.CUT_SLACK
doc["excluded_cap"] = se.EXCLUDED_CAP
assert se.CUT_SLACK / 2 < 4 * worst <= se.CUT_SLACK
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print("largest %.4e, 4 x = %.4e <= 2^%d; wrote %s" % (worst, 4 * worst, round(__import__("math").log2(se.CUT_SLACK)), out))
