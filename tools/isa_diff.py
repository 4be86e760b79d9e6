#!/usr/bin/env python3
"""Which kernels' gfx950 ISA changed between two `make -C raytracertest_amd/csrc asm` outputs (labels, comments and the
kernel's own name normalised).  Usage: isa_diff.py [--by-body] old.s new.s
--by-body: compare the multisets of normalised bodies instead of the names, for changes that rename kernels (template
arguments); lists the bodies present on one side only."""
import collections, hashlib, re, sys


def funcs(path):
    t = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", t, re.S | re.M):
        body = re.sub(r"\.LBB\d+_\d+", ".LBB", m.group(2))
        body = re.sub(r"[ \t]*;.*", "", body).replace(m.group(1), "<self>")   # (its own name: .amdhsa_kernel, .section)
        out[m.group(1)] = (hashlib.md5(body.encode()).hexdigest(), body.count("\n"))
    return out


args = [x for x in sys.argv[1:] if x != "--by-body"]
a, b = funcs(args[0]), funcs(args[1])
if "--by-body" in sys.argv:
    ha, hb = collections.Counter(v[0] for v in a.values()), collections.Counter(v[0] for v in b.values())
    for side, mine, other, names in (("old", ha, hb, a), ("new", hb, ha, b)):
        for h in sorted(mine - other):
            print("ONLY", side, (mine - other)[h], [k[:110] for k in sorted(names) if names[k][0] == h])
    print("bodies: %d old, %d new, %d in common" % (sum(ha.values()), sum(hb.values()), sum((ha & hb).values())))
    sys.exit(0 if ha == hb else 1)
same = 0
for k in sorted(a):
    if k not in b:
        print("GONE", k[:110])
    elif a[k][0] == b[k][0]:
        same += 1
    else:
        print("DIFF", k[:110], a[k][1], "->", b[k][1], "lines")
print("same %d, new %d" % (same, len(set(b) - set(a))))
