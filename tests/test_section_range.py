"""The section query's restatement at scales 2^k, without a device, in the manner of tests/test_range_cases.py: a scene and its
planes multiplied by 2^k -- every length times s, the normal (a difference or a cross product of scene lengths in a caller's hands)
times s, and d0, d1, which are then squared lengths, times s * s -- answer the same rows for k = -61 .. 62 on the lattice with two
spheres, and one step beyond either end a row differs.  Only second powers enter the rule (n.x, and the sphere rule's dot(n, n)):
above, the products and the d reach +inf; below, they run into the subnormals, where the planes one ulp beside a wall collapse
onto it.  The ends are the measured ones."""
import numpy as np
import pytest

import lattice_cases as lc
import section_expect as se
from test_section_expect import lattice_planes

f32 = np.float32
RANGE = (-61, 62)
INSIDE_KS = (-40, -17, -1, 1, 9, 33)
SPHERES = f32([[0.25, -0.5, 0.75, 0.5], [-1.75, -1.75, -1.75, 1.0]])


@pytest.fixture(scope="module", autouse=True)
def library_has_the_query():
    """The rule restated here is the one of the library under test: without rt_tracer_section there is nothing to restate."""
    from raytracertest_amd import api
    assert hasattr(api.load_library(), "rt_tracer_section") and hasattr(api.RayTracer, "Section")


# one step beyond: how many of the 235 rows differ, and the first of them as (plane, its count there, its count at k = 0)
BEYOND = {RANGE[0] - 1: (3, (18, 193, 81)), RANGE[1] + 1: (22, (2, 114, 113))}


def _at(k):
    s = np.float64(2.0) ** k
    rows = (lc.rooms().astype(np.float64) * s).astype(f32)               # (exact: a power of two)
    spheres = (SPHERES.astype(np.float64) * s).astype(f32)
    planes = lattice_planes().astype(np.float64)
    planes[:, 0:3] *= s
    planes[:, 3:5] *= s * s
    with np.errstate(all="ignore"):
        return se.expected(planes.astype(f32), rows, 16, spheres=spheres)


def _differing(a, b):
    return np.nonzero((a[0] != b[0]).any(axis=1) | (a[1] != b[1]))[0]


def test_inside_its_range_the_rule_answers_the_same_rows_and_beyond_it_does_not():
    base = _at(0)
    acc = se.table(lattice_planes(), lc.rooms(), spheres=SPHERES)
    assert (base[1] > 16).sum() > 100 and acc[:, -2:].sum(axis=0).min() >= 50         # the planes cut the walls and both spheres
    lo, hi = RANGE
    for k in INSIDE_KS + (lo, hi):
        bad = _differing(_at(k), base)
        assert bad.size == 0, (k, bad[:5])
    for k in (lo - 1, hi + 1):
        got = _at(k)
        bad = _differing(got, base)
        print("k = %d, one step beyond [%d, %d]: %d of %d rows differ; plane %d counts %d for %d" %
              (k, lo, hi, bad.size, base[1].shape[0], bad[0] if bad.size else -1, got[1][bad[0]] if bad.size else -1,
               base[1][bad[0]] if bad.size else -1))
        assert bad.size > 0, k
        assert (bad.size, (int(bad[0]), int(got[1][bad[0]]), int(base[1][bad[0]]))) == BEYOND[k], k
