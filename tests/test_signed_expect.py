"""CPU checks of the signed point queries' host side and of the restated pipeline (signed_expect.py): the library's feature table
against an independent float64 construction; the sign of the restated answer against analytic inside tests; that the face
normal alone would not do; that every feature code occurs; and that exact ties do not make the side ambiguous."""
import numpy as np
import pytest

import closest_expect as ce
import signed_expect as se
from lattice_cases import rooms
from query_accel_expect import records_of_rows

INF = np.float32(np.inf)


def _pipeline(pts, rows, table, spheres=None, normal_of=None):
    """The restated signed query: the brute-force winners, then their sides."""
    hits = ce.expected(ce.with_radius(pts, INF), rows, spheres=spheres)
    return hits, se.sides_of(pts, hits["prim"], rows, table, spheres=spheres, normal_of=normal_of)


@pytest.fixture(scope="module")
def closed():
    """{name: (rows, table, points, decided, inside, hits, sides)} of the three closed meshes, computed once."""
    from raytracertest_amd import api
    out = {}
    for name, (rows, inside_of) in se.closed_meshes().items():
        table = api.feature_normals(rows)
        pts = se.probe_points(rows)
        hits, sides = _pipeline(pts, rows, table)
        out[name] = (rows, table, pts, se.far_enough(pts, rows), inside_of(pts), hits, sides)
    return out


SCENES = {"cube": se.cube, "l_prism": se.l_prism, "spike": se.spike, "square": se.square, "rooms": rooms,
          "random_1100": lambda: ce.random_scene(1100, 3), "degenerate": ce.degenerate_scene}


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("edges", [False, True])
def test_library_table_equals_the_float64_construction(name, edges):
    from raytracertest_amd import api
    rows = SCENES[name]()
    if edges:                                                    # the same triangles as v0, e1, e2 rows
        r = rows.reshape(-1, 3, 4).copy()
        r[:, 1, :3] -= r[:, 0, :3]
        r[:, 2, :3] -= r[:, 0, :3]
        rows = r.reshape(-1, 4)
    got, info = api.feature_normals(rows, edges, return_info=True)
    want = se.feature_table64(rows, edges)
    assert got.shape == want.shape == (rows.shape[0] // 3, 7, 4) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print("%s edges=%d: max |difference| = %.3g (2^-22 = %.3g), info %s" % (name, edges, err, se.TABLE_TOL, info))
    assert err <= se.TABLE_TOL
    assert (got[:, :, 3] == 0).all()
    length = np.linalg.norm(got[:, :, :3].astype(np.float64), axis=2)
    assert (np.abs(length[length != 0] - 1) < 1e-6).all()
    assert info["triangles"] == rows.shape[0] // 3 and info["bytes"] == got.nbytes


def test_zero_area_triangles_contribute_nothing():
    from raytracertest_amd import api
    rows = ce.degenerate_scene()
    tab, info = api.feature_normals(rows, return_info=True)
    flat = np.arange(3, 8)                                       # degenerate_scene's five zero-area triangles
    assert (tab[flat, 0] == 0).all() and info["contributing"] == rows.shape[0] // 3 - 5
    keep = np.setdiff1d(np.arange(rows.shape[0] // 3), flat)
    alone = api.feature_normals(rows.reshape(-1, 3, 4)[keep].reshape(-1, 4))
    assert np.array_equal(tab[keep], alone)                      # the others' normals are what they are without them


def test_welding_takes_minus_zero_as_plus_zero():
    from raytracertest_amd import api
    a = np.zeros((2, 3, 4), np.float32)
    a[0, :, :3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    a[1, :, :3] = [[-0.0, 0, -0.0], [0, 0, 1], [1, -0.0, 0]]      # shares the edge (0,0,0)-(1,0,0); normal (0, 1, 0)
    tab = api.feature_normals(a.reshape(-1, 4))
    want = np.float32([0, 1, 1]) / np.float32(np.sqrt(2))
    assert np.allclose(tab[0, 4, :3], want, atol=1e-7) and np.array_equal(tab[0, 4], tab[1, 5])
    assert np.array_equal(tab[0, 1], tab[1, 1]) and np.array_equal(tab[0, 2], tab[1, 3])


@pytest.mark.parametrize("name", ["cube", "l_prism", "spike"])
def test_restated_sign_equals_the_analytic_inside_test(closed, name):
    rows, table, pts, decided, inside, hits, sides = closed[name]
    excluded = 1.0 - decided.mean()
    wrong = np.nonzero(decided & ((sides["s"] < 0) != inside))[0]
    print("%s: %d points, %.2f %% within 1e-4 of the surface, %d wrong signs" % (name, pts.shape[0], 100 * excluded, wrong.size))
    assert excluded <= 0.05
    assert (hits["prim"] >= 0).all() and (sides["s"][decided] != 0).all()
    assert wrong.size == 0, (pts[wrong[:5]], sides[wrong[:5]])
    assert inside[decided].any() and (~inside[decided]).any()


@pytest.mark.parametrize("name", ["l_prism", "spike"])
def test_the_face_normal_alone_gets_a_sign_wrong(closed, name):
    """Teeth: the same pipeline with the winner's face normal in place of the table's feature normal."""
    rows, table, pts, decided, inside, hits, _ = closed[name]
    sides = se.sides_of(pts, hits["prim"], rows, table, normal_of=se.face_normal_of(table))
    wrong = decided & ((sides["s"] < 0) != inside)
    print("%s: the face normal gets %d of %d decided signs wrong (features %s)" %
          (name, wrong.sum(), decided.sum(), np.unique(sides["feature"][wrong])))
    assert wrong.sum() >= 1
    assert (sides["feature"][wrong] != 0).all()                  # never where the nearest point is inside the face


def test_every_feature_code_occurs(closed):
    seen = set()
    for rows, table, pts, decided, inside, hits, sides in closed.values():
        seen |= set(np.unique(sides["feature"]).tolist())
    rows = se.cube()
    sph = np.float32([[2.5, 0.5, 0.0, 0.5]])
    pts = np.float32([[2.4, 0.5, 0.0], [3.5, 0.5, 0.0], [0.2, 0.6, 0.0]])
    hits, sides = _pipeline(pts, rows, se.feature_table64(rows), spheres=sph)
    assert hits["prim"][:2].tolist() == [12, 12] and 0 <= hits["prim"][2] < 12
    assert sides["s"][0] < 0 < sides["s"][1]                      # inside and outside the sphere
    seen |= set(sides["feature"].tolist())
    assert seen >= set(range(8)), seen
    none = se.sides_of(pts, [-1, -1, 99], rows, se.feature_table64(rows), spheres=sph)
    assert none["feature"].tolist() == [-1, -1, -1] and (none["s"] == 0).all()


def test_boundary_edges_of_an_open_mesh_carry_their_one_face_normal():
    rows = se.square()
    tab = se.feature_table64(rows)
    assert (tab[:, :, :3] == np.float32([0, 0, 1])).all()
    pts = np.float32([[1.5, 0.5, 0.75], [1.5, 0.5, 0.25], [-1, -1, 2], [0.5, 0.5, 0.4]])
    _, sides = _pipeline(pts, rows, tab)
    assert (np.sign(sides["s"]) == [1, -1, 1, -1]).all() and set(sides["feature"][:3].tolist()) <= {1, 2, 3, 4, 5, 6}


def test_exact_ties_do_not_make_the_side_ambiguous():
    """At the lattice's exact-tie points several triangles compute the same t.  Those whose nearest point is the SAME point share
    the feature that holds it -- welded, one table entry -- so whichever of them is taken as the winner the side has the same
    bits.  (Triangles that tie through different nearest points, as the six walls of a cell do for its centre, are different
    surfaces; rooms() winds its walls alternately, so they may differ in side as they differ in everything else.)"""
    rows = rooms()
    table = se.feature_table64(rows)
    pts = ce.lattice_points()
    t, u, v, _ = ce.table(pts, rows)
    v0, e1, e2 = records_of_rows(rows, False)
    groups = members = 0
    for i in range(pts.shape[0]):
        tied = np.nonzero(t[i] == t[i].min())[0]
        if tied.size < 2:
            continue
        c = (v0[tied] + u[i, tied, None] * e1[tied]) + v[i, tied, None] * e2[tied]      # exact: small dyadic numbers
        sides = se.sides_of(np.repeat(pts[i:i + 1], tied.size, 0), tied, rows, table)
        for key in np.unique(c, axis=0):
            same = (c == key).all(axis=1)
            if same.sum() > 1:
                groups += 1
                members += int(same.sum())
                assert np.unique(sides["s"][same].view(np.uint32)).size == 1, (pts[i], tied[same], sides[same])
    print("%d tie groups with %d members" % (groups, members))
    assert groups >= 100
