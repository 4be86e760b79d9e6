"""The dense-scene option matrix (tests/dense_cases.py) stays what tests/test_gpu_dense_options.py claims it is: every pair of
axis values in at least one case, every anchor present, frame shapes that run the launches they are named after."""
import dense_cases as dc


def test_cases_cover_every_pair_of_axis_values():
    covered = set()
    for c in dc.CASES:
        for axis, values in dc.AXES.items():
            assert c[axis] in values, (c["name"], axis, c[axis])
        assert not any(p in dc.pairs_of(c) for p in dc.INFEASIBLE), c["name"]
        covered |= dc.pairs_of(c)
    missing = dc.required_pairs() - covered
    assert not missing, sorted(tuple(sorted(p)) for p in missing)
    assert len({c["name"] for c in dc.CASES}) == len(dc.CASES)


def test_every_anchor_is_in_the_table():
    for what, holds in dc.ANCHORS.items():
        assert any(holds(c) for c in dc.CASES), "anchor missing: " + what


def test_cases_are_dense_scenes_and_the_shapes_launch_as_named():
    for c in dc.CASES:
        assert 4096 <= c["n_tris"] <= 9000, c["name"]            # dense scenes: the forms kernels need >= 4 096 triangles
        assert c["iters"] == "one" or dc.iterations(c) > 1, c["name"]
    W, rows, _, _ = dc.SHAPES["unsplit"]
    assert rows < 128 and dc.split_row(rows) == 0
    W, rows, full_h, r0 = dc.SHAPES["band"]
    assert rows >= 128 and r0 % 8 and r0 + rows <= full_h and dc.split_row(rows) > 0
    # split frames: each half of the launch has more than 4 x 4 macro tiles of 128 x 64 (rt_tracer.hpp: attach_macro_lists)
    W, rows, _, _ = dc.SHAPES["split"]
    r = dc.split_row(rows)
    for half in (r, rows - r):
        assert ((W + 127) // 128) * ((half + 63) // 64) > 16
    # the sphere behind the cloud, the one in front of it, the one off to the side
    z = dc.SPHERES[:, 2]
    assert z[0] + dc.SPHERES[0, 3] < -12.15 and z[1] - dc.SPHERES[1, 3] > -4.15 and abs(dc.SPHERES[2, 0]) > 5


def test_the_smooth_cases_use_edge_scenes_with_normals():
    c = next(c for c in dc.CASES if c["extras"] == "smooth")
    rows, edges = dc.scene(c, 11)
    assert edges and rows.shape == (3 * c["n_tris"], 4) and rows[:, 3].all()      # (.w: the packed vertex normals)
    rows, edges = dc.scene(dict(c, extras="none"), 11)
    assert not edges and rows.shape == (3 * c["n_tris"], 4)
