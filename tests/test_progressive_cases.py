"""tests/progressive_cases.py holds what it promises, without a device: schedule() is the reference's loop
(RayTracerImpl.cu:246-273) cut into launches that partition it, and the images expected() yields for one case differ from one
another in so many pixels that an update showing another iteration, or the other host image, cannot pass
tests/test_gpu_progressive.py."""
import itertools

import numpy as np
import pytest

import progressive_cases as pc


def reference_loop(iterationCount, updateInterval, mUpdateCallback):
    """RayTracerImpl.cu:246-273, statement by statement: the order of kernel runs and update callbacks"""
    events = []
    i = 0
    while i < iterationCount:                                          # :246
        events.append(("kernel", i))                                   # :249
        if mUpdateCallback is not None and i > 0 and updateInterval > 0 and i % updateInterval == 0:   # :256
            events.append(("update", i))                               # :265, :272
        i += 1
    return events


def check_schedule(n, spp, interval, has_cb, fuse):
    what = (n, spp, interval, has_cb, fuse)
    points, launches = pc.schedule(n, spp, interval, has_cb, fuse)
    ref = reference_loop(n, interval, (lambda: None) if has_cb else None)
    assert points == [i for kind, i in ref if kind == "update"], what
    # replayed as the reference's event order: a launch is its kernel runs, an update launch then calls back
    replay = []
    for first, last, emit, update in launches:
        replay += [("kernel", i) for i in range(first, last + 1)]
        if update:
            replay.append(("update", last))
    assert replay == ref, what
    covered = [i for first, last, _, _ in launches for i in range(first, last + 1)]
    assert covered == list(range(n)), what                             # the launches partition 0 .. n - 1, in order
    assert all(first <= last and last - first + 1 <= max(1, fuse) for first, last, _, _ in launches), what
    assert [last for _, last, _, update in launches if update] == points, what     # every update point ends a launch
    for k, (first, last, emit, update) in enumerate(launches):
        assert emit == (update or k == len(launches) - 1), what        # only the last launch and the update launches emit
        assert not update or last in points, what
    if not has_cb or interval == 0:
        assert points == [] and not any(u for _, _, _, u in launches), what
    if n == 0:
        assert launches == []
    return points, launches


@pytest.mark.parametrize("case", pc.CASES + [pc.CPP], ids=[c["name"] for c in pc.CASES] + ["cpp_driver"])
def test_schedule_of_every_case(case):
    for has_cb, fuse in itertools.product((True, False), (pc.fuse_of(case), 1)):
        check_schedule(case["n"], case["spp"], case["interval"], has_cb, fuse)


def test_schedule_of_the_cases_is_the_one_their_seam_needs():
    sched = lambda name: pc.schedule(pc.BY_NAME[name]["n"], pc.BY_NAME[name]["spp"], pc.BY_NAME[name]["interval"], True, pc.fuse_of(pc.BY_NAME[name]))
    assert sched("classic") == ([3, 6, 9], [(0, 3, True, True), (4, 6, True, True), (7, 9, True, True)])
    points, launches = sched("every")
    assert points == [1, 2, 3, 4, 5, 6] and launches == [(0, 1, True, True)] + [(i, i, True, True) for i in range(2, 7)]
    assert sched("groups") == ([100], [(0, 63, False, False), (64, 100, True, True), (101, 149, True, False)])
    points, launches = sched("settle")
    assert len(launches) == 20 and len(points) == 19                   # 19 launches behind the first, all of its owe key: > 16
    assert pc.fuse_of(pc.BY_NAME["scan"]) == 1 and len(sched("scan")[1]) == 6
    assert pc.fuse_of(pc.BY_NAME["nofuse"]) == 1 and len(sched("nofuse")[1]) == 5
    assert sched("one") == ([], [(0, 0, True, False)]) and sched("none") == ([], [])
    assert pc.BY_NAME["groups"]["frame"][1] >= 128 and pc.BY_NAME["settle"]["frame"][1] >= 128       # TraceEnqueue splits these
    assert sched("spheres") == ([3, 6], [(0, 3, True, True), (4, 6, True, True)])
    assert [(c["frame"], c["n"], c["spp"], c["interval"]) for c in pc.MULTI] == [((64, 50), 10, 1, 3), ((64, 50), 7, 2, 1)]
    assert pc.schedule(100, 1, 10, True, 64)[0] == list(range(10, 100, 10))                             # the C++ driver's nine updates


def test_schedule_of_random_arguments():
    rng = np.random.default_rng(20)
    for _ in range(3000):
        n, spp, fuse = int(rng.integers(0, 200)), int(rng.integers(0, 80)), int(rng.choice([1, 2, 3, 7, 16, 64]))
        interval = int(rng.choice([0, 1, 2, 3, 5, 10, 64, 65, 100, 250]))
        check_schedule(n, spp, interval, bool(rng.integers(0, 2)), fuse)


VARIANTS = [(c, mode, nearest) for c in pc.CASES + pc.MULTI + [pc.CPP] for mode, nearest in c["variants"]]


@pytest.mark.parametrize("case,mode,nearest", VARIANTS, ids=["%s-m%d%s" % (c["name"], m, "-nearest" if nh else "") for c, m, nh in VARIANTS])
def test_any_two_expected_images_of_a_case_differ_widely(orc, case, mode, nearest):
    """The teeth of the GPU tests, a condition on the inputs: within one Trace, and between a Trace and the one behind it on
    the same tracer, any two images differ in at least MIN_DIFFERING of the pixels."""
    first = pc.expected(orc, case, mode=mode, nearest=nearest)
    second = pc.expected(orc, case, o=first["o"])
    assert [i for i, _ in first["updates"]] == pc.schedule(case["n"], case["spp"], case["interval"], True, 1)[0]
    assert first["final"].shape == case["frame"][::-1]
    assert (first["counts"] == case["n"] * case["spp"]).all()
    if case["n"] > 0 and case["interval"] > 0 and (case["n"] - 1) % case["interval"] == 0 and case["n"] > 1:
        assert np.array_equal(first["updates"][-1][1], first["final"])  # the last iteration is an update point and the end
    images = [("first " + k, im) for k, im in pc.images_of(first)] + [("second " + k, im) for k, im in pc.images_of(second)]
    if case["n"] == 0:                                                 # cleared accumulators: both Traces show the same image
        assert len(images) == 2 and np.array_equal(images[0][1], images[1][1])
        return
    assert len(images) >= 2
    worst = min((pc.differing(a, b), ka, kb) for (ka, a), (kb, b) in itertools.combinations(images, 2))
    print("%s mode %d nearest %d: %d images, smallest differing fraction %.4f (%s | %s)" % (case["name"], mode, nearest, len(images), *worst))
    assert worst[0] >= pc.MIN_DIFFERING, worst


def test_stopped_state_is_a_shorter_trace(orc):
    """expected(n=m): the buffers after m iterations, and the same update images as the long Trace up to there"""
    case = pc.BY_NAME["every"]
    full = pc.expected(orc, case)
    part = pc.expected(orc, case, n=4)
    assert (part["counts"] == 4 * case["spp"]).all() and len(part["updates"]) == 3
    for (i, a), (j, b) in zip(part["updates"], full["updates"]):
        assert i == j and np.array_equal(a, b)
    assert not np.array_equal(part["rng"], full["rng"])


def test_fnv1a_is_the_drivers_hash():
    assert pc.fnv1a(np.zeros(0, np.uint32)) == 1469598103934665603
    assert pc.fnv1a(np.array([1], np.uint32)) == ((1469598103934665603 ^ 1) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
