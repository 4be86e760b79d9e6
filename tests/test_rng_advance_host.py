"""The host tables behind the owed RNG draws (rt_rng_host.hpp): advancing the XORWOW xorshift words by n draws through the
4-bit window table of T^n equals n single steps.  No GPU."""
import numpy as np
import pytest

from raytracertest_amd import api

N_FIXED = [0, 1, 4, 5, 6, 47, 48, 96, 97, 768, 3 * 16 * 64 + 1]
N_RANDOM = [int(x) for x in np.random.default_rng(20261017).integers(0, 1 << 20, 1000)]
STATES = np.random.default_rng(7).integers(0, 1 << 32, (64, 5), dtype=np.uint64).astype(np.uint32)
M32 = 0xFFFFFFFF


def xorshift_step(v):
    """Random.cuh's generator restated: one draw's change of v0..v4."""
    t = v[0] ^ (v[0] >> 2)
    return [v[1], v[2], v[3], v[4], ((v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))) & M32]


def columns_after(n):
    """The 64 states as columns of Python ints, stepped n times (vectorised over the states)."""
    v = [STATES[:, w].astype(np.uint64) for w in range(5)]
    for _ in range(n):
        t = v[0] ^ (v[0] >> np.uint64(2))
        v = [v[1], v[2], v[3], v[4], ((v[4] ^ (v[4] << np.uint64(4))) ^ (t ^ (t << np.uint64(1)))) & np.uint64(M32)]
    return np.stack(v, axis=1).astype(np.uint32)


def test_python_step_matches_library_step():
    s = [int(x) for x in STATES[0]]
    assert [int(x) for x in api.dbg_rng_advance_host(STATES[0], 1, False)] == xorshift_step(s)
    assert np.array_equal(columns_after(3)[0], api.dbg_rng_advance_host(STATES[0], 3, False))


@pytest.mark.parametrize("n", N_FIXED)
def test_table_equals_stepping_equals_n_steps(n):
    want = columns_after(n)
    tab, stp = api.dbg_rng_advance_host(STATES, n, True), api.dbg_rng_advance_host(STATES, n, False)
    assert np.array_equal(tab, stp) and np.array_equal(stp, want)
    for i in (0, 63):                                                    # the one-state entry point
        assert np.array_equal(api.dbg_rng_advance_host(STATES[i], n, True), want[i])
        assert np.array_equal(api.dbg_rng_advance_host(STATES[i], n, False), want[i])


def test_table_equals_stepping_random_n():
    """1 000 seeded n < 2^20, each over the 64 states: the table product against the library's stepping -- which the test
    above holds against n applications of xorshift_step, as does this one for the n below 2^14."""
    for n in N_RANDOM:
        tab, stp = api.dbg_rng_advance_host(STATES, n, True), api.dbg_rng_advance_host(STATES, n, False)
        assert np.array_equal(tab, stp), n
        if n < (1 << 14):
            assert np.array_equal(stp, columns_after(n)), n


def test_powers_add():
    """T^a T^b = T^(a+b) on random vectors."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        a, b = (int(x) for x in rng.integers(0, 1 << 19, 2))
        v = rng.integers(0, 1 << 32, 5, dtype=np.uint64).astype(np.uint32)
        ab = api.dbg_rng_advance_host(api.dbg_rng_advance_host(v, b, True), a, True)
        assert np.array_equal(ab, api.dbg_rng_advance_host(v, a + b, True)), (a, b)
        assert np.array_equal(ab, api.dbg_rng_advance_host(api.dbg_rng_advance_host(v, a, True), b, True)), (a, b)
