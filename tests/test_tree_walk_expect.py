"""tree_walk_expect.walk on a hand-built tree of four nodes, where the visiting order, the marks and the overflow can be read off:

    node 0   slots: node 1 (key 2), node 2 (key 2), node 3 (key 7), leaf {8} (key -inf)
    node 3   slots: leaf {0, 1} (key 1), EMPTY (key 9), leaf {2} (key 4), leaf {3} (skipped)
    node 1   slots: leaf {4, 5} (key 3), EMPTY, EMPTY, EMPTY
    node 2   slots: leaf {6, 7} (key 3), EMPTY, EMPTY, EMPTY

Node 0 enters node 3 and leaves [leaf {8}, node 2, node 1] waiting, node 1 on top: the better on top, and of the two equal keys
the lower slot first.  Node 3 enters leaf {2} and pushes leaf {0, 1}: four entries wait, the mark.  Then the pops: leaf {0, 1},
node 1, node 2, leaf {8}, whose key was clamped to -FLT_MAX."""
import numpy as np
import pytest

from query_expect import FLT_MAX
from tree_walk_expect import EMPTY, LEAF, leaf_span, walk

NODE = np.dtype([("child", np.uint32, 4), ("key", np.float32, 4)])
SKIP = np.nan                                   # this file's mark for "child() answers None"


def leaf_ref(first, count):
    return LEAF | ((count - 1) << 28) | first


def tree():
    nodes = np.zeros(4, NODE)
    nodes[0] = ([1, 2, 3, leaf_ref(8, 1)], [2, 2, 7, -np.inf])
    nodes[1] = ([leaf_ref(4, 2), EMPTY, EMPTY, EMPTY], [3, 0, 0, 0])
    nodes[2] = ([leaf_ref(6, 2), EMPTY, EMPTY, EMPTY], [3, 0, 0, 0])
    nodes[3] = ([leaf_ref(0, 2), EMPTY, leaf_ref(2, 1), leaf_ref(3, 1)], [1, 9, 4, SKIP])
    return nodes


def child(nd):
    return [None if np.isnan(k) else k for k in nd["key"]]


def run(cap=12, start=True, stale=None, enforce_cap=True, hit=None, nodes=None):
    """-> (records in visiting order, (mark, overflow)); hit: the record whose test ends the walk."""
    seen = []

    def leaf(k):
        seen.append(k)
        return k == hit
    return seen, walk(tree() if nodes is None else nodes, cap, start, child, leaf, stale, enforce_cap)


def test_leaf_references_decode():
    assert leaf_span(leaf_ref(8, 1)) == (8, 1) and leaf_span(leaf_ref(0, 2)) == (0, 2) and leaf_span(leaf_ref(5, 4)) == (5, 4)


def test_the_order_is_best_first_stable_among_equal_keys_and_the_better_waits_on_top():
    seen, (mark, overflow) = run()
    assert seen == [2, 0, 1, 4, 5, 6, 7, 8]                              # never record 3 (skipped), nothing through EMPTY
    assert (mark, overflow) == (4, False)


def test_nothing_is_visited_without_a_start_or_without_nodes():
    assert run(start=False) == ([], (0, False))
    assert run(nodes=np.zeros(0, NODE)) == ([], (0, False))


def test_a_stale_entry_is_dropped_at_its_pop_and_sees_its_clamped_key():
    keys = []
    seen, result = run(stale=lambda key: keys.append(key) or False)
    assert seen == [2, 0, 1, 4, 5, 6, 7, 8] and result == (4, False)
    assert keys == [1, 2, 2, -FLT_MAX]                                   # in the order of the pops; -inf arrives clamped

    def bound_raised_at_record_0(to):
        """A keyed query whose bound is -inf until record 0 is tested: entries pushed before that are judged again."""
        bound, seen = [-np.inf], []

        def leaf(k):
            seen.append(k)
            if k == 0:
                bound[0] = to
        return seen, walk(tree(), 12, True, child, leaf, lambda key: key < bound[0])
    assert bound_raised_at_record_0(2.0) == ([2, 0, 1, 4, 5, 6, 7], (4, False))  # strictly behind: the entries AT 2 stay, leaf {8} goes
    assert bound_raised_at_record_0(2.5) == ([2, 0, 1], (4, False))              # nodes 1 and 2 are dropped unopened


def test_an_any_hit_ends_the_walk_in_the_middle_of_a_leaf():
    assert run(hit=0) == ([2, 0], (4, False))                            # record 1 of the same leaf is not tested
    assert run(hit=2) == ([2], (4, False))
    assert run(hit=5) == ([2, 0, 1, 4, 5], (4, False))


def test_the_capacity_is_asserted_or_overflows():
    assert run(cap=4)[1] == (4, False)                                   # four entries fit exactly
    with pytest.raises(AssertionError):
        run(cap=3)                                                       # node 3's push is the fourth
    assert run(cap=3, enforce_cap=False) == ([2, 4, 5, 6, 7, 8], (3, True))      # leaf {0, 1} was not stored
    # pushes go worst first, so a full stack loses the BEST of the waiting: node 1 at node 0, then leaf {0, 1} at node 3
    assert run(cap=2, enforce_cap=False) == ([2, 6, 7, 8], (2, True))
    assert run(cap=0, enforce_cap=False) == ([2], (0, True))
