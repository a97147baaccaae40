"""The positional bisection of batch_verify_multi (verifier.bisect_tree) on the host alone, with a fake `holds` over a heap-ordered tree:
a node holds exactly when no LIVE bad leaf lies below it, which is what the pairing of a node's sum says for honest rho.  Verdicts are
exact, and the number of calls stays within 1 + 2 b log2 P for b bad leaves: a failing root, then at most two children per level on each
bad leaf's path.  A batch with nothing bad costs one call; a batch whose leaves are all masked costs none (there is nothing to pair)."""
import itertools

import pytest

from distributed_plonk_amd.verifier import bisect_tree, tree_leaves


def _run(P, K, bad, masked):
    """bisect_tree over K <= P leaves with `bad` failing and `masked` taken out of the fold; (verdicts, calls, nodes asked)."""
    live = [j not in masked for j in range(K)]
    asked = []

    def below(node):
        if node >= P - 1:
            return [node - (P - 1)]
        return below(2 * node + 1) + below(2 * node + 2)

    def holds(node):
        asked.append(node)
        return not any(j in bad and j < K and live[j] for j in below(node))

    verdict, calls = bisect_tree(P, live, holds)
    assert calls == len(asked) and len(set(asked)) == len(asked)          # no node is asked twice
    return verdict, calls, asked


@pytest.mark.parametrize("P", [8, 16])
def test_every_subset_of_up_to_three_bad_leaves(P):
    log_p = P.bit_length() - 1
    masked_sets = [set(), {0}, {P - 1}, {1, 2, P // 2}, set(range(0, P, 2))]
    seen = 0
    for b in range(4):
        for bad in itertools.combinations(range(P), b):
            for masked in masked_sets:
                verdict, calls, _ = _run(P, P, set(bad), masked)
                assert verdict == [j not in bad and j not in masked for j in range(P)], (bad, masked)
                effective = len(set(bad) - masked)                       # a masked bad leaf is rejected without a call
                assert calls <= 1 + 2 * effective * log_p, (bad, masked, calls)
                if effective == 0:
                    assert calls == (1 if len(masked) < P else 0)
                seen += 1
    assert seen == len(masked_sets) * sum(len(list(itertools.combinations(range(P), b))) for b in range(4))


@pytest.mark.parametrize("P,K", [(8, 5), (8, 7), (16, 9), (16, 13)])
def test_padding_leaves_are_never_asked(P, K):
    assert tree_leaves(K) == P
    for bad in [(), (0,), (K - 1,), (0, K - 1), (1, K // 2, K - 1)]:
        verdict, calls, asked = _run(P, K, set(bad), set())
        assert verdict == [j not in bad for j in range(K)]
        assert calls <= 1 + 2 * len(bad) * (P.bit_length() - 1)
        assert all(node < P - 1 + K for node in asked)                   # no padding leaf, and no node beyond the tree


def test_nothing_bad_is_one_call_and_all_masked_is_none():
    for P in (1, 2, 8, 16):
        assert _run(P, P, set(), set())[:2] == ([True] * P, 1)
        assert _run(P, P, set(), set(range(P)))[:2] == ([False] * P, 0)
        assert _run(P, P, set(range(P)), set(range(P)))[:2] == ([False] * P, 0)
    assert bisect_tree(1, [], lambda node: pytest.fail("asked")) == ([], 0)
    assert [tree_leaves(k) for k in (0, 1, 2, 3, 4, 5, 64, 65, 129)] == [1, 1, 2, 4, 4, 8, 64, 128, 256]


def test_a_single_leaf_and_a_failing_single_leaf():
    assert _run(1, 1, set(), set())[:2] == ([True], 1)
    assert _run(1, 1, {0}, set())[:2] == ([False], 1)


def test_the_right_child_of_a_failing_node_is_not_asked_when_the_left_one_holds():
    # bad leaf 7 of 8: root, then left halves hold and the right path is implied: 1 + 3 calls, where two per level would be 1 + 6
    verdict, calls, asked = _run(8, 8, {7}, set())
    assert verdict == [True] * 7 + [False] and asked == [0, 1, 5, 13]
    # bad leaf 0: the left child fails, so the right one has to be asked at every level
    verdict, calls, asked = _run(8, 8, {0}, set())
    assert verdict == [False] + [True] * 7 and calls == 7
