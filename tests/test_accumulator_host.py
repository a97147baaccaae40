"""The ternary Rescue accumulator on the host: the pure-Python reference (tests/accumulator_ref.py) against itself and its committed
fixtures, and the builder gadgets — rescue_hash3's wiring, accumulator_root's gate count against a hand count, its values under the
sequential big-integer solver (tests/hint_ref.py), what it refuses — and the size of the reference's circuit shape.  No GPU."""
import json
import os
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd.membership import membership_circuit, num_input_rows
from distributed_plonk_amd.rescue import RescueParams, acc_level_counts
from tests import accumulator_ref as A
from tests import rescue_ref as R
from tests.hint_ref import HintRefSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = list(A.CURVES)
PERMUTATION = 148                                       # 4 + 12 * (4 root5 + 4 lc + 4 pow5_lc): tests/test_rescue_host.py
# Per level, counted by hand from the gadget's definition: enforce_bool(is_left) 1, enforce_bool(is_right) 1, is_left + is_right 1 (add) and
# its enforce_bool 1, the two selects 2, mid = cur + sib1 + sib2 - l - r has five terms and a gate four input wires, so 2 — and the hash.
PER_LEVEL = PERMUTATION + 1 + 1 + 2 + 2 + 2


def golden(curve):
    with open(os.path.join(ROOT, "tests", "golden", f"accumulator_{curve}.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("curve", CURVES)
def test_fixture_equals_the_reference_live(curve):
    g = golden(curve)
    r = A.MODULI[curve]
    elems = A.fixture_elems(curve)
    assert g["params_sha256"] == R.params_sha256(curve)
    assert [int(x, 16) for x in g["elems"]] == elems and len(elems) == 10 and elems[0] == 0 and elems[-1] == r - 1
    levels = A.acc_nodes(curve, g["height"], elems)
    assert g["height"] == 3 and [[int(x, 16) for x in l] for l in g["levels"]] == levels
    assert [len(l) for l in levels] == [10, 4, 2, 1] and int(g["root"], 16) == levels[-1][0]
    assert sorted(g["paths"]) == ["0", "4", "9"]
    for uid, p in g["paths"].items():
        sib1, sib2, pos = A.acc_path(levels, int(uid))
        assert ([int(x, 16) for x in p["sib1"]], [int(x, 16) for x in p["sib2"]], p["positions"]) == (sib1, sib2, pos)
    assert g["tall_height"] == 32 and int(g["tall_root"], 16) == A.acc_nodes(curve, 32, elems)[-1][0]


@pytest.mark.parametrize("curve", CURVES)
def test_every_path_of_a_ten_leaf_tree_recomputes_the_root(curve):
    elems = A.fixture_elems(curve)
    levels = A.acc_nodes(curve, 3, elems)
    root = levels[-1][0]
    for uid in range(10):
        sib1, sib2, pos = A.acc_path(levels, uid)
        assert pos == [uid % 3, uid // 3 % 3, uid // 9 % 3]
        assert A.root_from_path(curve, uid, elems[uid], sib1, sib2, pos) == root
        assert A.root_from_path(curve, (uid + 1) % 10, elems[uid], sib1, sib2, pos) != root       # the uid is in the leaf hash
    # ragged levels: uid 9 is alone in its group at level 0, and its parent at level 1 too
    sib1, sib2, _ = A.acc_path(levels, 9)
    assert (sib1[0], sib2[0], sib1[1], sib2[1]) == (0, 0, 0, 0) and sib2[2] == 0 and sib1[2] == levels[2][0]
    # an empty subtree is 0, not a hash, and the chain above one node is hash3(x, 0, 0)
    tall = A.acc_nodes(curve, 5, elems[:1])
    assert [len(l) for l in tall] == [1] * 6
    assert tall[0][0] == A.hash3(curve, 0, 0, elems[0]) and all(tall[j + 1][0] == A.hash3(curve, tall[j][0], 0, 0) for j in range(5))
    assert A.level_counts(32, 50) == [50, 17, 6, 2] + [1] * 29 == acc_level_counts(32, 50)
    for bad in ((0, 1), (41, 1), (2, 0), (2, 10)):
        with pytest.raises(ValueError):
            acc_level_counts(*bad)


@pytest.mark.parametrize("curve", CURVES)
def test_rescue_hash3_wires_three_inputs_and_zero(curve):
    p = A.MODULI[curve]
    rnd = random.Random(300)
    b = BD.CircuitBuilder(curve)
    a, c, d = b.input(), b.input(), b.input()
    before = b.num_gates
    out = b.rescue_hash3(a, c, d)
    assert isinstance(out, int) and b.num_gates - before == PERMUTATION
    built = b.build()
    # the first four gates add K[0] to (a, c, d, zero) on wire 0
    assert [int(built.wire_vars[0, before + i]) for i in range(4)] == [a, c, d, b.zero]
    vals = [0, p - 1, rnd.randrange(p)]
    wit, _ = HintRefSolver(built, vals).solve()
    assert wit[out] == A.hash3(curve, *vals)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [1, 2])
def test_accumulator_root_gate_count_and_values(curve, m):
    p = A.MODULI[curve]
    height = 3
    elems = A.fixture_elems(curve)
    levels = A.acc_nodes(curve, height, elems)
    root = levels[-1][0]
    b = BD.CircuitBuilder(curve)
    pub = b.public_input()
    uid, elem = b.input(m), b.input(m)
    rows = [[b.input(m) for _ in range(4)] for _ in range(height)]
    before = b.num_gates
    got = b.accumulator_root(uid, elem, *[[r[i] for r in rows] for i in range(4)])
    assert b.num_gates - before == (PERMUTATION + height * PER_LEVEL) * m
    b.enforce_equal(got, pub)
    built = b.build()
    which = [9, 4][:m]                                  # 9: the ragged edge at two levels; 4: a middle position

    def values(which):
        vals = list(which) + [elems[i] for i in which]
        for j in range(height):
            paths = [A.acc_path(levels, i) for i in which]
            vals += [pth[0][j] for pth in paths] + [pth[1][j] for pth in paths]
            vals += [int(pth[2][j] == 0) for pth in paths] + [int(pth[2][j] == 2) for pth in paths]
        return vals

    good = values(which)
    ref = HintRefSolver(built, good, [root])
    wit, _ = ref.solve()
    assert [wit[int(v)] for v in np.atleast_1d(got)] == [root] * m
    assert ref.unsatisfied_gates(wit) == []
    row = lambda j, i: (2 + 4 * j + i) * m              # first value of input row i of level j
    for at, value in ((row(1, 0), (good[row(1, 0)] + 1) % p),        # a wrong sibling
                      (row(0, 3), 1 - good[row(0, 3)]),              # is_right flipped: with is_left set both are 1, else a wrong position
                      (row(0, 2), 2),                                # a flag of 2
                      (0, (good[0] + 1) % p)):                       # another uid in the leaf hash
        wrong = list(good)
        wrong[at] = value
        ref = HintRefSolver(built, wrong, [root])
        assert ref.unsatisfied_gates(ref.solve()[0]) != [], at
    # is_left = is_right = 1 fails at the flags even where cur, sib1 and sib2 are all equal
    both = list(good)
    both[row(0, 2)] = both[row(0, 3)] = 1
    ref = HintRefSolver(built, both, [root])
    assert ref.unsatisfied_gates(ref.solve()[0]) != []


def test_refused_arguments_emit_nothing():
    b = BD.CircuitBuilder("bn254")
    u, e = b.input(), b.input()
    s = [b.input() for _ in range(4)]
    two, three = b.input(2), b.input(3)
    g0, v0 = b.num_gates, b.num_vars
    bad = [
        lambda: b.accumulator_root(u, e, [s[0]], [s[1]], [s[2]], []),                      # lists of different lengths
        lambda: b.accumulator_root(u, e, [s[0], s[0]], [s[1]], [s[2]], [s[3]]),
        lambda: b.accumulator_root(u, e, [s[0]], [s[1]], [s[2]], [10 ** 6]),               # an unknown id
        lambda: b.accumulator_root(two, e, [three], [s[1]], [s[2]], [s[3]]),               # arrays of two lengths
        lambda: b.accumulator_root(u, e, [s[0]], [s[1]], [s[2]], [s[3]], params=RescueParams.default("bls12_381")),
        lambda: b.rescue_hash3(u, e, 10 ** 6),
        lambda: b.rescue_hash3(two, three, e),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert (b.num_gates, b.num_vars) == (g0, v0)
    for args in (("bn254", 0, 1), ("bn254", 41, 1), ("bn254", 3, 0)):
        with pytest.raises(ValueError):
            membership_circuit(*args)


def test_membership_circuit_has_the_reference_shape():
    built = membership_circuit("bn254", 32, 50)
    assert built.n == 2 ** 18
    assert built.num_public == 1 and len(built.input_vars) == num_input_rows(32) * 50 == 130 * 50
    # 2 constants, the public root, and per membership the gadget and its equality with the root
    assert built.num_gates_unpadded == 3 + 50 * (PERMUTATION + 32 * PER_LEVEL + 1)
    # the inputs are consecutive ids in creation order: row t of the path kernel's output is input_vars[t * m:][:m]
    assert np.array_equal(np.diff(built.input_vars), np.ones(130 * 50 - 1, dtype=np.int64))
    small = membership_circuit("bls12_381", 3, 1)       # m = 1: scalar ids
    assert len(small.input_vars) == 14 and small.n == 1024
