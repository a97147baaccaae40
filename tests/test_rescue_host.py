"""Rescue on the host: the pure-Python reference (tests/rescue_ref.py) against its committed fixtures, the package's default parameters
against the reference's, the MDS property of the matrix, and the builder gadgets — gate counts, levels, and the built permutation and
Merkle path solved by the sequential big-integer solver (tests/hint_ref.py) against the reference's values.  No GPU."""
import itertools
import json
import os
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd.rescue import RescueParams
from tests import rescue_ref as R
from tests.hint_ref import HintRefSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = list(R.CURVES)
GATES = 148                                             # 4 + 12 * (4 root5 + 4 lc + 4 pow5_lc)
PER_DEPTH = GATES + 3                                   # enforce_bool and two selects


def golden(curve):
    with open(os.path.join(ROOT, "tests", "golden", f"rescue_{curve}.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("curve", CURVES)
def test_reference_reproduces_the_fixtures(curve):
    g = golden(curve)
    assert g["params_sha256"] == R.params_sha256(curve)
    states, leaves = R.fixture_inputs(curve)
    r = R.MODULI[curve]
    assert len(g["states"]) == 8 and states[:3] == [[0] * 4, [r - 1] * 4, [1, 0, 0, 0]]
    for pair, s in zip(g["states"], states):
        assert [int(x, 16) for x in pair["in"]] == s
        assert [int(x, 16) for x in pair["out"]] == R.permute(curve, s)
    assert [int(x, 16) for x in g["leaves"]] == leaves and len(leaves) == 8
    nodes = R.merkle(curve, leaves)
    assert int(g["root"], 16) == nodes[0] and len(nodes) == 15
    for i in (0, 5, 7):                                 # a path recomputes to the root
        m, sibs, bits = 7 + i, [], []
        while m:
            sibs.append(nodes[m - 1 if m % 2 == 0 else m + 1])
            bits.append(int(m % 2 == 0))
            m = (m - 1) // 2
        assert bits == [(i >> j) & 1 for j in range(3)]
        assert R.root_from_path(curve, leaves[i], sibs, bits) == nodes[0]


@pytest.mark.parametrize("curve", CURVES)
def test_default_parameters_round_trip_to_the_reference(curve):
    f = _fr.FIELDS[curve]
    assert f.p == R.MODULI[curve]
    prm = RescueParams.default(curve)
    limbs = prm.limbs()
    assert limbs.shape == (116, 4) and limbs.dtype == np.uint64
    assert [f.from_limbs(l) for l in limbs] == R.flat_params(curve)
    M, K = R.default_params(curve)
    assert prm.mds == M and prm.round_keys == K
    again = RescueParams(curve, M, K)                   # injected tables give the same bytes
    assert np.array_equal(again.limbs(), limbs)
    with pytest.raises(ValueError):
        RescueParams(curve, M[:3], K)
    with pytest.raises(ValueError):
        RescueParams(curve, M, K[:24])


def det(m, p):
    if len(m) == 1:
        return m[0][0] % p
    return sum((-1) ** j * m[0][j] * det([row[:j] + row[j + 1:] for row in m[1:]], p) for j in range(len(m))) % p


@pytest.mark.parametrize("curve", CURVES)
def test_mds_matrix_has_no_vanishing_minor(curve):
    p = R.MODULI[curve]
    M, _ = R.default_params(curve)
    count = 0
    for k in range(1, 5):
        for rows in itertools.combinations(range(4), k):
            for cols in itertools.combinations(range(4), k):
                assert det([[M[i][j] for j in cols] for i in rows], p) != 0, (rows, cols)
                count += 1
    assert count == 16 + 36 + 16 + 1


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [1, 3])
def test_permutation_gadget_gate_count_levels_and_values(curve, m):
    p = R.MODULI[curve]
    rnd = random.Random(100 + m)
    b = BD.CircuitBuilder(curve)
    ins = [b.input(m) for _ in range(4)]
    before = b.num_gates
    out = b.rescue_permutation(ins)
    assert b.num_gates - before == GATES * m
    assert len(out) == 4 and all(np.atleast_1d(o).shape == (m,) for o in out)
    built = b.build()
    assert built.has_hints and int((built.hint_op == BD.HINT_ROOT5).sum()) == 48 * m
    states = [[rnd.randrange(p) for _ in range(4)] for _ in range(m)]
    states[0] = [0, p - 1, 1, rnd.randrange(p)]
    # input_vars lists element 0 of every instance first: ins[e] are m consecutive ids
    values = [states[i][e] for e in range(4) for i in range(m)]
    ref = HintRefSolver(built, values)
    wit, lvl = ref.solve()
    assert ref.unsatisfied_gates(wit) == []
    for i in range(m):
        assert [wit[int(np.atleast_1d(o)[i])] for o in out] == R.permute(curve, states[i])
    assert max(lvl[int(np.atleast_1d(o)[0])] for o in out) == 36          # 37 levels, counted from 0
    # scalar ids give scalar ids, and the gadget refuses what it cannot broadcast before emitting anything
    b2 = BD.CircuitBuilder(curve)
    a, c = b2.input(), b2.input(2)
    assert all(isinstance(v, int) for v in b2.rescue_permutation([a, a, b2.zero, b2.one]))
    g0 = b2.num_gates
    for bad in ([a, a, a], [a, b2.input(3), c, a], [a, a, a, 10 ** 6]):
        with pytest.raises(ValueError):
            b2.rescue_permutation(bad)
    with pytest.raises(ValueError):
        b2.rescue_permutation([a, a, a, a], params=RescueParams.default([x for x in CURVES if x != curve][0]))
    assert b2.num_gates == g0


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [1, 2])
def test_merkle_root_gadget_gate_count_and_values(curve, m):
    p = R.MODULI[curve]
    rnd = random.Random(200 + m)
    depth = 3
    leaves = [rnd.randrange(p) for _ in range(1 << depth)]
    nodes = R.merkle(curve, leaves)
    b = BD.CircuitBuilder(curve)
    root = b.public_input()
    leaf = b.input(m)
    bits = [b.input(m) for _ in range(depth)]
    sibs = [b.input(m) for _ in range(depth)]
    before = b.num_gates
    got = b.merkle_root(leaf, bits, sibs)
    assert b.num_gates - before == depth * PER_DEPTH * m
    b.enforce_equal(got, root)
    built = b.build()
    which = [5, 2][:m]
    cols = {"leaf": [], "bits": [[] for _ in range(depth)], "sibs": [[] for _ in range(depth)]}
    for i in which:
        cols["leaf"].append(leaves[i])
        node = (1 << depth) - 1 + i
        for j in range(depth):
            cols["bits"][j].append(int(node % 2 == 0))
            cols["sibs"][j].append(nodes[node - 1 if node % 2 == 0 else node + 1])
            node = (node - 1) // 2
    values = cols["leaf"] + [x for c in cols["bits"] for x in c] + [x for c in cols["sibs"] for x in c]
    ref = HintRefSolver(built, values, [nodes[0]])
    wit, _ = ref.solve()
    assert [wit[int(v)] for v in np.atleast_1d(got)] == [nodes[0]] * m
    assert ref.unsatisfied_gates(wit) == []
    # a wrong sibling or a non-boolean index bit leaves some gate unsatisfied
    wrong = list(values)
    wrong[m + depth * m] = (wrong[m + depth * m] + 1) % p
    ref = HintRefSolver(built, wrong, [nodes[0]])
    assert ref.unsatisfied_gates(ref.solve()[0]) != []
    wrong = list(values)
    wrong[m] = 2
    ref = HintRefSolver(built, wrong, [nodes[0]])
    assert ref.unsatisfied_gates(ref.solve()[0]) != []
    with pytest.raises(ValueError):
        b.merkle_root(leaf, bits, sibs[:2])
