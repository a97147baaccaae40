"""The builder's hinted operations on the host alone: inv, inv_or_zero, div, root5, bit and the operations composed from them (to_bits,
range_check, is_zero, is_equal, select, less_than).  The witness comes from tests/hint_ref.py (Python ints); every gate equation is then
checked with the reference's own residual — satisfied where the operation's contract holds, a named gate unsatisfied where it does not
— and the emitted wires, selectors and hint_op are pinned against the table of the builder's docstrings.  No device code runs here:
tests/test_gpu_hints.py compares the device solver with the same reference."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import fr as _fr
from tests.hint_ref import HintRefSolver

CURVES = ["bn254", "bls12_381"]
S = BD.SELECTOR_INDEX


def operands(curve: str, seed: int, count: int = 6):
    """0, 1, r - 1, 2^k - 1 and 2^k for some k, and random residues"""
    p = _fr.FIELDS[curve].p
    rnd = random.Random(seed)
    ks = [1, 7, 8, 63, 64, p.bit_length() - 2, p.bit_length() - 1]
    return [0, 1, p - 1] + [(1 << k) - 1 for k in ks] + [1 << k for k in ks] + [rnd.randrange(p) for _ in range(count)]


def solved(built, inputs, publics=()):
    ref = HintRefSolver(built, inputs, publics)
    witness, _ = ref.solve()
    return ref, witness


def selectors_at(ref, g):
    """{selector name: residue} of the non-zero selectors of gate g"""
    q = ref.selectors(g)
    return {name: q[i] for name, i in S.items() if q[i]}


# ---------------------------------------------------------------------------------------------- satisfied circuits
@pytest.mark.parametrize("curve", CURVES)
def test_primitives_are_satisfied_on_edge_and_random_operands(curve):
    p = _fr.FIELDS[curve].p
    xs = operands(curve, 1)
    nz = [x for x in xs if x]
    b = BD.CircuitBuilder(curve)
    x = b.input(len(xs))
    z = b.input(len(nz))
    inv, ioz, r5 = b.inv(z), b.inv_or_zero(x), b.root5(x)
    num, den = b.input(len(nz)), b.input(len(nz))
    quo = b.div(num, den)
    zero_quo = b.div(b.zero, b.zero)                                     # 0 / 0 = 0 satisfies y * 0 = 0
    bit0, bit_top, bit_255 = b.bit(x, 0), b.bit(x, p.bit_length() - 1), b.bit(x, 255)
    ks = np.arange(len(xs)) % p.bit_length()
    bit_each = b.bit(x, ks)
    built = b.build()
    rnd = random.Random(2)
    nums = [rnd.randrange(p) for _ in nz]
    ref, w = solved(built, xs + nz + nums + nz[::-1])
    assert ref.unsatisfied_gates(w) == []
    for i, v in enumerate(xs):
        assert w[ioz[i]] == (pow(v, -1, p) if v else 0)
        assert pow(w[r5[i]], 5, p) == v
        assert (w[bit0[i]], w[bit_top[i]], w[bit_255[i]], w[bit_each[i]]) == (v & 1, (v >> (p.bit_length() - 1)) & 1, 0, (v >> int(ks[i])) & 1)
    for i, v in enumerate(nz):
        assert w[inv[i]] * v % p == 1
        assert w[quo[i]] * nz[::-1][i] % p == nums[i]
    assert w[zero_quo] == 0


@pytest.mark.parametrize("curve", CURVES)
def test_composed_operations_are_satisfied_and_compute_what_they_say(curve):
    p = _fr.FIELDS[curve].p
    bl = p.bit_length()
    xs = operands(curve, 3)
    rnd = random.Random(4)
    b = BD.CircuitBuilder(curve)
    x, y = b.input(len(xs)), b.input(len(xs))
    iz = b.is_zero(x)
    eq = b.is_equal(x, y)
    sel = b.select(iz, x, y)                                             # iz is boolean by construction
    nb = 64
    small = [v % (1 << nb) for v in xs] + [0, (1 << nb) - 1]
    other = [rnd.randrange(1 << nb) for _ in xs] + [0, (1 << nb) - 1]
    s, t = b.input(len(small)), b.input(len(small))
    lt, gt = b.less_than(s, t, nb), b.less_than(t, s, nb)
    bits = b.to_bits(s, nb)
    b.range_check(s, nb)
    wide = b.input(3)
    wide_bits = b.to_bits(wide, bl - 1)                                  # the widest unique decomposition
    wl, wr = b.input(2), b.input(2)
    wide_lt = b.less_than(wl, wr, bl - 2)
    one_bit = b.to_bits(b.one, 1)
    built = b.build()
    ys = [xs[i] if i % 2 else rnd.randrange(p) for i in range(len(xs))]
    wides = [(1 << (bl - 1)) - 1, 1 << (bl - 2), rnd.randrange(1 << (bl - 1))]
    top = (1 << (bl - 2)) - 1
    ref, w = solved(built, xs + ys + small + other + wides + [top, 0] + [0, top])
    assert ref.unsatisfied_gates(w) == []
    for i, v in enumerate(xs):
        assert w[iz[i]] == (v == 0) and w[eq[i]] == (v == ys[i])
        assert w[sel[i]] == (v if v == 0 else ys[i])
    for i, v in enumerate(small):
        assert w[lt[i]] == (v < other[i]) and w[gt[i]] == (other[i] < v)
        assert [w[bits[k][i]] for k in range(nb)] == [(v >> k) & 1 for k in range(nb)]
    for i, v in enumerate(wides):
        assert sum(w[wide_bits[k][i]] << k for k in range(bl - 1)) == v
    assert [w[v] for v in wide_lt] == [0, 1]
    assert w[one_bit[0]] == 1


# ---------------------------------------------------------------------------------------------- unsatisfied circuits, each pinned
@pytest.mark.parametrize("curve", CURVES)
def test_inv_of_zero_is_unsatisfied_at_its_own_gate(curve):
    b = BD.CircuitBuilder(curve)
    x = b.input()
    y = b.inv(x)
    built = b.build()
    ref, w = solved(built, [0])
    assert w[y] == 0 and ref.unsatisfied_gates(w) == [int(built.def_gate[y])]
    assert ref.unsatisfied_gates(solved(built, [5])[1]) == []


@pytest.mark.parametrize("curve", CURVES)
def test_a_bit_flipped_from_0_to_2_is_unsatisfied(curve):
    b = BD.CircuitBuilder(curve)
    x = b.input()
    bits = b.to_bits(x, 8)
    built = b.build()
    ref, w = solved(built, [0b10110001])
    assert ref.unsatisfied_gates(w) == [] and w[bits[1]] == 0
    w[bits[1]] = 2
    bad = ref.unsatisfied_gates(w)
    assert int(built.def_gate[bits[1]]) in bad                           # y * y = y at the bit's own gate (and the recomposition after it)


@pytest.mark.parametrize("curve", CURVES)
def test_an_inverse_off_by_one_is_unsatisfied(curve):
    p = _fr.FIELDS[curve].p
    b = BD.CircuitBuilder(curve)
    x, a = b.input(2)
    y, q = b.inv(x), b.div(a, x)
    built = b.build()
    ref, w = solved(built, [7, 11])
    assert ref.unsatisfied_gates(w) == []
    for v in (y, q):
        t = list(w)
        t[v] = (t[v] + 1) % p
        assert ref.unsatisfied_gates(t) == [int(built.def_gate[v])]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k", [1, 4, 5, 64])
def test_range_check_of_two_to_the_k_is_unsatisfied(curve, k):
    b = BD.CircuitBuilder(curve)
    x = b.input()
    b.range_check(x, k)
    built = b.build()
    last = built.num_gates_unpadded - 1                                  # the recomposition's final gate: the constraint on x
    ref, w = solved(built, [1 << k])
    assert ref.unsatisfied_gates(w) == [last]
    assert ref.unsatisfied_gates(solved(built, [(1 << k) - 1])[1]) == []


@pytest.mark.parametrize("curve", CURVES)
def test_less_than_with_swapped_operands_is_unsatisfied(curve):
    """the result of less_than(a, b) pinned to 1; the same circuit with the operands' values swapped names the pinning gate"""
    b = BD.CircuitBuilder(curve)
    x, y = b.input(2)
    b.enforce_constant(b.less_than(x, y, 16), 1)
    built = b.build()
    pin = built.num_gates_unpadded - 1
    ref, w = solved(built, [1234, 40000])
    assert ref.unsatisfied_gates(w) == []
    ref, w = solved(built, [40000, 1234])
    assert ref.unsatisfied_gates(w) == [pin]
    ref, w = solved(built, [1234, 1234])
    assert ref.unsatisfied_gates(w) == [pin]


# ---------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("curve", CURVES)
def test_the_five_primitives_emit_the_documented_gate(curve):
    p = _fr.FIELDS[curve].p
    b = BD.CircuitBuilder(curve)
    x, a = b.input(2)
    before = b.num_gates
    outs = [b.inv(x), b.inv_or_zero(x), b.div(a, x), b.root5(x), b.bit(x, 77)]
    assert b.num_gates == before + 5                                     # one gate each
    built = b.build()
    ref = HintRefSolver(built, [1, 1])
    z = b.zero
    want = [([x, outs[0], x, z], {"q_mul0": 1, "q_c": p - 1}, BD.HINT_INV),
            ([z, z, x, z], {}, BD.HINT_INV),
            ([outs[2], x, a, x], {"q_mul0": 1, "q_lc2": p - 1}, BD.HINT_DIV),
            ([outs[3], z, x, z], {"q_hash0": 1, "q_lc2": p - 1}, BD.HINT_ROOT5),
            ([outs[4], outs[4], x, z], {"q_mul0": 1, "q_lc0": p - 1}, BD.HINT_BIT | 77 << 8)]
    for y, (wires, sel, op) in zip(outs, want):
        g = int(built.def_gate[y])
        assert [int(v) for v in built.wire_vars[:, g]] == wires + [y]
        assert selectors_at(ref, g) == sel                               # q_o = 0: wire 4 is free in the equation
        assert int(built.hint_op[g]) == op
    assert built.hint_op.dtype == np.uint32 and built.hint_op.shape == (built.n,)
    assert int(np.count_nonzero(built.hint_op)) == 5 and built.has_hints
    # bit with one index per element
    b = BD.CircuitBuilder(curve)
    xs = b.input(3)
    ys = b.bit(xs, [0, 200, 255])
    built = b.build()
    assert [int(h) for h in built.hint_op[built.def_gate[ys]]] == [4, 4 | 200 << 8, 4 | 255 << 8]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("nbits", [1, 2, 3, 4, 5, 7, 8, 64, 253])
def test_to_bits_stays_within_its_gate_bound(curve, nbits):
    b = BD.CircuitBuilder(curve)
    x = b.input(5)
    before = b.num_gates
    bits = b.to_bits(x, nbits)
    assert len(bits) == nbits and all(len(v) == 5 for v in bits)
    per_element = (b.num_gates - before) // 5
    assert (b.num_gates - before) % 5 == 0 and nbits < per_element <= nbits + -(-nbits // 3) + 1
    built = b.build()
    assert int(np.count_nonzero(built.hint_op)) == 5 * nbits


@pytest.mark.parametrize("curve", CURVES)
def test_a_circuit_without_hints_has_a_zero_hint_op_and_takes_the_old_entry(curve):
    b = BD.CircuitBuilder(curve)
    x, y = b.input(2)
    out = b.public_input()
    b.enforce_equal(b.mul(b.pow5_lc([x, y], [1, 3], const=7), y), out)
    built = b.build()
    assert built.hint_op.shape == (built.n,) and not built.hint_op.any() and not built.has_hints

    class Recorder:
        """stands in for a worker: records which solver entry solve_dev calls"""
        curve_name = curve

        class Buf:
            ptr = 1

            def upload(self, a):
                return self

            def free(self):
                pass

        def __init__(self):
            self.calls = []

        def alloc(self, nbytes):
            return self.Buf()

        def memset_dev(self, *a):
            pass

        def circuit_solve_dev(self, *a):
            self.calls.append(("plain", len(a)))
            return -1, 0, 0

        def circuit_solve_hints_dev(self, *a):
            self.calls.append(("hints", len(a)))
            return -1, 0, 0

    rec = Recorder()
    built.solve_dev(rec, np.zeros((2, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)).close()
    assert rec.calls == [("plain", 7)]
    # positional construction without hint_op, as before hints existed
    again = BD.BuiltCircuit(built.curve, built.wire_vars, built.selector_evals, built.num_vars, built.def_gate, built.input_vars, built.public_vars,
                            built.zero_var, built.num_gates_unpadded)
    assert not again.has_hints and again.hint_op.shape == (built.n,)
    # one hint is enough for the new entry
    b2 = BD.CircuitBuilder(curve)
    b2.inv(b2.input())
    rec = Recorder()
    b2.build().solve_dev(rec, np.zeros((1, 4), dtype=np.uint64)).close()
    assert rec.calls == [("hints", 8)]


# ---------------------------------------------------------------------------------------------- refused calls
@pytest.mark.parametrize("curve", CURVES)
def test_refused_calls_raise_value_error_and_emit_nothing(curve):
    bl = _fr.FIELDS[curve].p.bit_length()
    b = BD.CircuitBuilder(curve)
    x, y3 = b.input(2), b.input(3)
    s = int(x[0])
    unknown = b.num_vars
    refused = [lambda: b.to_bits(s, 0), lambda: b.to_bits(s, bl), lambda: b.to_bits(s, -1), lambda: b.to_bits(s, 2.0),
               lambda: b.range_check(s, bl), lambda: b.range_check(s, 0),
               lambda: b.less_than(s, s, bl - 1), lambda: b.less_than(s, s, 0),
               lambda: b.bit(s, 256), lambda: b.bit(s, -1), lambda: b.bit(x, [0, 256]), lambda: b.bit(s, 1.5),
               lambda: b.bit(x, [1, 2, 3]), lambda: b.div(x, y3), lambda: b.select(x, y3, s), lambda: b.is_equal(x, y3), lambda: b.less_than(x, y3, 8),
               lambda: b.inv(unknown), lambda: b.inv_or_zero(-1), lambda: b.div(s, unknown), lambda: b.root5([s, unknown]), lambda: b.bit(unknown, 0),
               lambda: b.to_bits(unknown, 8), lambda: b.range_check(unknown, 8), lambda: b.is_zero(unknown), lambda: b.is_equal(s, unknown),
               lambda: b.select(s, s, unknown), lambda: b.less_than(unknown, s, 8), lambda: b.less_than(s, unknown, 8)]
    gates, variables = b.num_gates, b.num_vars
    for i, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        assert (b.num_gates, b.num_vars) == (gates, variables), i
    assert b.to_bits(s, bl - 1) is not None and b.less_than(s, s, bl - 2) is not None          # the widest accepted
