"""distributed_plonk_amd/builder.py on the host (no GPU): every operation's gate row against hand-written selectors and wires, the
layout build() promises (IO gates first, def_gate consistent with wire 4, a power of two with jellyfish's padding gates),
broadcasting, the constant cache, argument errors, and the hand-written chain circuit of tests/test_gpu_circuit.py rebuilt through the
builder — both solved by tests/solve_ref.py."""
import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import fr as _fr
from tests.solve_ref import GIVEN, RefSolver

CURVES = ["bn254", "bls12_381"]
NAMES = ["q_lc0", "q_lc1", "q_lc2", "q_lc3", "q_mul0", "q_mul1", "q_hash0", "q_hash1", "q_hash2", "q_hash3", "q_o", "q_c", "q_ecc"]


def row(built, g):
    """gate g as (wires tuple, {selector name: plain residue} of the non-zero selectors)"""
    f = _fr.FIELDS[built.curve]
    sel = {NAMES[t]: f.from_limbs(built.selector_evals[t, g]) for t in range(13)}
    return tuple(int(v) for v in built.wire_vars[:, g]), {k: v for k, v in sel.items() if v}


@pytest.mark.parametrize("curve", CURVES)
def test_every_operation_emits_the_hand_written_gate(curve):
    p = _fr.FIELDS[curve].p
    b = BD.CircuitBuilder(curve)
    z = b.zero
    assert (b.zero, b.one) == (0, 1)
    pi = b.public_input()
    a, c, d, e = b.input(4)
    v_add, v_sub, v_mul = b.add(a, c), b.sub(a, c), b.mul(a, c)
    v_lc = b.lc([a, c, d], [2, -3, 5], const=7)
    v_ma = b.mul_add(a, c, d, e, q0=11, q1=-1)
    v_ma1 = b.mul_add(a, c, d, e)
    v_p5 = b.pow5_lc([a, c, d, e], [1, 2, 3, 4], const=-9)
    v_gate = b.gate([a, c, d, e], {"q_lc1": 4, "q_mul1": 6, "q_hash2": 8, "q_o": -2, "q_c": 1})
    v_const = b.constant(42)
    assert b.gate([a, c, d, e], {"q_lc0": 1, "q_o": 3}, out=v_add) is None
    b.enforce_equal(a, c)
    b.enforce_constant(d, 13)
    b.enforce_bool(e)
    b.enforce_mul(a, c, d)
    built = b.build()
    assert built.num_public == 1 and list(built.public_vars) == [pi] and list(built.input_vars) == [a, c, d, e]
    assert row(built, 0) == ((z, z, z, z, pi), {"q_o": 1})                         # the IO gate comes first
    g = {v: int(built.def_gate[v]) for v in range(built.num_vars) if built.def_gate[v] != GIVEN}
    assert all(built.def_gate[v] == GIVEN for v in (a, c, d, e))
    assert row(built, g[b.zero]) == ((0, 0, 0, 0, 0), {"q_o": 1})
    assert row(built, g[b.one]) == ((z, z, z, z, 1), {"q_o": 1, "q_c": 1})
    assert row(built, g[v_add]) == ((a, c, z, z, v_add), {"q_lc0": 1, "q_lc1": 1, "q_o": 1})
    assert row(built, g[v_sub]) == ((a, c, z, z, v_sub), {"q_lc0": 1, "q_lc1": p - 1, "q_o": 1})
    assert row(built, g[v_mul]) == ((a, c, z, z, v_mul), {"q_mul0": 1, "q_o": 1})
    assert row(built, g[v_lc]) == ((a, c, d, z, v_lc), {"q_lc0": 2, "q_lc1": p - 3, "q_lc2": 5, "q_c": 7, "q_o": 1})
    assert row(built, g[v_ma]) == ((a, c, d, e, v_ma), {"q_mul0": 11, "q_mul1": p - 1, "q_o": 1})
    assert row(built, g[v_ma1]) == ((a, c, d, e, v_ma1), {"q_mul0": 1, "q_mul1": 1, "q_o": 1})
    assert row(built, g[v_p5]) == ((a, c, d, e, v_p5), {"q_hash0": 1, "q_hash1": 2, "q_hash2": 3, "q_hash3": 4, "q_c": p - 9, "q_o": 1})
    assert row(built, g[v_gate]) == ((a, c, d, e, v_gate), {"q_lc1": 4, "q_mul1": 6, "q_hash2": 8, "q_o": p - 2, "q_c": 1})
    assert row(built, g[v_const]) == ((z, z, z, z, v_const), {"q_c": 42, "q_o": 1})
    last = g[v_const]
    assert row(built, last + 1) == ((a, c, d, e, v_add), {"q_lc0": 1, "q_o": 3})
    assert row(built, last + 2) == ((a, c, z, z, z), {"q_lc0": 1, "q_lc1": p - 1})
    assert row(built, last + 3) == ((z, z, z, z, d), {"q_c": 13, "q_o": 1})
    assert row(built, last + 4) == ((e, e, z, z, e), {"q_mul0": 1, "q_o": 1})
    assert row(built, last + 5) == ((a, c, z, z, d), {"q_mul0": 1, "q_o": 1})
    assert built.num_gates_unpadded == last + 6 and b.num_gates == last + 6
    # the defining gates give the values the operations mean; the constraints hold exactly when they should
    va, vc, ve = 3, 4, 1
    ref = RefSolver(built, [va, vc, va * vc, ve], [99])
    wit, _ = ref.solve()
    assert [wit[v] for v in (pi, v_add, v_sub, v_mul, v_const)] == [99, 7, p - 1, 12, 42]
    assert wit[v_lc] == (2 * va - 3 * vc + 5 * 12 + 7) % p and wit[v_ma] == (11 * 12 - 12 * ve) % p
    assert wit[v_p5] == (va ** 5 + 2 * vc ** 5 + 3 * 12 ** 5 + 4 * ve ** 5 - 9) % p
    assert wit[v_gate] == (4 * vc + 6 * 12 * ve + 8 * 12 ** 5 + 1) * pow(p - 2, -1, p) % p
    # gate(out=) asks a = 3 (a + c); enforce_equal a = c; enforce_constant d = 13: not so for these inputs.  enforce_bool(e), enforce_mul hold
    assert ref.unsatisfied_gates(wit) == [last + 1, last + 2, last + 3]


@pytest.mark.parametrize("curve", CURVES)
def test_layout_io_first_def_gate_padding(curve):
    b = BD.CircuitBuilder(curve)
    x = b.input(5)
    y = b.mul(x, x)
    p1 = b.public_input()
    t = b.add(y, p1)
    p2 = b.public_input(2)                                   # requested after other gates, placed first all the same
    b.enforce_equal(t, p2[0])
    built = b.build()
    assert built.num_public == 3 and list(built.public_vars) == [p1, p2[0], p2[1]]
    assert [int(v) for v in built.wire_vars[4, :3]] == [p1, p2[0], p2[1]]
    assert [int(built.def_gate[v]) for v in built.public_vars] == [0, 1, 2]
    n, g = built.n, built.num_gates_unpadded
    assert g == 3 + 2 + 5 + 5 + 5 and n == 32 and n & (n - 1) == 0
    assert not built.selector_evals[:, g:].any() and (built.wire_vars[:, g:] == built.zero_var).all()      # jellyfish's padding gates
    assert built.wire_vars.dtype == np.uint32 and built.def_gate.dtype == np.uint32 and built.selector_evals.shape == (13, n, 4)
    defined = np.flatnonzero(built.def_gate != GIVEN)
    assert np.array_equal(built.wire_vars[4, built.def_gate[defined].astype(np.int64)], defined.astype(np.uint32))
    assert len(set(built.def_gate[defined].tolist())) == len(defined)
    assert sorted(np.flatnonzero(built.def_gate == GIVEN).tolist()) == sorted(int(v) for v in x)
    assert BD.CircuitBuilder(curve).build().n == 2                                 # the zero and one gates alone


@pytest.mark.parametrize("curve", CURVES)
def test_broadcasting_and_the_constant_cache(curve):
    p = _fr.FIELDS[curve].p
    b = BD.CircuitBuilder(curve)
    xs = b.input(4)
    s = b.input()
    assert isinstance(s, int) and xs.shape == (4,)
    out = b.mul(xs, s)                                       # an array against a scalar
    assert out.shape == (4,) and isinstance(b.add(s, s), int)
    lin = b.lc([xs, s], [[1, 2, 3, 4], 10], const=[5, 6, 7, 8])      # per-gate coefficients against shared ones
    one_elem = b.add(xs, np.array([s]))                      # a length-1 array broadcasts too
    assert one_elem.shape == (4,)
    n_before = b.num_gates
    c1, c2, c3 = b.constant(5), b.constant(5 + p), b.constant(6)
    assert c1 == c2 != c3 and b.num_gates == n_before + 2 and b.constant(0) == b.zero and b.constant(1) == b.one
    built = b.build()
    vals = [2, 3, 5, 7]
    wit, lvl = RefSolver(built, vals + [11]).solve()
    assert [wit[v] for v in out] == [22, 33, 55, 77]
    assert [wit[v] for v in lin] == [(k + 1) * vals[k] + 110 + 5 + k for k in range(4)]
    assert [wit[v] for v in one_elem] == [v + 11 for v in vals]
    assert lvl[int(xs[0])] == -1 and lvl[int(out[0])] == 0


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors(curve):
    b = BD.CircuitBuilder(curve)
    x = b.input(3)
    y = b.input(2)
    with pytest.raises(ValueError, match="unknown variable id"):
        b.add(x, b.num_vars)
    with pytest.raises(ValueError, match="unknown variable id"):
        b.mul(-1, x)
    with pytest.raises(ValueError, match="at most 4"):
        b.lc([x] * 5, [1] * 5)
    with pytest.raises(ValueError, match="at most 4"):
        b.pow5_lc([x] * 5, [1] * 5)
    with pytest.raises(ValueError, match="mismatched lengths"):
        b.lc([x, x], [1])
    with pytest.raises(ValueError, match="mismatched lengths"):
        b.add(x, y)
    with pytest.raises(ValueError, match="mismatched lengths"):
        b.lc([x], [[1, 2]])
    with pytest.raises(ValueError, match="unknown selector"):
        b.gate([x, x, x, x], {"q_ecc": 1})
    with pytest.raises(ValueError, match="q_o != 0"):
        b.gate([x, x, x, x], {"q_lc0": 1, "q_o": 0})
    with pytest.raises(ValueError, match="4"):
        b.gate([x, x, x], {"q_lc0": 1})
    with pytest.raises(ValueError, match="integers"):
        b.add(x, np.array([0.5, 1.0, 2.0]))
    gates, nvars = b.num_gates, b.num_vars
    assert (gates, nvars) == (2, 7)                          # a refused call emits nothing
    built = b.build()
    with pytest.raises(ValueError, match="input values"):
        built.solve_dev(type("W", (), {"curve_name": curve})(), np.zeros((4, 4), dtype=np.uint64))
    with pytest.raises(ValueError, match="worker over"):
        built.solve_dev(type("W", (), {"curve_name": "other"})(), np.zeros((5, 4), dtype=np.uint64))


@pytest.mark.parametrize("curve", CURVES)
def test_the_hand_written_chain_circuit_rebuilt_through_the_builder(curve):
    """tests/test_gpu_circuit.py's _chain_circuit — gates out_t = x_t^5 + x_t y_t + c_t, two IO gates carrying the last and the middle output —
    written there as raw selector columns with a host-computed witness; here the builder emits it and solve_ref finds the same values."""
    p = _fr.FIELDS[curve].p
    rs = np.random.RandomState(10)
    T, num_io = 27, 2
    ys = [int(v) for v in rs.randint(1, 1 << 62, size=T)]
    cs = [int(v) for v in rs.randint(0, 1 << 62, size=T)]
    x0 = int(rs.randint(1, 1 << 62))
    # by hand, as the GPU test writes it: variables 0 zero, 1 x_0, 2 + 2t y_t, 3 + 2t out_t
    vals, x = [0, x0], x0
    for t in range(T):
        x = (pow(x, 5, p) + x * ys[t] + cs[t]) % p
        vals += [ys[t], x]
    pub_vars = [3 + 2 * (T - 1), 3 + 2 * (T // 2)]
    hand_wv = np.zeros((5, num_io + T), dtype=np.int64)
    hand_sel = [dict() for _ in range(num_io + T)]
    for j in range(num_io):
        hand_wv[4, j] = pub_vars[j]
        hand_sel[j] = {"q_o": 1}
    for t in range(T):
        j = num_io + t
        hand_wv[:, j] = [1 if t == 0 else 3 + 2 * (t - 1), 2 + 2 * t, 0, 0, 3 + 2 * t]
        hand_sel[j] = {"q_hash0": 1, "q_mul0": 1, "q_o": 1, **({"q_c": cs[t]} if cs[t] else {})}
    # through the builder: the outputs are defined by their gates, the two public outputs tied to them by equality
    b = BD.CircuitBuilder(curve)
    bx = b.input()
    by = b.input(T)
    pubs = b.public_input(2)
    outs = []
    for t in range(T):
        bx = b.gate([bx, by[t], b.zero, b.zero], {"q_hash0": 1, "q_mul0": 1, "q_c": cs[t]})
        outs.append(bx)
    b.enforce_equal(outs[T - 1], pubs[0])
    b.enforce_equal(outs[T // 2], pubs[1])
    built = b.build()
    # same gates up to variable numbering: map the builder's ids to the hand-written ones
    to_hand = {b.zero: 0, int(built.input_vars[0]): 1, **{int(by[t]): 2 + 2 * t for t in range(T)}, **{outs[t]: 3 + 2 * t for t in range(T)}}
    for t in range(T):
        wires, sel = row(built, int(built.def_gate[outs[t]]))
        assert tuple(to_hand[v] for v in wires) == tuple(hand_wv[:, num_io + t]) and sel == hand_sel[num_io + t]
    for j in range(num_io):
        assert row(built, j)[1] == hand_sel[j]
    ref = RefSolver(built, [x0] + ys, [vals[v] for v in pub_vars])
    wit, lvl = ref.solve()
    assert [wit[outs[t]] for t in range(T)] == [vals[3 + 2 * t] for t in range(T)]
    assert ref.unsatisfied_gates(wit) == [] and ref.depth() == T
    # the hand-written witness satisfies the hand-written gates under the same reference equation
    for j in range(num_io + T):
        q = {name: 0 for name in NAMES}
        q.update(hand_sel[j])
        w = [vals[v] for v in hand_wv[:, j]]
        pi = vals[pub_vars[j]] if j < num_io else 0
        assert (q["q_c"] + pi + q["q_hash0"] * pow(w[0], 5, p) + q["q_mul0"] * w[0] * w[1] - q["q_o"] * w[4]) % p == 0
    # a wrong public output is caught at its equality gate
    bad = RefSolver(built, [x0] + ys, [vals[pub_vars[0]] + 1, vals[pub_vars[1]]])
    assert bad.unsatisfied_gates(bad.solve()[0]) == [built.num_gates_unpadded - 2]
