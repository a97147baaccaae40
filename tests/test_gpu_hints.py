"""Hinted definitions on the device (plonk_circuit_solve_hints_dev behind builder.BuiltCircuit.solve_dev) against tests/hint_ref.py, the
sequential big-integer solver with Python's pow for the hints: bit-for-bit witnesses and equal level / evaluation counters on random
layered circuits that mix every old builder operation with every new one, the frontier shapes at which the per-class lists can go wrong
(one pow hint beside a thousand gates and the reverse, pow levels around the wave and workgroup sizes, BIT-only levels, pow feeding pow,
hints at level 0, a DIV whose sources arrive in different levels or are one variable, a pow5 / root5 alternation), BIT at its edge
arguments, cycles through a hint gate, validation errors, hint_op = NULL, determinism, and a circuit of div, is_zero, select,
range_check, less_than and root5 built, solved, preprocessed, proved and verified.

tests/test_hostemu_hints.py runs a selection of this file on the CPU."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.transcript import PlonkTranscript
from tests.circuit_cases import random_layered, random_layered_hints
from tests.hint_ref import GIVEN, HintRefSolver
from tests.test_gpu_solve import TAU, trapdoor_key

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]


# ---------------------------------------------------------------------------------------------- helpers
def solve_and_compare(w, built, inputs, publics=()):
    """the device witness against the reference, bit for bit, and the counters; -> (device witness, reference)"""
    ref = HintRefSolver(built, inputs, publics)
    want, _ = ref.solve()
    s = built.solve_dev(w, ref.limbs(inputs), ref.limbs(publics))
    try:
        got = s.witness()
        assert np.array_equal(got, ref.limbs(want))
        assert s.levels == ref.depth()
        assert s.evaluations == int((built.def_gate != GIVEN).sum())
    finally:
        s.close()
        built.close()
    return got, ref


def rebuilt(built, wire_vars=None, selector_evals=None, def_gate=None, hint_op=None):
    """a copy of a BuiltCircuit with some arrays replaced"""
    pick = lambda new, old: old.copy() if new is None else new
    return BD.BuiltCircuit(built.curve, pick(wire_vars, built.wire_vars), pick(selector_evals, built.selector_evals), built.num_vars,
                           pick(def_gate, built.def_gate), built.input_vars, built.public_vars, built.zero_var, built.num_gates_unpadded,
                           hint_op=pick(hint_op, built.hint_op))


def raw_solve(w, built, inputs=None, hint_op="own", entry="hints", wire_vars=None):
    """The C entry on a BuiltCircuit's arrays.  hint_op: "own", None (NULL) or an array; entry: "hints" or "plain".
    -> (witness bytes, unsolved, levels, evaluations)"""
    f = _fr.FIELDS[built.curve]
    witness = np.zeros((built.num_vars, 4), dtype=np.uint64)
    if inputs is not None:
        witness[built.input_vars] = np.array([f.to_limbs(int(v) % f.p) for v in inputs], dtype=np.uint64).reshape(-1, 4)
    hint = built.hint_op if isinstance(hint_op, str) else hint_op
    arrs = [built.wire_vars if wire_vars is None else wire_vars, built.selector_evals, built.def_gate, witness] + ([] if hint is None else [hint])
    bufs = [w.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for a in arrs] + [w.alloc(built.n * 32)]
    try:
        w.memset_dev(bufs[-1].ptr, 0, built.n * 32)
        if entry == "plain":
            out = w.circuit_solve_dev(bufs[0].ptr, built.n, built.num_vars, bufs[1].ptr, bufs[-1].ptr, bufs[2].ptr, bufs[3].ptr)
        else:
            out = w.circuit_solve_hints_dev(bufs[0].ptr, built.n, built.num_vars, bufs[1].ptr, bufs[-1].ptr, bufs[2].ptr,
                                            0 if hint is None else bufs[4].ptr, bufs[3].ptr)
        return (bufs[3].download((built.num_vars, 4)).tobytes(),) + tuple(out)
    finally:
        for x in bufs:
            x.free()


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_n", [3, 5, 8, 12], ids=lambda v: f"log{v}")
def test_random_layered_circuits_with_hints_match_the_reference(gpu_workers, curve, cid, log_n):
    built, inputs, publics = random_layered_hints(curve, log_n, 2000 * log_n + cid)
    assert built.has_hints
    solve_and_compare(gpu_workers(curve), built, inputs, publics)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_frontier_one_pow_hint_beside_a_thousand_gates_and_the_reverse(gpu_workers, curve, cid):
    p = _fr.FIELDS[curve].p
    rnd = random.Random(40 + cid)
    b = BD.CircuitBuilder(curve)
    x = b.input(1000)
    t = b.add(x, x)                                         # level 0
    sq = b.mul(t, t)                                        # level 1: 1000 gates ...
    lone = b.inv(int(t[0]))                                 # ... and 1 pow hint
    roots = b.root5(sq)                                     # level 2: 1000 pow hints ...
    b.mul(lone, lone)                                       # ... and 1 gate
    b.add(roots, lone)                                      # level 3
    _, ref = solve_and_compare(gpu_workers(curve), b.build(), [rnd.randrange(p) for _ in range(1000)])
    assert ref.depth() == 4


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257])
def test_frontier_pow_levels_around_the_wave_and_workgroup_sizes(gpu_workers, curve, cid, count):
    """levels of exactly `count` hints of one class, of both classes at once, and a pow hint feeding a pow hint of the next level"""
    p = _fr.FIELDS[curve].p
    rnd = random.Random(count + cid)
    b = BD.CircuitBuilder(curve)
    x = b.input(count)
    t = b.add(x, b.one)                                     # level 1 (`one` is a constant gate of level 0)
    u = b.inv(t)                                            # level 2: count hints of exponent r - 2
    v = b.root5(u)                                          # level 3: count of exponent d, each fed by a pow hint
    b.root5(t)                                              # level 2 too: both pow classes in one level
    q = b.div(v, t)                                         # level 4
    b.mul(q, u)
    inputs = [rnd.randrange(p) for _ in range(count)]
    inputs[0], inputs[-1] = p - 1, 0                        # t = 0 (inverse 0, quotient 0), t = 1
    got, ref = solve_and_compare(gpu_workers(curve), b.build(), inputs)
    f = _fr.FIELDS[curve]
    assert ref.depth() == 6 and f.from_limbs(got[int(u[0])]) == 0 and f.from_limbs(got[int(q[0])]) == 0 and f.from_limbs(got[int(q[-1])]) == 1


@pytest.mark.parametrize("curve,cid", CURVES)
def test_frontier_bit_only_level_level0_hints_and_div_sources(gpu_workers, curve, cid):
    p = _fr.FIELDS[curve].p
    rnd = random.Random(60 + cid)
    b = BD.CircuitBuilder(curve)
    x, y = b.input(70), b.input(70)
    # hints whose sources are all given: level 0
    i0, d0, r0, b0 = b.inv(x), b.div(x, y), b.root5(y), b.bit(x, 3)
    t = b.add(x, y)                                         # level 0
    bits = [b.bit(t, k) for k in (0, 1, 100)]               # level 1 holds BIT hints only
    c = b.mul(bits[0], t)                                   # level 2
    dq = b.div(t, c)                                        # sources ready after levels 0 and 2 -> level 3
    dr = b.div(c, t)                                        # the same the other way round
    same = b.div(c, c)                                      # both sources one variable: 1, or 0 for c = 0
    b.lc([dq, dr, same, i0], [1, 2, 3, 4])                  # level 4, as the next two: level 1 stays with the BIT hints
    b.lc([d0, r0, b0, dq], [1, 1, 1, 1])
    b.add(bits[2], dq)
    xs = [rnd.randrange(p) for _ in range(70)]
    ys = [rnd.randrange(p) for _ in range(70)]
    xs[0], ys[0] = 5, p - 5                                 # t = 0
    xs[1], ys[1] = 0, 0
    xs[2], ys[2] = 4, 3                                     # t = 7: odd, c = 7
    built = b.build()
    got, ref = solve_and_compare(gpu_workers(curve), built, xs + ys)
    f = _fr.FIELDS[curve]
    assert [f.from_limbs(got[int(v)]) for v in same[:3]] == [0, 0, 1]
    assert ref.lvl[int(i0[0])] == 0 and ref.lvl[int(d0[0])] == 0 and ref.lvl[int(r0[0])] == 0 and ref.lvl[int(b0[0])] == 0
    assert ref.lvl[int(dq[0])] == 3 and ref.lvl[int(dr[0])] == 3 and ref.lvl[int(same[0])] == 3
    level1 = [v for v in range(built.num_vars) if ref.lvl[v] == 1]
    assert len(level1) == 3 * 70 and all(ref.opcode(int(built.def_gate[v])) == BD.HINT_BIT for v in level1)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_frontier_pow5_root5_alternation_on_parallel_chains(gpu_workers, curve, cid):
    p = _fr.FIELDS[curve].p
    rnd = random.Random(70 + cid)
    depth, chains = 64, 128
    b = BD.CircuitBuilder(curve)
    x = b.input(chains)
    for t in range(depth):
        x = b.pow5_lc([x], [1], const=rnd.randrange(p)) if t % 2 == 0 else b.root5(x)
    _, ref = solve_and_compare(gpu_workers(curve), b.build(), [rnd.randrange(p) for _ in range(chains)])
    assert ref.depth() == depth


@pytest.mark.parametrize("curve,cid", CURVES)
def test_bit_at_its_edge_arguments_and_values(gpu_workers, curve, cid):
    f = _fr.FIELDS[curve]
    p, bl = f.p, f.p.bit_length()
    values = [p - 1, 0, 1] + [1 << k for k in (0, 31, 32, 63, 64, 200, bl - 2, bl - 1)] + [(1 << k) - 1 for k in (1, 32, 33, 64, 65, bl - 1)]
    args = sorted({0, 1, 31, 32, 33, 63, 64, 127, 128, bl - 2, bl - 1, bl, min(bl + 1, 255), 254, 255})     # bl is 254 or 255
    b = BD.CircuitBuilder(curve)
    x = b.input(len(values))
    outs = [b.bit(x, k) for k in args]
    each = b.bit(x, np.arange(len(values)) * 13 % 256)      # one argument per element
    got, _ = solve_and_compare(gpu_workers(curve), b.build(), values)
    for k, ys in zip(args, outs):
        assert [f.from_limbs(got[int(y)]) for y in ys] == [(v >> k) & 1 for v in values], k
    assert all(f.from_limbs(got[int(y)]) == 0 for k, ys in zip(args, outs) if k >= bl for y in ys)
    assert [f.from_limbs(got[int(y)]) for y in each] == [(v >> (i * 13 % 256)) & 1 for i, v in enumerate(values)]


# ---------------------------------------------------------------------------------------------- cycles and validation
def hinted_small(curve: str):
    b = BD.CircuitBuilder(curve)
    a = b.input()
    x = b.add(a, a)
    y = b.inv(x)
    z = b.mul(y, y)
    k = b.bit(z, 2)
    b.enforce_equal(z, z)
    return b.build(), (a, x, y, z, k)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_a_cycle_through_a_hint_gate_is_reported_with_its_smallest_variable(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, (a, x, y, z, k) = hinted_small(curve)
    # as built, the inv gate reads y on wire 1 and the bit gate reads k on wires 0 and 1: dead for scheduling, no cycle
    assert int(built.wire_vars[1, built.def_gate[y]]) == y and int(built.wire_vars[0, built.def_gate[k]]) == k
    got, ref = solve_and_compare(w, built, [3])
    assert _fr.FIELDS[curve].from_limbs(got[y]) == pow(6, -1, ref.f.p)
    wv = built.wire_vars.copy()
    wv[0, int(built.def_gate[x])] = z                       # x = z + a, y = 1 / x, z = y * y
    cyc = rebuilt(built, wire_vars=wv)
    _, unsolved, levels, evaluations = raw_solve(w, cyc, [3])
    assert unsolved == x and x < y < z
    assert evaluations == 2 and levels == 1                 # the zero and one gates; x, y, z and k (downstream) stay
    with pytest.raises(CI.UnsolvableCircuit) as e:
        cyc.solve_dev(w, np.zeros((1, 4), dtype=np.uint64))
    assert e.value.variable == x and f"variable {x}" in str(e.value)
    cyc.close()
    # a hint gate whose SOURCE wire reads its own output is the shortest cycle
    wv = built.wire_vars.copy()
    wv[2, int(built.def_gate[y])] = y
    assert raw_solve(w, rebuilt(built, wire_vars=wv), [3])[1] == y


@pytest.mark.parametrize("curve,cid", CURVES)
def test_invalid_hints_are_reported_and_the_worker_recovers(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, (a, x, y, z, k) = hinted_small(curve)
    gy, gk, gx = int(built.def_gate[y]), int(built.def_gate[k]), int(built.def_gate[x])
    constraint = built.num_gates_unpadded - 1               # the enforce_equal gate: defines nothing

    def fails(mentions, **kw):
        with pytest.raises(PlonkError) as e:
            raw_solve(w, built, [3], **kw)
        assert e.value.code == -1, str(e.value)
        for m in mentions:
            assert m in str(e.value), str(e.value)

    def with_hint(g, value):
        h = built.hint_op.copy()
        h[g] = value
        return h

    fails([f"variable {y}", f"gate {gy}", "opcode"], hint_op=with_hint(gy, 5))
    fails([f"variable {y}", f"gate {gy}", "opcode"], hint_op=with_hint(gy, 255))
    fails([f"variable {x}", f"gate {gx}", "opcode"], hint_op=with_hint(gx, 0x100))          # an argument without an opcode
    fails([f"variable {k}", f"gate {gk}", "argument"], hint_op=with_hint(gk, 4 | 256 << 8))
    fails([f"gate {constraint}", "defines no variable"], hint_op=with_hint(constraint, 1))
    fails([f"gate {built.n - 1}", "defines no variable"], hint_op=with_hint(built.n - 1, 4))  # a padding gate
    # a hint gate has q_o = 0: fine for the new entry, refused by the old one as ever
    assert raw_solve(w, built, [3])[1] == -1
    fails([f"variable {y}", f"gate {gy}", "q_o", "plonk_circuit_solve_dev"], entry="plain")
    # an ordinary gate with q_o = 0 is still refused by the new entry
    sel = built.selector_evals.copy()
    sel[10, gx] = 0
    with pytest.raises(PlonkError) as e:
        raw_solve(w, rebuilt(built, selector_evals=sel), [3])
    assert e.value.code == -1 and f"variable {x}" in str(e.value) and "q_o" in str(e.value)
    # the worker still solves a good circuit
    solve_and_compare(w, built, [3])


@pytest.mark.parametrize("curve,cid", CURVES)
def test_null_hint_op_is_the_old_entry(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, inputs, publics = random_layered(curve, 8, 91 + cid)
    assert not built.has_hints
    f = _fr.FIELDS[curve]
    pub = np.zeros((built.n, 4), dtype=np.uint64)
    pub[0] = f.to_limbs(publics[0])

    def run(entry, hint_op):
        witness = np.zeros((built.num_vars, 4), dtype=np.uint64)
        witness[built.input_vars] = np.array([f.to_limbs(v) for v in inputs], dtype=np.uint64).reshape(-1, 4)
        arrs = [built.wire_vars, built.selector_evals, built.def_gate, witness, pub] + ([] if hint_op is None else [hint_op])
        bufs = [w.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for a in arrs]
        try:
            args = [bufs[0].ptr, built.n, built.num_vars, bufs[1].ptr, bufs[4].ptr, bufs[2].ptr]
            if entry == "plain":
                out = w.circuit_solve_dev(*args, bufs[3].ptr)
            else:
                out = w.circuit_solve_hints_dev(*args, 0 if hint_op is None else bufs[5].ptr, bufs[3].ptr)
            return bufs[3].download((built.num_vars, 4)).tobytes(), tuple(out)
        finally:
            for x in bufs:
                x.free()

    old = run("plain", None)
    assert old[1][0] == -1 and old[1][2] == int((built.def_gate != GIVEN).sum())
    assert run("hints", None) == old
    assert run("hints", built.hint_op) == old               # an all-zero array: the hinted kernels on a circuit without hints


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_runs_with_hints_give_identical_bytes(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, inputs, publics = random_layered_hints(curve, 12, 57 + cid)
    ref = HintRefSolver(built, inputs, publics)
    outs = []
    for _ in range(2):
        s = built.solve_dev(w, ref.limbs(inputs), ref.limbs(publics))
        outs.append((s.witness().tobytes(), s.levels, s.evaluations))
        s.close()
    built.close()
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------- end to end
NBITS = 8


def ledger_circuit(curve: str, m: int, seed: int):
    """m rows (a, b) of NBITS-bit values: q = a / b, e = (a == b), lt = (a < b), lo = lt ? a : b, r = lo^(1/5) checked again by a
    forward pow5 gate, and the public input is sum q r + e lo.  -> (BuiltCircuit, input residues, the public value)"""
    p = _fr.FIELDS[curve].p
    rnd = random.Random(seed)
    b = BD.CircuitBuilder(curve)
    total = b.public_input()
    a, c = b.input(m), b.input(m)
    b.range_check(a, NBITS)
    q = b.div(a, c)
    e = b.is_equal(a, c)                                    # is_zero of the difference
    lt = b.less_than(a, c, NBITS)
    lo = b.select(lt, a, c)
    r = b.root5(lo)
    b.enforce_equal(b.pow5_lc([r], [1]), lo)
    t = b.mul_add(q, r, e, lo)
    acc = int(t[0])
    for i in range(1, m):
        acc = b.add(acc, int(t[i]))
    b.enforce_equal(acc, total)
    av = [rnd.randrange(1 << NBITS) for _ in range(m)]
    cv = [rnd.randrange(1, 1 << NBITS) for _ in range(m)]
    av[0], cv[0] = 0, 255
    if m > 1:
        av[1] = cv[1]
    d = pow(5, -1, p - 1)
    value = sum(x * pow(y, -1, p) * pow(min(x, y), d, p) + (x == y) * min(x, y) for x, y in zip(av, cv)) % p
    return b.build(), av + cv, value


@pytest.mark.parametrize("log_n,m", [(8, 3), (10, 14)], ids=["log8", "log10"])
def test_hinted_circuit_is_built_solved_proved_and_verified(gpu_workers, oracle, log_n, m):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    curve, cid = "bn254", 0
    w = gpu_workers(curve)
    n = 1 << log_n
    built, inputs, value = ledger_circuit(curve, m, seed=log_n)
    assert built.n == n and built.has_hints
    ref = HintRefSolver(built, inputs, [value])
    assert ref.unsatisfied_gates(ref.solve()[0]) == []
    inst = built.preprocess(w, ref.limbs(inputs), ref.limbs([value]), check=True)
    ck = trapdoor_key(w, n)
    pv = Prover(w, log_n)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        assert np.array_equal(pub, ref.limbs([value]))
        blinders = dict(wires=oracle.rand_fr(cid, 92, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 93, 3))
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
        V.verify(B.CURVES[curve], vk, pub, proof, TAU, transcript=PlonkTranscript(curve))
    finally:
        pv.close()
        inst.close()
        ck.free()
    # an input beyond its range check: the solver still fills the witness, the check refuses it
    wrong = list(inputs)
    wrong[m - 1] = 1 << NBITS
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, ref.limbs(wrong), ref.limbs([value]), check=True).close()
    built.close()
    w.trim()
