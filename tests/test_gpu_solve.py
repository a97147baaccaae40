"""The witness solver on the device (plonk_circuit_solve_dev behind builder.BuiltCircuit.solve_dev) against tests/solve_ref.py, a
sequential big-integer solver written from the gate equation: random layered circuits mixing every builder operation, the scheduling
shapes (a chain, independent gates, definitions after uses, one variable on two live wires, a dead wire on the gate's own output),
cycles and invalid arguments, run-to-run determinism, a membership circuit built, solved, preprocessed, proved and verified, and
a 2^22-gate circuit of parallel hash chains checked by the satisfiability kernel (which shares no code path with the level loop).

tests/test_hostemu_solve.py runs a selection of this file on the CPU."""
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
from tests.circuit_cases import random_layered
from tests.solve_ref import GIVEN, RefSolver

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3
CHAIN = 1 << 12
INDEPENDENT_LOG = 20


# ---------------------------------------------------------------------------------------------- circuits
def solve_and_compare(w, built, inputs, publics):
    """the device witness against the reference, bit for bit, and the counters; -> the device witness"""
    ref = RefSolver(built, inputs, publics)
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
    return got


def rebuilt(built, wire_vars=None, selector_evals=None, def_gate=None):
    """a copy of a BuiltCircuit with some arrays replaced"""
    pick = lambda new, old: old.copy() if new is None else new
    return BD.BuiltCircuit(built.curve, pick(wire_vars, built.wire_vars), pick(selector_evals, built.selector_evals), built.num_vars,
                           pick(def_gate, built.def_gate), built.input_vars, built.public_vars, built.zero_var, built.num_gates_unpadded)


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_n", [3, 5, 8, 12, 16], ids=lambda v: f"log{v}")
def test_random_layered_circuits_match_the_reference(gpu_workers, curve, cid, log_n):
    w = gpu_workers(curve)
    built, inputs, publics = random_layered(curve, log_n, 1000 * log_n + cid)
    solve_and_compare(w, built, inputs, publics)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_chain_takes_one_level_per_gate(gpu_workers, curve, cid):
    p = _fr.FIELDS[curve].p
    rnd = random.Random(5 + cid)
    b = BD.CircuitBuilder(curve)
    x = b.input()
    for _ in range(CHAIN):
        x = b.pow5_lc([x], [1], const=rnd.randrange(p))
    built = b.build()
    w = gpu_workers(curve)
    x0 = rnd.randrange(p)
    ref = RefSolver(built, [x0])
    s = built.solve_dev(w, ref.limbs([x0]))
    try:
        assert s.levels == CHAIN and s.evaluations == CHAIN + 2          # + the zero and one gates
        assert np.array_equal(s.witness(), ref.limbs(ref.solve()[0]))
        assert ref.depth() == CHAIN
    finally:
        s.close()
        built.close()
        w.trim()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_independent_gates_take_one_level(gpu_workers, oracle, curve, cid):
    w = gpu_workers(curve)
    count = (1 << INDEPENDENT_LOG) - 2
    b = BD.CircuitBuilder(curve)
    a, c = b.input(count), b.input(count)
    out = b.mul_add(a, c, a, a, q0=3, q1=5)
    built = b.build()
    assert built.n == 1 << INDEPENDENT_LOG
    inputs = oracle.rand_fr(cid, 21, 2 * count)
    s = built.solve_dev(w, inputs)
    try:
        assert s.levels == 1 and s.evaluations == count + 2
        x, y = inputs[:count], inputs[count:]
        f = _fr.FIELDS[curve]
        k3, k5 = (np.broadcast_to(f.to_limbs(v), (count, 4)).copy() for v in (3, 5))
        want = oracle.field_op(cid, 0, "add", oracle.field_op(cid, 0, "mul", k3, oracle.field_op(cid, 0, "mul", x, y)),
                               oracle.field_op(cid, 0, "mul", k5, oracle.field_op(cid, 0, "mul", x, x)))
        assert np.array_equal(s.d_witness.download((count, 4), byte_offset=int(out[0]) * 32), want)
    finally:
        s.close()
        built.close()
        w.trim()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_definitions_after_uses_give_the_same_witness(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, inputs, publics = random_layered(curve, 10, 77 + cid)
    base = solve_and_compare(w, built, inputs, publics)
    lo, hi = built.num_public, built.num_gates_unpadded
    perm = np.arange(built.n)
    perm[lo:hi] = lo + np.random.RandomState(3 + cid).permutation(hi - lo)       # new gate j is old gate perm[j]
    where = np.empty(built.n, dtype=np.int64)
    where[perm] = np.arange(built.n)
    def_gate = built.def_gate.copy()
    defined = def_gate != GIVEN
    def_gate[defined] = where[def_gate[defined].astype(np.int64)].astype(np.uint32)
    shuffled = rebuilt(built, built.wire_vars[:, perm].copy(), built.selector_evals[:, perm].copy(), def_gate)
    assert np.array_equal(solve_and_compare(w, shuffled, inputs, publics), base)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_one_variable_on_two_live_wires_and_a_dead_wire_on_the_own_output(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    b = BD.CircuitBuilder(curve)
    x, y = b.input(2)
    t = b.add(x, y)
    sq = b.mul(t, t)                                        # two live wires, one unsolved variable: two counts
    u = b.mul_add(t, sq, t, t, q0=2, q1=7)                  # three of one, one of another
    v = b.lc([sq], [3], const=11)                           # wires 1-3 dead
    built = b.build()
    wv = built.wire_vars.copy()
    g = int(built.def_gate[v])
    wv[1, g], wv[2, g], wv[3, g] = v, v, u                  # dead wires: the gate's own output, and a later variable
    edited = rebuilt(built, wire_vars=wv)
    got = solve_and_compare(w, edited, [5, 9], [])
    f = _fr.FIELDS[curve]
    assert f.from_limbs(got[v]) == 3 * 14 * 14 + 11 and f.from_limbs(got[u]) == 2 * 14 ** 3 + 7 * 14 * 14


# ---------------------------------------------------------------------------------------------- errors
def raw_solve(w, built, wire_vars=None, selector_evals=None, def_gate=None, num_vars=None):
    """plonk_circuit_solve_dev on a BuiltCircuit's arrays, some replaced; the witness is zero -> (unsolved, levels, evaluations)"""
    arrs = [built.wire_vars if wire_vars is None else wire_vars, built.selector_evals if selector_evals is None else selector_evals,
            built.def_gate if def_gate is None else def_gate]
    nv = built.num_vars if num_vars is None else num_vars
    bufs = [w.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for a in arrs] + [w.alloc(built.n * 32), w.alloc(max(nv, built.num_vars) * 32)]
    try:
        w.memset_dev(bufs[3].ptr, 0, built.n * 32)
        w.memset_dev(bufs[4].ptr, 0, max(nv, built.num_vars) * 32)
        return w.circuit_solve_dev(bufs[0].ptr, built.n, nv, bufs[1].ptr, bufs[3].ptr, bufs[2].ptr, bufs[4].ptr)
    finally:
        for x in bufs:
            x.free()


def small_circuit(curve: str):
    b = BD.CircuitBuilder(curve)
    a, c, d = b.input(3)
    x = b.add(a, c)
    y = b.add(x, d)
    z = b.mul(y, y)
    return b.build(), (a, c, d, x, y, z)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_a_cycle_is_reported_with_its_smallest_variable(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, (a, c, d, x, y, z) = small_circuit(curve)
    wv = built.wire_vars.copy()
    wv[0, int(built.def_gate[x])] = y                       # x = y + c, y = x + d
    cyc = rebuilt(built, wire_vars=wv)
    unsolved, levels, evaluations = raw_solve(w, cyc)
    assert unsolved == x and x < y
    assert evaluations == 2 and levels == 1                 # the zero and one gates; x, y and z (downstream) stay
    with pytest.raises(CI.UnsolvableCircuit) as e:
        cyc.solve_dev(w, np.zeros((3, 4), dtype=np.uint64))
    assert e.value.variable == x and f"variable {x}" in str(e.value)
    cyc.close()
    # a live wire on the gate's own output is the shortest cycle
    wv = built.wire_vars.copy()
    wv[1, int(built.def_gate[z])] = z
    assert raw_solve(w, rebuilt(built, wire_vars=wv))[0] == z


@pytest.mark.parametrize("curve,cid", CURVES)
def test_invalid_definitions_are_reported_and_the_worker_recovers(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    f = _fr.FIELDS[curve]
    built, (a, c, d, x, y, z) = small_circuit(curve)
    n, gx, gy = built.n, int(built.def_gate[x]), int(built.def_gate[y])

    def fails(mentions, **kw):
        with pytest.raises(PlonkError) as e:
            raw_solve(w, built, **kw)
        assert e.value.code == -1, str(e.value)
        for m in mentions:
            assert m in str(e.value), str(e.value)

    def with_def(v, g):
        dg = built.def_gate.copy()
        dg[v] = g
        return dg

    def with_sel(t, g, value):
        sel = built.selector_evals.copy()
        sel[t, g] = f.to_limbs(value)
        return sel

    fails([f"variable {y}", f"gate {n}"], def_gate=with_def(y, n))                       # def_gate[v] >= n
    fails([f"variable {y}", f"gate {gx}", "wire 4"], def_gate=with_def(y, gx))           # wire 4 of that gate reads x: two claims on gate gx
    fails([f"variable {a}", f"gate {gx}", "wire 4"], def_gate=with_def(a, gx))           # a given variable claiming x's gate
    fails([f"variable {x}", f"gate {gx}", "q_o"], selector_evals=with_sel(10, gx, 0))
    fails([f"variable {y}", f"gate {gy}", "q_ecc"], selector_evals=with_sel(12, gy, 5))
    wv = built.wire_vars.copy()
    wv[2, gy] = built.num_vars
    fails(["wire 2", f"gate {gy}"], wire_vars=wv)                                        # an id >= num_vars, on a dead wire too
    with pytest.raises(PlonkError) as e:
        w.circuit_solve_dev(0, n, built.num_vars, 0, 0, 0, 0)
    assert e.value.code == -1
    for bad_n in (n + 1, 0):
        with pytest.raises(PlonkError) as e:
            w.circuit_solve_dev(1, bad_n, built.num_vars, 1, 1, 1, 1)            # refused before any pointer is used
        assert e.value.code == -2
    # the worker still solves a good circuit
    got = solve_and_compare(w, built, [3, 4, 5], [])
    assert f.from_limbs(got[z]) == 144


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_runs_give_identical_bytes(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, inputs, publics = random_layered(curve, 12, 31 + cid)
    ref = RefSolver(built, inputs, publics)
    outs = []
    for _ in range(2):
        s = built.solve_dev(w, ref.limbs(inputs), ref.limbs(publics))
        outs.append((s.witness().tobytes(), s.levels, s.evaluations))
        s.close()
    built.close()
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------- end to end
ARITY, HEIGHT, SPONGE_ROUNDS = 3, 4, 2


class Sponge:
    """A fixed width-4 sponge for the tree's node hash: per round a pow5_lc layer (state <- M1 * state^5 + c1) and an lc layer
    (state <- M2 * state + c2), the node being state[0] after SPONGE_ROUNDS rounds from (left, mid, right, 0).  Its matrices and
    constants are drawn here from a seed: this is NOT jellyfish's Rescue permutation (whose constants are not available here), only
    the same kind of gates — q_hash and q_lc rows of four terms — in the same shape as the reference's compute_merkle_root."""

    def __init__(self, curve: str, seed: int = 2024):
        self.p = _fr.FIELDS[curve].p
        rnd = random.Random(seed)
        draw = lambda: rnd.randrange(1, self.p)
        self.rounds = [([[draw() for _ in range(4)] for _ in range(4)], [draw() for _ in range(4)],
                        [[draw() for _ in range(4)] for _ in range(4)], [draw() for _ in range(4)]) for _ in range(SPONGE_ROUNDS)]

    def ints(self, l, m, r):
        p, st = self.p, [l, m, r, 0]
        for M1, c1, M2, c2 in self.rounds:
            st = [(sum(M1[i][j] * pow(st[j], 5, p) for j in range(4)) + c1[i]) % p for i in range(4)]
            st = [(sum(M2[i][j] * st[j] for j in range(4)) + c2[i]) % p for i in range(4)]
        return st[0]

    def gates(self, b, l, m, r):
        st = [l, m, r, np.full(len(l), b.zero, dtype=np.int64)]
        for M1, c1, M2, c2 in self.rounds:
            st = [b.pow5_lc(st, M1[i], const=c1[i]) for i in range(4)]
            st = [b.lc(st, M2[i], const=c2[i]) for i in range(4)]
        return st[0]


def membership_circuit(curve: str, m: int, seed: int):
    """m membership paths of height HEIGHT in one 3-ary tree.  -> (BuiltCircuit, input residues, root, index of path 0's equality gate)"""
    H = Sponge(curve)
    rnd = random.Random(seed)
    leaves = [rnd.randrange(H.p) for _ in range(ARITY ** HEIGHT)]
    levels = [leaves]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([H.ints(*cur[i:i + 3]) for i in range(0, len(cur), 3)])
    root = levels[-1][0]
    index = [rnd.randrange(len(leaves)) for _ in range(m)]
    b = BD.CircuitBuilder(curve)
    d_root = b.public_input()
    cur = b.input(m)
    values = [[leaves[i] for i in index]]
    at = list(index)
    for h in range(HEIGHT):
        s0, s1 = b.input(m), b.input(m)
        pos = np.array([i % 3 for i in at])
        sib = [[levels[h][i - i % 3 + k] for k in range(3) if k != i % 3] for i in at]
        values += [[s[0] for s in sib], [s[1] for s in sib]]
        left = np.where(pos == 0, cur, s0)
        mid = np.where(pos == 1, cur, np.where(pos == 0, s0, s1))
        right = np.where(pos == 2, cur, s1)
        cur = H.gates(b, left, mid, right)
        at = [i // 3 for i in at]
    b.enforce_equal(d_root, cur)
    built = b.build()
    return built, [v for col in values for v in col], root, built.num_gates_unpadded - m


def trapdoor_key(w, n: int):
    f = _fr.FIELDS[w.curve_name]
    key_size = ((n + 3 + 31) >> 5) << 5
    q = 64 if w.curve_name == "bn254" else 96
    ck = w.alloc(key_size * q)
    w.memset_dev(ck.ptr, 0, key_size * q)
    w.synth_srs(f.to_limbs(TAU), n + 3, ck.ptr)
    w.init_dev(ck.ptr, key_size, n, 8 * n)
    return ck


@pytest.mark.parametrize("curve,cid,log_n,m", [("bls12_381", 1, 12, 62), ("bn254", 0, 14, 250), ("bn254", 0, 8, 3)],
                         ids=["bls12_381-log12", "bn254-log14", "bn254-log8"])
def test_membership_circuit_is_built_solved_proved_and_verified(gpu_workers, oracle, curve, cid, log_n, m):
    """The reference's workload shape (generate_circuit, dispatcher2.rs:1226-1271): parallel membership paths in a 3-ary tree under a
    sponge node hash (see Sponge: not jellyfish's Rescue), the root public, leaves and siblings inputs, one equality gate per path."""
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    w = gpu_workers(curve)
    n = 1 << log_n
    built, inputs, root, eq_gate = membership_circuit(curve, m, seed=log_n)
    assert built.n == n
    ref = RefSolver(built, inputs, [root])
    inst = built.preprocess(w, ref.limbs(inputs), ref.limbs([root]))
    ck = trapdoor_key(w, n)
    pv = Prover(w, log_n)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        assert np.array_equal(pub, ref.limbs([root]))
        blinders = dict(wires=oracle.rand_fr(cid, 90, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 91, 3))
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
        V.verify(B.CURVES[curve], vk, pub, proof, TAU, transcript=PlonkTranscript(curve))
    finally:
        pv.close()
        inst.close()
        ck.free()
    # one wrong sibling: the solver still fills the witness, the check names that path's equality gate
    path = m // 2
    wrong = list(inputs)
    wrong[m + 2 * m + path] = (wrong[m + 2 * m + path] + 1) % ref.f.p        # s0 of level 1 of that path
    with pytest.raises(CI.UnsatisfiedCircuit) as e:
        built.preprocess(w, ref.limbs(wrong), ref.limbs([root])).close()
    assert e.value.gate == eq_gate + path
    built.close()
    w.trim()


def test_full_size_hash_chains_bn254_log22(gpu_workers, oracle):
    """2^22 gates as 65535 parallel chains of depth 64 built with 64 array operations.  The solved witness satisfies every gate under
    plonk_circuit_check_dev, 4096 sampled variables equal the reference evaluated along their own chains, and each defining gate was
    evaluated once."""
    curve, cid, log_n, depth = "bn254", 0, 22, 64
    w = gpu_workers(curve)
    f = _fr.FIELDS[curve]
    n = 1 << log_n
    chains = (n - 2) // depth
    rnd = random.Random(22)
    b = BD.CircuitBuilder(curve)
    x, y = b.input(chains), b.input(chains)
    last = []
    for t in range(depth):
        if t % 3 == 2:
            x = b.mul_add(x, y, x, x, q0=rnd.randrange(f.p), q1=rnd.randrange(f.p))
        else:
            x = b.pow5_lc([x, y], [1, rnd.randrange(f.p)], const=rnd.randrange(f.p))
        last.append(x)
    built = b.build()
    assert built.n == n and built.num_gates_unpadded == depth * chains + 2
    inputs = oracle.rand_fr(cid, 2222, 2 * chains)
    s = built.solve_dev(w, inputs)
    d_wires = None
    try:
        assert s.evaluations == depth * chains + 2 and s.levels == depth
        d_wires = w.alloc(5 * n * 32)
        w.circuit_witness_dev(s.d_wire_vars, n, s.d_witness.ptr, built.num_vars, d_wires.ptr)
        assert w.circuit_check_dev(d_wires.ptr, s.d_selector_evals, s.d_pub.ptr, None, n) == (-1, -1)
        rs = np.random.RandomState(4096)
        sample = np.concatenate([last[-1][rs.randint(0, chains, size=2048)], rs.randint(0, built.num_vars, size=2048)])
        # ids: 0 zero, 1 one, then x, y and the 64 rounds, `chains` each: variable v >= 2 belongs to chain (v - 2) % chains
        assert int(built.input_vars[0]) == 2 and int(x[0]) == 2 + (depth + 1) * chains
        given = {}
        for c in {(int(v) - 2) % chains for v in sample if v >= 2}:
            given[2 + c], given[2 + chains + c] = f.from_limbs(inputs[c]), f.from_limbs(inputs[chains + c])
        ref = RefSolver(built, given=given)
        got = s.d_witness.download((built.num_vars, 4))
        for v in sample:
            assert f.from_limbs(got[int(v)]) == ref.value(int(v)), int(v)
    finally:
        s.close()
        built.close()
        if d_wires is not None:
            d_wires.free()
        w.trim()
