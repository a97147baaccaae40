"""The solve schedule and its replay (plonk_circuit_schedule_dev / plonk_circuit_replay_dev behind BuiltCircuit.schedule, solve_many_dev and
setup): the recorded order against a restatement from tests/hint_ref.py (tests/replay_ref.py: the level of def_gate[v] is lvl[v], the class
comes from the opcode, ties break by gate), replayed witnesses limb for limb against solve_dev for every fuse width, the shapes at which each launch form
can go wrong (a segment wider than a workgroup times K; a fused run of more than 64 levels of a few gates), device inputs, and one
accumulator's memberships set up once and proved per witness.

tests/test_hostemu_solve_replay.py runs a selection of this file on the CPU; tools/fuzz_abi.py (`--only replay`) replays random layered circuits
at the launch plan's boundaries against the reference solver."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import rescue as RS
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd.membership import membership_circuit
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.worker import REPLAY_FUSE_DEFAULT
from tests.hint_ref import HintRefSolver
from tests.replay_ref import ref_schedule

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


# ---------------------------------------------------------------------------------------------- circuits
def fanout_circuit(curve: str):
    """about 40 gates without hints: two public inputs, values used by several later gates, levels of different widths"""
    b = BD.CircuitBuilder(curve)
    p0, p1 = b.public_input(2)
    x = b.input(4)
    y = b.input()
    s = b.add(x, y)                                         # 4 gates, y fans out to all of them
    t = b.mul(s, s)
    u = b.mul_add(t, x, s, y)
    v = b.pow5_lc([u, t], [1, 3], const=7)
    acc = int(v[0])
    for i in range(1, 4):
        acc = b.add(acc, int(v[i]))                         # a chain
    z = b.lc([acc, p0, p1, y], [1, 2, 3, 4])
    b.mul(z, s)                                             # z fans out again
    b.sub(s, z)
    b.enforce_equal(b.mul(p0, p1), b.mul(p1, p0))
    return b.build(), 5, 2


def hinted_circuit(curve: str):
    """inv, div, root5 and to_bits(x, 8) beside ordinary gates, hints at level 0 and behind gates, one public input"""
    b = BD.CircuitBuilder(curve)
    out = b.public_input()
    x = b.input(3)
    small = b.input()
    i0 = b.inv(x)                                           # sources given: level 0
    s = b.add(x, out)
    q = b.div(s, i0)
    r = b.root5(b.mul(q, s))
    bits = b.to_bits(small, 8)
    t = b.mul(r, int(np.asarray(bits[0]).reshape(-1)[0]))
    b.lc([t, q, i0, b.inv(t)], [1, 1, 1, 1])
    b.root5(b.root5(r))
    return b.build(), 4, 1


def rescue_circuit(curve: str):
    """one rescue_hash2: root5 hints, dozens of levels, each a few gates wide"""
    b = BD.CircuitBuilder(curve)
    l, r = b.input(2)
    out = b.public_input()
    b.enforce_equal(b.rescue_hash2(l, r), out)
    return b.build(), 2, 1


def rescue_chain_circuit(curve: str):
    """two rescue_hash2, the second over the first's digest: one hash is 38 levels deep, the chain more than 64"""
    b = BD.CircuitBuilder(curve)
    l, r = b.input(2)
    out = b.public_input()
    b.enforce_equal(b.rescue_hash2(b.rescue_hash2(l, r), r), out)
    return b.build(), 2, 1


def flat_circuit(curve: str):
    """3000 independent products: one segment wider than a workgroup times K"""
    b = BD.CircuitBuilder(curve)
    x = b.input(3000)
    b.mul(x, x)
    return b.build(), 3000, 0


CIRCUITS = {"fanout": fanout_circuit, "hinted": hinted_circuit, "rescue": rescue_circuit, "rescue_chain": rescue_chain_circuit, "flat": flat_circuit}
_cases = {}


def case(curve: str, name: str, K: int):
    """(built, K input rows, K public rows as residues, the reference solver of row 0 — solved), computed once"""
    key = (curve, name, K)
    if key not in _cases:
        built, num_in, num_pub = CIRCUITS[name](curve)
        assert len(built.input_vars) == num_in and built.num_public == num_pub
        p = _fr.FIELDS[curve].p
        rnd = random.Random(f"replay {curve} {name}")
        ins = [[rnd.randrange(p) for _ in range(num_in)] for _ in range(K)]
        if name == "hinted":
            for row in ins:
                row[3] = rnd.randrange(256)                 # to_bits(.., 8)
            ins[-1][0] = 0                                  # an inverse of zero
        pubs = [[rnd.randrange(p) for _ in range(num_pub)] for _ in range(K)]
        ref = HintRefSolver(built, ins[0], pubs[0])
        ref.solve()
        _cases[key] = (built, ins, pubs, ref)
    return _cases[key]


def limbs3(ref, rows) -> np.ndarray:
    """K rows of residues -> (K, len, 4) Montgomery limbs"""
    return np.stack([ref.limbs(r).reshape(-1, 4) for r in rows]) if rows[0] else np.zeros((len(rows), 0, 4), dtype=np.uint64)


def solved_one_by_one(w, built, ref, ins, pubs):
    """solve_dev per row -> ([witness], levels, evaluations)"""
    outs = []
    for i, pu in zip(ins, pubs):
        s = built.solve_dev(w, ref.limbs(i), ref.limbs(pu))
        try:
            outs.append(s.witness())
            counters = (s.levels, s.evaluations)
        finally:
            s.close()
    return outs, counters


# ---------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("name", ["fanout", "hinted", "rescue"])
def test_schedule_matches_the_reference_order(gpu_workers, curve, cid, name):
    w = gpu_workers(curve)
    built, ins, pubs, ref = case(curve, name, 3)
    try:
        sched = built.schedule(w)
        order, seg, levels, evaluations = ref_schedule(built, ref)
        assert (sched.levels, sched.evaluations) == (levels, evaluations)
        assert np.array_equal(sched.seg, seg)
        assert np.array_equal(sched.order(), order)
        assert built.schedule(w) is sched                   # recorded once per upload
        _, counters = solved_one_by_one(w, built, ref, ins[:1], pubs[:1])
        assert counters == (sched.levels, sched.evaluations)
        if name == "fanout":
            assert not built.has_hints
            per_class = np.diff(sched.seg.astype(np.int64)).reshape(-1, 3).sum(axis=0)
            assert per_class[1] == 0 and per_class[2] == 0  # a circuit without hints has class 0 only
        if name == "hinted":
            per_class = np.diff(sched.seg.astype(np.int64)).reshape(-1, 3).sum(axis=0)
            assert per_class.min() > 0                      # every class occurs
    finally:
        built.close()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_recordings_give_the_same_schedule(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, _, _, _ = case(curve, "rescue", 2)
    runs = []
    for _ in range(2):
        sched = built.schedule(w)
        runs.append((sched.order().tobytes(), sched.seg.tobytes(), sched.levels, sched.evaluations))
        built.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_a_cycle_is_reported_by_schedule_as_by_solve(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    b = BD.CircuitBuilder(curve)
    a = b.input()
    x = b.add(a, a)
    y = b.inv(x)
    z = b.mul(y, y)
    b.add(z, a)
    built = b.build()
    wv = built.wire_vars.copy()
    wv[0, int(built.def_gate[x])] = z                       # x = z + a, y = 1 / x, z = y * y
    cyc = BD.BuiltCircuit(built.curve, wv, built.selector_evals, built.num_vars, built.def_gate, built.input_vars, built.public_vars, built.zero_var,
                          built.num_gates_unpadded, hint_op=built.hint_op)
    try:
        with pytest.raises(CI.UnsolvableCircuit) as by_solve:
            cyc.solve_dev(w, np.zeros((1, 4), dtype=np.uint64))
        with pytest.raises(CI.UnsolvableCircuit) as by_schedule:
            cyc.schedule(w)
        assert by_schedule.value.variable == by_solve.value.variable == x
        with pytest.raises(CI.UnsolvableCircuit):
            cyc.solve_many_dev(w, np.zeros((2, 1, 4), dtype=np.uint64))
    finally:
        cyc.close()


# ---------------------------------------------------------------------------------------------- the replay
def replay_and_compare(w, built, ref, ins, pubs, widths):
    want, _ = solved_one_by_one(w, built, ref, ins, pubs)
    K = len(ins)
    for fw in widths:
        batch = built.solve_many_dev(w, limbs3(ref, ins), limbs3(ref, pubs) if built.num_public else None, fuse_width=fw)
        try:
            assert batch.K == K
            for b in range(K):
                assert np.array_equal(batch.witness(b), want[b]), (fw, b)
        finally:
            batch.close()
    return want


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("name", ["fanout", "hinted"])
def test_replay_equals_solve_for_every_fuse_width(gpu_workers, curve, cid, name):
    w = gpu_workers(curve)
    built, ins, pubs, ref = case(curve, name, 3)
    try:
        want = replay_and_compare(w, built, ref, ins, pubs, [0, 1, None, built.n])
        assert np.array_equal(want[0], ref.limbs(ref.solve()[0]))
        assert not np.array_equal(want[0], want[1])
        replay_and_compare(w, built, ref, ins[:1], pubs[:1], [0, None])            # K = 1
    finally:
        built.close()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_replay_of_one_rescue_hash_equals_solve(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, ins, pubs, ref = case(curve, "rescue", 2)
    try:
        replay_and_compare(w, built, ref, ins, pubs, [0, None])
    finally:
        built.close()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_replay_fuses_a_run_of_more_than_64_narrow_levels(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, ins, pubs, ref = case(curve, "rescue_chain", 2)
    try:
        sched = built.schedule(w)
        per_level = np.diff(sched.seg.astype(np.int64)).reshape(-1, 3).sum(axis=1)
        assert sched.levels > 64 and per_level.min() >= 1 and per_level.max() <= 8       # 4 per level, a few more in the first two: one fused launch
        replay_and_compare(w, built, ref, ins, pubs, [0, 1, 4, None])                    # 4 breaks the run at the wider levels, 1 at every one
    finally:
        built.close()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_replay_of_a_segment_wider_than_a_workgroup_times_K(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built, ins, pubs, ref = case(curve, "flat", 2)
    try:
        sched = built.schedule(w)
        assert np.diff(sched.seg.astype(np.int64)).max() >= 3000
        replay_and_compare(w, built, ref, ins, pubs, [0, None, built.n])
    finally:
        built.close()


# ---------------------------------------------------------------------------------------------- memberships: device inputs, one setup, K proofs
HEIGHT, COUNT = 2, 9
UID_SETS = [[0, 4, 8], [1, 2, 3], [8, 7, 0]]


def accumulator(w, curve):
    rnd = random.Random(f"replay accumulator {curve}")
    f = _fr.FIELDS[curve]
    elems = np.array([f.to_limbs(rnd.randrange(f.p)) for _ in range(COUNT)], dtype=np.uint64).reshape(COUNT, 4)
    return RS.Accumulator(w, RS.RescueParams.default(curve), elems, HEIGHT)


def member_inputs(acc, uid_sets, rows):
    """-> (one device buffer with every set's solver inputs one after another, the same as a (K, rows * m, 4) host array)"""
    w, m = acc.worker, len(uid_sets[0])
    d_all = w.alloc(len(uid_sets) * rows * m * 32)
    host = []
    for b, uids in enumerate(uid_sets):
        buf = acc.witness_inputs_dev(uids)
        try:
            w.memcpy_d2d(d_all.ptr + b * rows * m * 32, buf.ptr, rows * m * 32)
            host.append(buf.download((rows * m, 4)))
        finally:
            buf.free()
    return d_all, np.stack(host)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_device_inputs_give_the_same_witnesses_as_host_inputs(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    built = membership_circuit(curve, HEIGHT, 3)
    acc = accumulator(w, curve)
    d_all = None
    try:
        K = len(UID_SETS)
        d_all, host = member_inputs(acc, UID_SETS, 2 + 4 * HEIGHT)
        roots = np.broadcast_to(acc.root.reshape(1, 1, 4), (K, 1, 4))
        from_host = built.solve_many_dev(w, host, roots)
        from_dev = built.solve_many_dev(w, public_inputs=roots, d_inputs=d_all.ptr)
        try:
            for b in range(K):
                one = built.solve_dev(w, host[b], roots[b])
                try:
                    want = one.witness()
                finally:
                    one.close()
                assert np.array_equal(from_host.witness(b), want) and np.array_equal(from_dev.witness(b), want), b
        finally:
            from_host.close()
            from_dev.close()
        with pytest.raises(ValueError):
            built.solve_many_dev(w, host, roots, d_inputs=d_all.ptr)
    finally:
        if d_all is not None:
            d_all.free()
        acc.close()
        built.close()


def test_one_setup_proves_every_witness_and_refuses_a_wrong_one(gpu_workers, oracle):
    from tests.test_gpu_solve import trapdoor_key
    curve, cid = "bn254", 0
    w = gpu_workers(curve)
    built = membership_circuit(curve, HEIGHT, 3)
    acc = accumulator(w, curve)
    d_all = key = batch = pv = ck = None
    try:
        rows = 2 + 4 * HEIGHT
        d_all, host = member_inputs(acc, UID_SETS, rows)
        swapped = host[0].reshape(rows, 3, 4).copy()                    # row 2 / 3: sib1 / sib2 of level 0; column 1: uid 4, the middle of its group
        swapped[2, 1], swapped[3, 1] = host[0].reshape(rows, 3, 4)[3, 1], host[0].reshape(rows, 3, 4)[2, 1]
        assert not np.array_equal(swapped[2, 1], swapped[3, 1])
        inputs = np.concatenate([host, swapped.reshape(1, rows * 3, 4)])
        K = inputs.shape[0]
        root = acc.root.reshape(1, 4).copy()
        key = built.setup(w)                                            # once
        batch = built.solve_many_dev(w, inputs, np.broadcast_to(root.reshape(1, 1, 4), (K, 1, 4)))
        # the key is what preprocess computes for the same circuit
        inst = built.preprocess(w, host[0], root)
        try:
            n = built.n
            assert np.array_equal(key.d_id.download((5 * n, 4)), inst.d_id.download((5 * n, 4)))
            assert np.array_equal(key.d_idx.download((5 * n,)), inst.d_idx.download((5 * n,)))
            assert np.array_equal(key.d_sel.download((13 * n, 4)), inst.d_sel.download((13 * n, 4)))
            assert np.array_equal(key.d_sig.download((5 * n, 4)), inst.d_sig.download((5 * n, 4)))
            first_wires = inst.d_wires.download((5 * n, 4))
        finally:
            inst.close()
        ck = trapdoor_key(w, built.n)
        pv = Prover(w, built.log_n)
        pv.load_key_dev(key.sel_ptrs, key.sig_ptrs, key.k)            # once
        vk = pv.verifying_key()
        ok = VF.OpenKey.from_trapdoor(curve, TAU)
        blinders = dict(wires=oracle.rand_fr(cid, 98, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 99, 3))
        proved = 0
        with pytest.raises(CI.UnsatisfiedCircuit):
            for b, one in enumerate(key.instances(batch)):              # the fourth raises when it is made
                try:
                    if b == 0:
                        assert np.array_equal(one.d_wires.download((5 * n, 4)), first_wires)
                    pub = one.public_inputs()
                    assert np.array_equal(pub, root) and (one.n, one.log_n, one.num_inputs) == (n, built.log_n, 1)
                    proof = pv.prove_dev(one.wev, one.d_id.ptr, one.d_idx.ptr, one.d_pi.ptr, blinders, pv.fiat_shamir(pub))
                    assert VF.verify(w, vk, ok, pub, proof)
                    proved += 1
                finally:
                    one.close()
        assert proved == 3
        # without the check the fourth is placed like any other; host values for the public input are taken too
        last = key.instance(batch.d_witness.ptr + 3 * built.num_vars * 32, root, check=False)
        last.close()
    finally:
        for x in (pv, batch, key):
            if x is not None:
                x.close()
        for x in (ck, d_all):
            if x is not None:
                x.free()
        acc.close()
        built.close()
        w.trim()
