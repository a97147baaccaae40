"""The Edwards gadgets of builder.py solved on the device, and the whole pipeline of a signature circuit: every gadget circuit of
tests/test_edwards_host.py (GADGET_CASES, m = 3) solved by solve_dev equals the sequential big-integer solve, variable for variable;
edwards.schnorr_circuit(curve, 2) is built, solved from keys and signatures made ON THE DEVICE (edwards.keygen, edwards.schnorr_sign), proved
and verified with verifier.verify — the worked example of the README —; a tampered signature raises UnsatisfiedCircuit; and solve_many_dev
replays K = 3 signature sets, one of them bad: each witness bit-identical to solve_dev's, the bad set alone refused by CircuitKey.instances.

tests/test_hostemu_edwards.py runs one of the solves on the CPU."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd.prover import Prover
from tests import edwards_ref as E
from tests.hint_ref import HintRefSolver
from tests.test_edwards_host import GADGET_CASES
from tests.test_gpu_edwards import from_limbs, pts_from_limbs, to_limbs
from tests.test_gpu_solve import TAU, trapdoor_key

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("name", list(GADGET_CASES))
def test_gadget_circuits_solve_on_the_device_as_on_the_cpu(gpu_workers, curve, cid, name):
    w = gpu_workers(curve)
    built, values, pub, _ = GADGET_CASES[name](curve, 3)
    ref = HintRefSolver(built, values, pub)
    want, _ = ref.solve()
    assert ref.unsatisfied_gates(want) == []
    s = built.solve_dev(w, to_limbs(curve, values), to_limbs(curve, pub))
    try:
        assert s.levels == ref.depth()
        assert np.array_equal(s.witness(), ref.limbs(want))
    finally:
        s.close()
        built.close()


_made = {}


def device_signatures(w, curve, sets, m):
    """`sets` x m keys and signatures made on the device, checked against the reference once -> (pk, messages, (R, s)) arrays of sets * m rows"""
    key = (curve, sets, m)
    if key not in _made:
        prm = ED.EdwardsParams.default(curve)
        r, G = E.MODULI[curve], E.PARAMS[curve]["G"]
        rnd = random.Random(f"circuit signatures {curve}")
        sks, nonces, msgs = ([rnd.randrange(1, r) for _ in range(sets * m)] for _ in range(3))
        pk = ED.keygen(w, prm, to_limbs(curve, sks))
        R, s = ED.schnorr_sign(w, prm, to_limbs(curve, sks), to_limbs(curve, nonces), to_limbs(curve, msgs))
        assert pts_from_limbs(curve, pk[:1]) == [E.mul(curve, sks[0], G)]
        assert (pts_from_limbs(curve, R[:1])[0], from_limbs(curve, s[:1])[0]) == E.schnorr_sign(curve, sks[0], nonces[0], msgs[0])
        assert ED.in_subgroup(w, prm, pk).all() and ED.schnorr_verify(w, prm, pk, to_limbs(curve, msgs), (R, s)).all()
        _made[key] = (pk, to_limbs(curve, msgs), (R, s))
    return _made[key]


def blinders(curve, seed):
    rnd = random.Random(seed)
    r = E.MODULI[curve]
    return dict(wires=to_limbs(curve, [rnd.randrange(r) for _ in range(10)]).reshape(5, 2, 4), perm=to_limbs(curve, [rnd.randrange(r) for _ in range(3)]))


def test_schnorr_circuit_is_built_solved_proved_and_verified(gpu_workers):
    curve, m = "bn254", 2
    w = gpu_workers(curve)
    pk, msgs, (R, s) = device_signatures(w, curve, 1, m)
    built = ED.schnorr_circuit(curve, m)
    assert built.n == 1 << 14 and built.has_hints and built.num_public == 3 * m
    inputs, public = ED.schnorr_witness_inputs(pk, msgs, (R, s))
    inst = built.preprocess(w, inputs, public, check=True)
    ck = pv = None
    try:
        ck = trapdoor_key(w, built.n)
        pv = Prover(w, built.log_n)
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        assert np.array_equal(pub, public)
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders(curve, 1), pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        ok = VF.OpenKey.from_trapdoor(curve, TAU)
        assert VF.verify(w, vk, ok, pub, proof)
        other = pub.copy()                                 # the proof speaks about THESE public keys and messages
        other[2 * m] = to_limbs(curve, [from_limbs(curve, pub[2 * m:2 * m + 1])[0] + 1])[0]
        assert not VF.verify(w, vk, ok, other, proof)
    finally:
        if pv is not None:
            pv.close()
        inst.close()
        if ck is not None:
            ck.free()
    # a tampered signature: s + 1 in the second one; then R of the first replaced by another curve point
    l = E.PARAMS[curve]["l"]
    bad_s = s.copy()
    bad_s[1] = to_limbs(curve, [(from_limbs(curve, s[1:2])[0] + 1) % l])[0]
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, ED.schnorr_witness_inputs(pk, msgs, (R, bad_s))[0], public, check=True).close()
    bad_R = R.copy()
    bad_R[0] = R[1]
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, ED.schnorr_witness_inputs(pk, msgs, (bad_R, s))[0], public, check=True).close()
    built.close()
    w.trim()


def test_replay_solves_three_signature_sets_and_refuses_the_bad_one(gpu_workers):
    curve, m, K = "bn254", 2, 3
    w = gpu_workers(curve)
    pk, msgs, (R, s) = device_signatures(w, curve, K, m)
    s = s.copy()
    bad = 1
    s[bad * m] = to_limbs(curve, [(from_limbs(curve, s[bad * m:bad * m + 1])[0] + 1) % E.PARAMS[curve]["l"]])[0]
    sets = [ED.schnorr_witness_inputs(pk[b * m:(b + 1) * m], msgs[b * m:(b + 1) * m], (R[b * m:(b + 1) * m], s[b * m:(b + 1) * m])) for b in range(K)]
    inputs, publics = np.stack([x for x, _ in sets]), np.stack([y for _, y in sets])
    built = ED.schnorr_circuit(curve, m)
    key = batch = None
    try:
        batch = built.solve_many_dev(w, inputs, publics)
        for b in range(K):
            one = built.solve_dev(w, inputs[b], publics[b])
            try:
                assert np.array_equal(batch.witness(b), one.witness()), b
            finally:
                one.close()
        key = built.setup(w)
        refused = []
        for b in range(K):
            d_wit = batch.d_witness.ptr + b * built.num_vars * 32
            d_pub = batch.d_pub.ptr + b * built.num_public * 32
            try:
                key.instance(d_wit, d_pub, True).close()
            except CI.UnsatisfiedCircuit:
                refused.append(b)
        assert refused == [bad]
        with pytest.raises(CI.UnsatisfiedCircuit):           # and through the generator: the first two are made, the bad one raises
            for b, one in enumerate(key.instances(batch)):
                one.close()
                assert b < bad
    finally:
        for x in (batch, key):
            if x is not None:
                x.close()
        built.close()
        w.trim()
