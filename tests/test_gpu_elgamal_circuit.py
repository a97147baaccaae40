"""The sponge, stream and encryption gadgets of builder.py solved on the device, and the whole pipeline of an encryption circuit: every
gadget circuit of tests/test_elgamal_host.py (GADGET_CASES, m = 3) solved by solve_dev equals the sequential big-integer solve, variable for
variable; elgamal.elgamal_circuit("bn254", 2, 4) is built, solved from keys and ciphertexts made ON THE DEVICE (elgamal.keygen,
elgamal.encrypt), proved and verified with verifier.verify — the worked example of the README —; the proof is refused for another ciphertext,
a witness with another message or another r raises UnsatisfiedCircuit; and solve_many_dev replays K = 3 witness sets, one of them bad: each
witness bit-identical to solve_dev's, the bad set alone refused by CircuitKey.instances.

tests/test_hostemu_elgamal.py runs one of the solves on the CPU."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import elgamal as EG
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd.prover import Prover
from tests import edwards_ref as E
from tests import elgamal_ref as G
from tests.hint_ref import HintRefSolver
from tests.test_elgamal_host import GADGET_CASES
from tests.test_gpu_edwards import from_limbs, pts_from_limbs, to_limbs
from tests.test_gpu_edwards_circuit import blinders
from tests.test_gpu_elgamal import texts_from_limbs, texts_to_limbs
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


def device_ciphertexts(w, curve, sets, m, L):
    """`sets` x m keys and ciphertexts made on the device, one checked against the reference -> (ek, r, msg, (E, ct)) arrays of sets * m rows"""
    key = (curve, sets, m, L)
    if key not in _made:
        prm = ED.EdwardsParams.default(curve)
        r, l = E.MODULI[curve], E.PARAMS[curve]["l"]
        rnd = random.Random(f"circuit ciphertexts {curve}")
        dks, rands = ([rnd.randrange(1, l) for _ in range(sets * m)] for _ in range(2))
        msgs = [[rnd.randrange(r) for _ in range(L)] for _ in range(sets * m)]
        dk_limbs, r_limbs, msg_limbs = to_limbs(curve, dks), to_limbs(curve, rands), texts_to_limbs(curve, msgs)
        ek = EG.keygen(w, prm, dk_limbs)
        Ep, ct = EG.encrypt(w, prm, ek, msg_limbs, r_limbs)
        ek0 = G.keygen(curve, dks[0])
        assert pts_from_limbs(curve, ek[:1]) == [ek0]
        assert (pts_from_limbs(curve, Ep[:1])[0], texts_from_limbs(curve, ct[:1])[0]) == G.encrypt(curve, ek0, msgs[0], rands[0])
        assert ED.in_subgroup(w, prm, ek).all()
        back, ok = EG.decrypt(w, prm, dk_limbs, (Ep, ct))
        assert ok.all() and np.array_equal(back, msg_limbs)
        _made[key] = (ek, r_limbs, msg_limbs, (Ep, ct))
    return _made[key]


def bump(curve, limbs, modulus):
    """the element + 1 mod `modulus`, as limbs"""
    return to_limbs(curve, [(from_limbs(curve, np.asarray(limbs).reshape(1, 4))[0] + 1) % modulus])[0]


def test_encryption_circuit_is_built_solved_proved_and_verified(gpu_workers):
    curve, m, L = "bn254", 2, 4
    w = gpu_workers(curve)
    ek, rand, msg, (Ep, ct) = device_ciphertexts(w, curve, 1, m, L)
    built = EG.elgamal_circuit(curve, m, L)
    assert built.n == 1 << 14 and built.has_hints and built.num_public == (4 + L) * m and len(built.input_vars) == (1 + L) * m
    inputs, public = EG.elgamal_witness_inputs(ek, rand, msg, (Ep, ct))
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
        other = pub.copy()                                 # the proof speaks about THIS ciphertext: ct_1 of the second one changed
        at = (4 + 1) * m + 1
        other[at] = bump(curve, pub[at], E.MODULI[curve])
        assert not VF.verify(w, vk, ok, other, proof)
    finally:
        if pv is not None:
            pv.close()
        inst.close()
        if ck is not None:
            ck.free()
    # a witness with another message (msg_2 of the first ciphertext), then with another r (of the second)
    bad_msg = msg.copy()
    bad_msg[0, 2] = bump(curve, msg[0, 2], E.MODULI[curve])
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, EG.elgamal_witness_inputs(ek, rand, bad_msg, (Ep, ct))[0], public, check=True).close()
    bad_r = rand.copy()
    bad_r[1] = bump(curve, rand[1], E.PARAMS[curve]["l"])
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, EG.elgamal_witness_inputs(ek, bad_r, msg, (Ep, ct))[0], public, check=True).close()
    built.close()
    w.trim()


def test_replay_solves_three_witness_sets_and_refuses_the_bad_one(gpu_workers):
    curve, m, L, K = "bn254", 2, 4, 3
    w = gpu_workers(curve)
    ek, rand, msg, (Ep, ct) = device_ciphertexts(w, curve, K, m, L)
    msg = msg.copy()
    bad = 1
    msg[bad * m, 3] = bump(curve, msg[bad * m, 3], E.MODULI[curve])
    cut = lambda a, b: a[b * m:(b + 1) * m]
    sets = [EG.elgamal_witness_inputs(cut(ek, b), cut(rand, b), cut(msg, b), (cut(Ep, b), cut(ct, b))) for b in range(K)]
    inputs, publics = np.stack([x for x, _ in sets]), np.stack([y for _, y in sets])
    built = EG.elgamal_circuit(curve, m, L)
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
        with pytest.raises(CI.UnsatisfiedCircuit):           # and through the generator: the first is made, the bad one raises
            for b, one in enumerate(key.instances(batch)):
                one.close()
                assert b < bad
    finally:
        for x in (batch, key):
            if x is not None:
                x.close()
        built.close()
        w.trim()
