"""Batched verification on the device (plonk_verify_batch_dev, distributed_plonk_amd/verifier.py) against the trapdoor verifier
oracle/verifier_ref.py: device challenges bit-identical to PlonkTranscript, PI(zeta) / r(zeta) / E and the points A, B (rho = 1) equal to
the integer statement, honest proofs accepted without the trapdoor (pairing on the host), every mutation rejected by both verifiers,
batch_verify with bisection, malformed input reported by status, check_srs."""
import copy

import numpy as np
import pytest

from distributed_plonk_amd import _ffi
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.synthetic import SyntheticInstance
from distributed_plonk_amd.transcript import PlonkTranscript
from tests.circuit_cases import _blinders, _proved

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


def _ref_ok(curve, vk, pub, proof, tau=TAU):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    try:
        V.verify(B.CURVES[curve], vk, pub, proof, tau, transcript=PlonkTranscript(curve))
        return True
    except V.VerificationError:
        return False


def _g1_point(curve, s):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    cv = B.CURVES[curve]
    return V.point_limbs(cv, B.scalar_mul(cv, s, (cv.gx, cv.gy)))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_device_challenges_scalars_and_points_match_the_reference(gpu_workers, oracle, curve, cid):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid)
    cv = B.CURVES[curve]
    f = _fr.FIELDS[curve]
    rng = np.random.RandomState(5)
    pubs = [pub] + [np.stack([f.to_limbs(int(x)) for x in rng.randint(0, 1 << 62, size=3)]) for _ in range(4)]
    prfs = [proofs[i % len(proofs)] for i in range(len(pubs))]
    one = np.stack([f.to_limbs(1)] * len(pubs))
    pts, status, dbg = VF.device_verify(w, vk, pubs, prfs, one, debug=True)
    assert (status == 0).all()
    for j, (pi, pr) in enumerate(zip(pubs, prfs)):
        t = PlonkTranscript(curve)
        ch = V.derive_challenges(t, vk, pi, pr)
        for i, name in enumerate(["beta", "gamma", "alpha", "zeta", "v", "u"]):
            assert np.array_equal(dbg[j, i], ch[name]), (j, name)
        # the integer statement with the same challenges (verify raises for the wrong public inputs: recompute the parts by hand then)
        n = vk["domain_size"]
        I = lambda l: V.fr_int(cv, l)
        zeta = I(ch["zeta"])
        pi_int = V.lagrange_pi_eval(cv, n, [I(x) for x in pi], zeta)
        assert V.fr_int(cv, dbg[j, 6]) == pi_int
        if j == 0:
            res = V.verify(cv, vk, pi, pr, TAU, challenges=ch)
            assert V.fr_int(cv, dbg[j, 7]) == res["lin_eval"] and V.fr_int(cv, dbg[j, 8]) == res["batch_eval"]
            r = cv.fr.p
            u, omega = I(ch["u"]), cv.fr.root_of_unity(n)
            P = lambda pt: V.point_int(cv, pt)
            A = V.g1_lincomb(cv, [(1, P(pr["opening_proof"])), (u, P(pr["shifted_opening_proof"]))])
            Bp = V.g1_lincomb(cv, [(zeta, P(pr["opening_proof"])), (u * zeta * omega % r, P(pr["shifted_opening_proof"])), (1, res["batch_comm"]),
                                   (u, P(pr["prod_perm_poly_comm"])), ((-(res["batch_eval"] + u * I(pr["perm_next_eval"]))) % r, (cv.gx, cv.gy))])
            assert np.array_equal(pts[j, 1], V.point_limbs(cv, A)[0])
            assert np.array_equal(pts[j, 0], V.point_limbs(cv, Bp)[0])


@pytest.mark.parametrize("curve,cid", CURVES)
def test_honest_proofs_accepted_and_mutations_rejected(gpu_workers, oracle, curve, cid):
    w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid)
    ok_key = VF.OpenKey.from_trapdoor(curve, TAU)
    st = {}
    for pr in proofs:
        assert VF.verify(w, vk, ok_key, pub, pr, stats=st) and _ref_ok(curve, vk, pub, pr)
        assert st["pairing_checks"] == 1
    pr = proofs[0]
    other = _g1_point(curve, 12345)
    names = [("wires_poly_comms", i) for i in range(5)] + [("prod_perm_poly_comm", None)] + [("split_quot_poly_comms", i) for i in range(5)] \
        + [("opening_proof", None), ("shifted_opening_proof", None)]
    f = _fr.FIELDS[curve]
    for name, i in names:
        bad = copy.deepcopy(pr)
        if i is None:
            bad[name] = other
        else:
            bad[name] = list(bad[name])
            bad[name][i] = other
        assert not VF.verify(w, vk, ok_key, pub, bad), (name, i)
        assert not _ref_ok(curve, vk, pub, bad), (name, i)
    evs = [("wires_evals", i) for i in range(5)] + [("wire_sigma_evals", i) for i in range(4)] + [("perm_next_eval", None)]
    for name, i in evs:
        bad = copy.deepcopy(pr)
        if i is None:
            bad[name] = f.to_limbs((f.from_limbs(bad[name]) + 1) % f.p)
        else:
            bad[name] = [np.asarray(x) for x in bad[name]]
            bad[name][i] = f.to_limbs((f.from_limbs(bad[name][i]) + 1) % f.p)
        assert not VF.verify(w, vk, ok_key, pub, bad), (name, i)
        assert not _ref_ok(curve, vk, pub, bad), (name, i)
    pub2 = pub.copy()
    pub2[1] = f.to_limbs((f.from_limbs(pub2[1]) + 1) % f.p)
    assert not VF.verify(w, vk, ok_key, pub2, pr) and not _ref_ok(curve, vk, pub2, pr)
    # another circuit's verifying key, an open key of another tau
    _, vk2, pub_o, _ = _proved(gpu_workers, oracle, curve, cid, nproofs=1, seed=9)
    assert not VF.verify(w, vk2, ok_key, pub, pr) and not _ref_ok(curve, vk2, pub, pr)
    assert not VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU + 1), pub, pr) and not _ref_ok(curve, vk, pub, pr, tau=TAU + 1)


def test_honest_proof_accepted_bn254_2p20(gpu_workers, oracle):
    w, vk, pub, proofs = _proved(gpu_workers, oracle, "bn254", 0, log_n=20, nproofs=1, seed=4)
    assert VF.verify(w, vk, VF.OpenKey.from_trapdoor("bn254", TAU), pub, proofs[0])


@pytest.mark.parametrize("curve,cid", CURVES)
def test_hand_written_circuit_verifies(gpu_workers, oracle, curve, cid):
    from tests.test_gpu_circuit import _chain_circuit, _trapdoor_key
    from distributed_plonk_amd import circuit as CI
    w = gpu_workers(curve)
    n = 1 << 10
    circ = _chain_circuit(cid, n - 37, seed=10 + cid).pad(0)
    inst = CI.preprocess(w, circ)
    ck = _trapdoor_key(w, n)
    pv = Prover(w, 10)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, _blinders(oracle, cid, 90), pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
    finally:
        pv.close()
        inst.close()
        ck.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_batch_verify_bisects_to_the_bad_proofs(gpu_workers, oracle, curve, cid):
    w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid)
    key = VF.OpenKey.from_trapdoor(curve, TAU)
    f = _fr.FIELDS[curve]
    K = 64
    batch = [proofs[i % len(proofs)] for i in range(K)]
    st = {}
    assert VF.batch_verify(w, vk, key, [pub] * K, batch, seed=1, stats=st) == [True] * K
    assert st["pairing_checks"] == 1
    bad_idx = [3, 31, 50]
    for i in bad_idx:
        b = copy.deepcopy(batch[i])
        b["perm_next_eval"] = f.to_limbs((f.from_limbs(b["perm_next_eval"]) + i) % f.p)
        batch[i] = b
    got = VF.batch_verify(w, vk, key, [pub] * K, batch, seed=2, stats=st)
    assert [i for i, v in enumerate(got) if not v] == bad_idx
    assert st["pairing_checks"] <= 1 + 2 * len(bad_idx) * 6
    assert VF.batch_verify(w, vk, key, [pub] * K, batch, seed=2) == got
    assert VF.batch_verify(w, vk, key, [pub], [batch[3]]) == [VF.verify(w, vk, key, pub, batch[3])] == [False]
    assert VF.batch_verify(w, vk, key, [pub], [batch[0]], seed=5) == [VF.verify(w, vk, key, pub, batch[0])] == [True]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_malformed_input_gives_a_status(gpu_workers, oracle, curve, cid):
    w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid)
    key = VF.OpenKey.from_trapdoor(curve, TAU)
    pr = copy.deepcopy(proofs[0])
    xy, inf = pr["opening_proof"]
    off = np.array(xy, dtype=np.uint64).copy()
    off[0] ^= np.uint64(1)
    pr["opening_proof"] = (off, False)
    st = {}
    assert VF.batch_verify(w, vk, key, [pub, pub], [pr, proofs[1]], seed=3, stats=st) == [False, True]
    assert st["status"][0] & 1 and st["status"][1] == 0
    if curve == "bls12_381":
        # an on-curve point of order 3 (x = 0: y^2 = 4 has the solution y = 2) lies outside the r-subgroup
        q = w.q64
        tor = np.array(VF._fq_mont(curve, 0) + VF._fq_mont(curve, 2), dtype=np.uint64)
        assert tor.shape == (2 * q,)
        pr2 = copy.deepcopy(proofs[0])
        pr2["wires_poly_comms"] = list(pr2["wires_poly_comms"])
        pr2["wires_poly_comms"][2] = (tor, False)
        assert VF.batch_verify(w, vk, key, [pub], [pr2], seed=3, stats=st) == [False]
        assert st["status"][0] == 2
    # bad arguments are refused, then a working call
    recs = VF.proof_record(curve, proofs[0])[None, :]
    kb = VF._vk_state(curve, vk, 3)
    import ctypes as C
    with pytest.raises(PlonkError):
        _ffi.check(_ffi.lib().plonk_verify_batch_dev(w.ctx, C.byref(kb), 1, None, None, None, None, None, None))
    kb.domain_size = 1000
    d = w.alloc(recs.nbytes).upload(recs)
    kb.d_comms = d.ptr
    try:
        rc = _ffi.lib().plonk_verify_batch_dev(w.ctx, C.byref(kb), 1, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, None)
        assert rc == -2
    finally:
        d.free()
    assert VF.verify(w, vk, key, pub, proofs[0])


@pytest.mark.parametrize("curve,cid", CURVES)
def test_check_srs(gpu_workers, oracle, curve, cid):
    w = gpu_workers(curve)
    log_n = 6
    inst = SyntheticInstance(w, log_n, seed=2, num_inputs=1, tau=TAU)
    try:
        key = VF.OpenKey.from_trapdoor(curve, TAU)
        assert VF.check_srs(w, key, 32, seed=1)
        assert not VF.check_srs(w, VF.OpenKey.from_trapdoor(curve, TAU + 1), 32, seed=1)
        # one power altered: P_7 <- P_7 + G
        q = w.q64
        ck = inst.d_ck.download((inst.key_size, 2 * q))
        from oracle import bigint_ref as B
        from oracle import verifier_ref as V
        cv = B.CURVES[curve]
        P7 = V.point_int(cv, (ck[7], False))
        ck[7] = V.point_limbs(cv, B.affine_add(cv, P7, (cv.gx, cv.gy)))[0]
        inst.d_ck.upload(ck)
        w.init_dev(inst.d_ck.ptr, inst.key_size, inst.n, 8 * inst.n)
        assert not VF.check_srs(w, key, 32, seed=1)
    finally:
        inst.close()
