"""Preprocessing of user circuits on the device (distributed_plonk_amd/circuit.py over plonk_circuit_{permutation,witness,check}_dev):
the copy-constraint permutation against a numpy restatement of jellyfish's compute_wire_permutation (the stable-argsort recipe of
oracle/prover_ref.py:make_circuit), against the synthetic generator's own wiring at full size, witness placement and the
satisfiability check against numpy, a hand-written circuit proved end to end and accepted by oracle/verifier_ref.py, argument
validation and run-to-run determinism."""
import numpy as np
import pytest

from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.synthetic import SyntheticInstance, wire_subset_separators
from distributed_plonk_amd.transcript import PlonkTranscript
from distributed_plonk_amd import fr as _fr
from tests.circuit_cases import ref_id_perm, ref_perm_idx, wiring

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


def run_permutation(w, wire_vars: np.ndarray, num_vars: int, k: np.ndarray):
    n = wire_vars.shape[1]
    dv = w.alloc(wire_vars.size * 4).upload(np.ascontiguousarray(wire_vars, dtype=np.uint32))
    did, didx, dsig = w.alloc(5 * n * 32), w.alloc(5 * n * 8), w.alloc(5 * n * 32)
    try:
        w.circuit_permutation_dev(dv.ptr, n, num_vars, k, did.ptr, didx.ptr, dsig.ptr)
        w.sync()
        return did.download((5 * n, 4)), didx.download((5 * n,)), dsig.download((5 * n, 4))
    finally:
        for b in (dv, did, didx, dsig):
            b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_n", [3, 5, 8, 12, 16])
@pytest.mark.parametrize("kind", ["identity", "single", "random", "heavy"])
def test_permutation_matches_stable_argsort(gpu_workers, oracle, curve, cid, log_n, kind):
    w = gpu_workers(curve)
    n = 1 << log_n
    k = wire_subset_separators(_fr.FIELDS[curve], 3 + log_n)
    wv, nv = wiring(kind, n, 100 * log_n + cid)
    id_perm, perm_idx, sigma = run_permutation(w, wv, nv, k)
    want_idx = ref_perm_idx(wv)
    assert np.array_equal(perm_idx, want_idx)
    want_id = ref_id_perm(oracle, cid, n, k)
    assert np.array_equal(id_perm, want_id)
    assert np.array_equal(sigma, want_id[want_idx.astype(np.int64)])
    if kind == "identity":
        assert np.array_equal(perm_idx, np.arange(5 * n, dtype=np.uint64))


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("num_vars", [(1 << 8) + 1, (1 << 16) + 1, (1 << 24) + 1])
def test_permutation_every_radix_pass_count(gpu_workers, oracle, curve, cid, num_vars):
    """ids that need 2, 3 and 4 eight-bit passes (the largest id is present)."""
    w = gpu_workers(curve)
    n = 1 << 10
    rs = np.random.RandomState(num_vars & 0xFFFF)
    wv = rs.randint(0, num_vars, size=(5, n)).astype(np.uint32)
    wv[:, :8] = rs.randint(0, 4, size=(5, 8))                 # some repeats whatever num_vars is
    wv[2, 17] = num_vars - 1
    wv[4, 100] = num_vars - 1
    k = wire_subset_separators(_fr.FIELDS[curve], 5)
    id_perm, perm_idx, sigma = run_permutation(w, wv, num_vars, k)
    want_idx = ref_perm_idx(wv)
    assert np.array_equal(perm_idx, want_idx)
    assert np.array_equal(sigma, id_perm[want_idx.astype(np.int64)])
    assert np.array_equal(id_perm, ref_id_perm(oracle, cid, n, k))


def _synth_wire_vars(perm_idx: np.ndarray, n: int) -> np.ndarray:
    """The variable of every position of a synthetic instance: its cycles start in column 0 and run through columns 0 -> 1 -> ... -> 4."""
    pi = perm_idx.astype(np.int64)
    var = np.full(5 * n, -1, dtype=np.int64)
    cur = np.arange(n, dtype=np.int64)
    for hop in range(5):
        assert np.array_equal(cur // n, np.full(n, hop))
        var[cur] = np.arange(n)
        cur = pi[cur]
    assert np.array_equal(cur, np.arange(n)) and (var >= 0).all()
    return var.astype(np.uint32).reshape(5, n)


def _compare_columns(a, b, n: int, what: str):
    for i in range(5):
        assert np.array_equal(a.download((n, 4), byte_offset=i * n * 32), b.download((n, 4), byte_offset=i * n * 32)), f"{what} column {i}"


@pytest.mark.parametrize("curve,log_n", [("bn254", 20), ("bls12_381", 22), ("bn254", 24)], ids=["bn254-log20", "bls12_381-log22", "bn254-log24"])
def test_full_size_reproduces_the_synthetic_generator(gpu_workers, curve, log_n):
    """preprocess_dev on the wiring recovered from plonk_synth_circuit's cycles, with the witness read back from its column 0, gives back
    the generator's perm_idx, sigma evaluations and wires bit for bit, and the check finds the instance satisfied."""
    w = gpu_workers(curve)
    n = 1 << log_n
    inst = SyntheticInstance(w, log_n, seed=7 + log_n, num_inputs=3)
    dv = pre = None
    try:
        perm_idx = inst.d_idx.download((5 * n,))
        wv = _synth_wire_vars(perm_idx, n)
        dv = w.alloc(wv.nbytes).upload(wv)
        pre = CI.preprocess_dev(w, dv.ptr, n, n, inst.wev[0], inst.d_sel_ev.ptr, inst.d_pi.ptr, 3, k=inst.k, check=True)
        assert np.array_equal(pre.d_idx.download((5 * n,)), perm_idx)
        del perm_idx, wv
        _compare_columns(pre.d_sig_ev, inst.d_sig_ev, n, "sigma evaluations")
        _compare_columns(pre.d_wires, inst.d_wires, n, "wires")
        _compare_columns(pre.d_id, inst.d_id, n, "id_perm")
        assert np.array_equal(pre.public_inputs(), inst.public_inputs())
    finally:
        if pre is not None:
            pre.close()
        if dv is not None:
            dv.free()
        inst.close()
        w.trim()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_witness_placement_and_check(gpu_workers, oracle, curve, cid):
    from oracle import prover_ref as P
    w = gpu_workers(curve)
    log_n = 10
    n = 1 << log_n
    rs = np.random.RandomState(cid)
    # placement against numpy indexing
    nv = 3 * n
    wv = rs.randint(0, nv, size=(5, n)).astype(np.uint32)
    wit = oracle.rand_fr(cid, 11, nv)
    dv, dwit, dw = w.alloc(wv.nbytes).upload(wv), w.alloc(wit.nbytes).upload(wit), w.alloc(5 * n * 32)
    try:
        w.circuit_witness_dev(dv.ptr, n, dwit.ptr, nv, dw.ptr)
        assert np.array_equal(dw.download((5, n, 4)), wit[wv.astype(np.int64)])
    finally:
        for b in (dv, dwit, dw):
            b.free()
    # a synthetic instance is satisfied
    inst = SyntheticInstance(w, log_n, seed=5, num_inputs=2)
    try:
        assert w.circuit_check_dev(inst.d_wires.ptr, inst.d_sel_ev.ptr, inst.d_pi.ptr, inst.d_idx.ptr, n) == (-1, -1)
    finally:
        inst.close()
    # so is a make_circuit instance; then one selector, one wire value, one broken cycle
    circ = P.make_circuit(cid, log_n, 3)
    sel_ev = np.stack([oracle.ntt(cid, circ["selectors"][t], False, False) for t in range(13)])
    wires = circ["wires"].copy()
    perm_idx = circ["perm_idx"]
    dw, dsel, dpi, didx = (w.alloc(a.nbytes).upload(a) for a in (wires, sel_ev, circ["pub_input"], perm_idx))
    try:
        chk = lambda idx=didx.ptr: w.circuit_check_dev(dw.ptr, dsel.ptr, dpi.ptr, idx, n)
        assert chk() == (-1, -1)
        assert chk(None) == (-1, -1)
        g = 357
        bad_sel = sel_ev.copy()
        bad_sel[11, g, 0] ^= 1
        dsel.upload(bad_sel)
        assert chk() == (g, -1)
        dsel.upload(sel_ev)
        # one wire value changed: its gate fails, and the cycle through that position breaks
        i, g = 2, 611
        bad = wires.copy()
        bad[i, g] = oracle.rand_fr(cid, 77, 1)[0]
        dw.upload(bad)
        flat = bad.reshape(5 * n, 4)
        viol = np.flatnonzero((flat != flat[perm_idx.astype(np.int64)]).any(axis=1))
        want_copy = int(viol[0]) if viol.size else -1
        assert want_copy >= 0 or perm_idx[i * n + g] == i * n + g
        assert chk() == (g, want_copy)
        assert chk(None) == (g, -1)
    finally:
        for b in (dw, dsel, dpi, didx):
            b.free()


def _chain_circuit(cid: int, num_gates: int, seed: int, num_io: int = 2) -> CI.Circuit:
    """A hand-written circuit: gates out_t = x_t^5 + x_t * y_t + c_t (q_hash[0], q_mul[0], q_c, q_o), x_{t+1} = out_t (cycles between
    columns 4 and 0), num_io IO gates at gates 0 .. num_io carrying public outputs (e = out, q_o = 1, PI - e = 0); variable 0 is zero."""
    from oracle import prover_ref as P
    f = P.CURVE_OBJ[cid].fr
    p = f.p
    rs = np.random.RandomState(seed)
    T = num_gates - num_io
    ys = [int(v) for v in rs.randint(1, 1 << 62, size=T)]
    cs = [int(v) for v in rs.randint(0, 1 << 62, size=T)]
    # variables: 0 zero, 1 x_0, 2 + 2t y_t, 3 + 2t out_t
    vals = [0, int(rs.randint(1, 1 << 62))]
    x = vals[1]
    outs = []
    for t in range(T):
        out = (pow(x, 5, p) + x * ys[t] + cs[t]) % p
        vals += [ys[t], out]
        outs.append(out)
        x = out
    num_vars = len(vals)
    wv = np.zeros((5, num_gates), dtype=np.uint32)
    one = P.fr_to_limbs(f, 1)
    sel = np.zeros((13, num_gates, 4), dtype=np.uint64)
    pub_vars = [3 + 2 * (T - 1), 3 + 2 * (T // 2)]
    for j in range(num_io):
        wv[4, j] = pub_vars[j]
        sel[10, j] = one
    for t in range(T):
        j = num_io + t
        wv[0, j] = 1 if t == 0 else 3 + 2 * (t - 1)
        wv[1, j] = 2 + 2 * t
        wv[4, j] = 3 + 2 * t
        sel[6, j] = one               # q_hash[0]: a^5
        sel[4, j] = one               # q_mul[0]: ab
        sel[10, j] = one              # q_o
    sel[11, num_io:] = P.fr_vec_to_limbs(f, cs)
    witness = P.fr_vec_to_limbs(f, vals)
    pub = P.fr_vec_to_limbs(f, [vals[v] for v in pub_vars[:num_io]])
    return CI.Circuit(wv, witness, sel, pub)


def _trapdoor_key(w, n: int):
    f = _fr.FIELDS[w.curve_name]
    key_size = ((n + 3 + 31) >> 5) << 5
    q = 64 if w.curve_name == "bn254" else 96
    ck = w.alloc(key_size * q)
    w.memset_dev(ck.ptr, 0, key_size * q)
    w.synth_srs(f.to_limbs(TAU), n + 3, ck.ptr)
    w.init_dev(ck.ptr, key_size, n, 8 * n)
    return ck


@pytest.mark.parametrize("curve,cid,log_n", [("bn254", 0, 10), ("bls12_381", 1, 10), ("bn254", 0, 20)], ids=["bn254-log10", "bls12_381-log10", "bn254-log20"])
def test_hand_written_circuit_proves_and_verifies(gpu_workers, oracle, curve, cid, log_n):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    w = gpu_workers(curve)
    n = 1 << log_n
    circ = _chain_circuit(cid, n - 37, seed=log_n + cid).pad(0)
    assert circ.num_gates == n
    inst = CI.preprocess(w, circ)
    ck = _trapdoor_key(w, n)
    pv = Prover(w, log_n)
    bad = dsel = None
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        assert np.array_equal(pub, circ.public_inputs)
        blinders = dict(wires=oracle.rand_fr(cid, 90, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 91, 3))
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        V.verify(B.CURVES[curve], vk, pub, proof, TAU, transcript=PlonkTranscript(curve))
        # a padding gate's wire 0 set to 1: its gate still holds (zero selectors), its copy constraint with the zero variable does not
        bad = w.alloc(5 * n * 32)
        w.memcpy_d2d(bad.ptr, inst.d_wires.ptr, 5 * n * 32)
        w.write_bytes(bad.ptr + (n - 1) * 32, _fr.FIELDS[curve].to_limbs(1))
        dsel = w.alloc(circ.selector_evals.nbytes).upload(circ.selector_evals)
        perm_idx = inst.d_idx.download((5 * n,))
        pred = int(np.flatnonzero(perm_idx == n - 1)[0])              # the position whose cycle successor was edited
        assert w.circuit_check_dev(bad.ptr, dsel.ptr, inst.d_pi.ptr, inst.d_idx.ptr, n) == (-1, min(pred, n - 1))
        wev_bad = [bad.ptr + i * n * 32 for i in range(5)]
        proof_bad = pv.prove_dev(wev_bad, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub), check_degree=False)
        with pytest.raises(V.VerificationError):
            V.verify(B.CURVES[curve], vk, pub, proof_bad, TAU, transcript=PlonkTranscript(curve))
    finally:
        pv.close()
        inst.close()
        ck.free()
        for b in (bad, dsel):
            if b is not None:
                b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_invalid_arguments_are_reported(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    n = 64
    k = wire_subset_separators(_fr.FIELDS[curve], 1)
    wv = np.random.RandomState(1).randint(0, 100, size=(5, n)).astype(np.uint32)
    wv[3, 9] = 100                                            # == num_vars
    dv, did, didx, dsig = w.alloc(wv.nbytes).upload(wv), w.alloc(5 * n * 32), w.alloc(5 * n * 8), w.alloc(5 * n * 32)
    dwit, dw = w.alloc(100 * 32), w.alloc(5 * n * 32)
    dsel = w.alloc(13 * n * 32)                               # circuit_check_dev reads 13 selector vectors: a 5n buffer in their place is read past its end
    try:
        with pytest.raises(PlonkError) as e:
            w.circuit_permutation_dev(dv.ptr, n, 100, k, did.ptr, didx.ptr, dsig.ptr)
        assert e.value.code == -1 and "wire 3 of gate 9" in str(e.value)
        with pytest.raises(PlonkError) as e:
            w.circuit_witness_dev(dv.ptr, n, dwit.ptr, 100, dw.ptr)
        assert e.value.code == -1 and "wire 3 of gate 9" in str(e.value)
        with pytest.raises(PlonkError) as e:
            w.circuit_permutation_dev(dv.ptr, 48, 101, k, did.ptr, didx.ptr, dsig.ptr)
        assert e.value.code == -2
        with pytest.raises(PlonkError) as e:
            w.circuit_witness_dev(dv.ptr, 48, dwit.ptr, 101, dw.ptr)
        assert e.value.code == -2
        with pytest.raises(PlonkError) as e:
            w.circuit_check_dev(dw.ptr, dw.ptr, dw.ptr, None, 48)
        assert e.value.code == -2
        with pytest.raises(PlonkError) as e:
            w.circuit_permutation_dev(dv.ptr, n, 101, k, None, didx.ptr, dsig.ptr)
        assert e.value.code == -1
        with pytest.raises(PlonkError) as e:
            w.circuit_witness_dev(None, n, dwit.ptr, 101, dw.ptr)
        assert e.value.code == -1
        with pytest.raises(PlonkError) as e:
            w.circuit_check_dev(None, dw.ptr, dw.ptr, None, n)
        assert e.value.code == -1
        bad_idx = np.arange(5 * n, dtype=np.uint64)
        bad_idx[200] = 5 * n
        didx.upload(bad_idx)
        with pytest.raises(PlonkError) as e:
            w.circuit_check_dev(dw.ptr, dsel.ptr, did.ptr, didx.ptr, n)
        assert e.value.code == -1 and "perm_idx[200]" in str(e.value)
        # the context still works
        _, perm_idx, _ = run_permutation(w, wv, 101, k)
        assert np.array_equal(perm_idx, ref_perm_idx(wv))
    finally:
        for b in (dv, did, didx, dsig, dwit, dw, dsel):
            b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_preprocess_is_deterministic(gpu_workers, oracle, curve, cid):
    w = gpu_workers(curve)
    n = 1 << 12
    rs = np.random.RandomState(40 + cid)
    nv = n // 3
    wv = rs.randint(0, nv, size=(5, n))
    wv[:, rs.permutation(n)[: n // 2]] = 0
    circ = CI.Circuit(wv, oracle.rand_fr(cid, 41, nv), oracle.rand_fr(cid, 42, 13 * n).reshape(13, n, 4), oracle.rand_fr(cid, 43, 3))
    outs = []
    for _ in range(2):
        inst = CI.preprocess(w, circ, check=False)
        try:
            outs.append(inst.download())
        finally:
            inst.close()
    for name in outs[0]:
        assert outs[0][name].tobytes() == outs[1][name].tobytes(), name
    assert np.array_equal(outs[0]["perm_idx"], ref_perm_idx(wv))
    with pytest.raises(CI.UnsatisfiedCircuit) as e:
        CI.preprocess(w, circ).close()
    assert e.value.gate >= 0
