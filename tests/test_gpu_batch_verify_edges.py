"""The batched device verifier (plonk_verify_batch_dev, csrc/verify_kernels.hpp) on the inputs a forger controls and on the batch shapes
its three kernels split differently, bit for bit against the integer statement oracle/verifier_ref.folded_statement.

tests/test_gpu_batch_verify.py feeds the verifier honest proofs with 3 public inputs in batches of 1, 2, 5 and 64.  Here:

  * a sweep of crafted records (every point G, G / -G alternating, everything at infinity, zero / one / r-1 evaluations, W_z = +-W_zw, a proof
    point equal to a key point or its negative, one point at infinity in each slot, random records, honest proofs) under three verifying keys
    (the real one, one with selector commitments at infinity, one of G and -G only), with 0..13 and n public inputs and domains 2, 4, 2^22
    (and 2^32 where the field has the two-adicity): the six challenges, PI(zeta), r(zeta), E and both output points of EVERY record equal the
    integer statement, for rho = 1, a random rho and rho = r - 1.  The reference has no acceptance check in it, so the suite sees which wrong
    point the device computes for a wrong proof.  No record is skipped: a record the reference cannot evaluate fails the test;
  * batches of 1, 63, 64, 65, 127, 129 and 200 records (partial and second workgroups of all three kernels) with failing records at lanes 0,
    63, 64 and K - 1: every lane as for the same record alone;
  * the status words: exactly 8 for a coordinate >= q, an evaluation, a public input or rho >= r; exactly 1 for a point off the curve in each
    of the 13 slots; 1 | 8 for both; on BLS12-381 exactly 2 for a point of the curve outside the r-subgroup in each slot, and 0 for its
    cofactor multiple.  Failing lanes return (O, O), the others the integer statement, batch_verify accepts exactly the honest lanes.

ST_ZETA_DOMAIN (4) is not exercised: zeta comes out of the Fiat-Shamir hash, and no input is known that makes it an n-th root of unity.

STROBE positions (see test_public_input_counts_reach_the_strobe_wraps, which measures them on the Python transcript).  A challenge is a `prf`
operation, whose begin_op runs the permutation first: every squeeze starts at position 0 and its 64 bytes never cross the 166-byte rate.  What
the public-input count (52 bytes each) does move across the rate is the challenge's framing and the begin_op positions:
  * the framing of the first challenge (label "beta", its length, the prf header) straddles the rate for 10 public inputs on BN254 and for 3
    on BLS12-381;
  * a begin_op of the device's part of the transcript lands on pos == 165 (its first byte wraps, and run_f has to clear pos_begin) for 6, 10,
    13 and 32 public inputs on BN254 and for 7, 8, 10, 13 and 32 on BLS12-381.
"""
import copy
import random

import numpy as np
import pytest

from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import transcript as _tr
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.transcript import PlonkTranscript
from tests.test_gpu_batch_verify import CURVES, TAU, _proved

pytestmark = pytest.mark.gpu

LOG_N = 5
N = 1 << LOG_N
COUNTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 13, N]           # public inputs; 6 and 10 are there for the STROBE wraps (module docstring)
STRADDLE = {"bn254": {10}, "bls12_381": {3}}              # of COUNTS: the first challenge's framing crosses the rate
BEGIN_165 = {"bn254": {6, 10, 13, 32}, "bls12_381": {7, 8, 10, 13, 32}}    # of COUNTS: a device-side begin_op at pos == 165
PARTS = ["degenerate", "coincide", "one_inf", "evals", "random", "honest", "domains"]
BIG_LOG_N = {"bn254": [22], "bls12_381": [22, 32]}        # 2^32 needs a two-adicity of 32: BN254's is 28
NAMES = ["beta", "gamma", "alpha", "zeta", "v", "u"]
_SWEEP, _REF, _POOL, _SINGLE = {}, {}, {}, {}


def _mods(curve):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    return B, V, B.CURVES[curve], _fr.FIELDS[curve]


def _inf(curve):
    return np.zeros(2 * VF._q64(curve), np.uint64), True


def _mul(curve, s):
    B, V, cv, _ = _mods(curve)
    return V.point_limbs(cv, B.scalar_mul(cv, s % cv.fr.p, (cv.gx, cv.gy)))


def _neg(curve, pt):
    B, V, cv, _ = _mods(curve)
    return V.point_limbs(cv, B.affine_neg(cv, V.point_int(cv, pt)))


def _proof(curve, pts, evs):
    f = _fr.FIELDS[curve]
    assert len(pts) == 13 and len(evs) == 10
    e = [f.to_limbs(x) for x in evs]
    return dict(wires_poly_comms=list(pts[:5]), prod_perm_poly_comm=pts[5], split_quot_poly_comms=list(pts[6:11]), opening_proof=pts[11],
                shifted_opening_proof=pts[12], wires_evals=e[:5], wire_sigma_evals=e[5:9], perm_next_eval=e[9])


def _with_point(proof, slot, pt):
    p = copy.copy(proof)
    if slot < 5 or 6 <= slot < 11:
        name, i = ("wires_poly_comms", slot) if slot < 5 else ("split_quot_poly_comms", slot - 6)
        p[name] = list(p[name])
        p[name][i] = pt
    else:
        p[{5: "prod_perm_poly_comm", 11: "opening_proof", 12: "shifted_opening_proof"}[slot]] = pt
    return p


def _with_eval(proof, i, limbs):
    p = copy.copy(proof)
    if i == 9:
        p["perm_next_eval"] = limbs
    else:
        name, j = ("wires_evals", i) if i < 5 else ("wire_sigma_evals", i - 5)
        p[name] = list(p[name])
        p[name][j] = limbs
    return p


def _points_of(proof):
    return list(proof["wires_poly_comms"]) + [proof["prod_perm_poly_comm"]] + list(proof["split_quot_poly_comms"]) \
        + [proof["opening_proof"], proof["shifted_opening_proof"]]


def _over(limbs, modulus):
    """The same residue written non-canonically: value + modulus where the limbs hold it, all-ones limbs otherwise."""
    limbs = np.asarray(limbs, dtype=np.uint64)
    n = limbs.shape[0]
    v = sum(int(x) << (64 * i) for i, x in enumerate(limbs)) + modulus
    if v >> (64 * n):
        return np.full(n, 2 ** 64 - 1, dtype=np.uint64)
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ the sweep
def _sweep(gpu_workers, oracle, curve, cid):
    """(worker, {key name: vk}, [case]) for one curve; built once.  A case: label, part, vk (key name), pub [m, 4], proof, honest."""
    if curve not in _SWEEP:
        B, V, cv, f = _mods(curve)
        w, vk, pub, proofs = _proved(gpu_workers, oracle, curve, cid, log_n=LOG_N, nproofs=3, seed=3)
        assert vk["domain_size"] == N and len(pub) == 3
        r = f.p
        rng = random.Random(7100 + cid)
        G, O = _mul(curve, 1), _inf(curve)
        NG = _neg(curve, G)
        rp = lambda: _mul(curve, rng.randrange(1, r))
        revs = lambda: [rng.randrange(r) for _ in range(10)]
        R13 = [rp() for _ in range(13)]
        S5 = [rp() for _ in range(5)]
        sparse = dict(vk, selector_comms=[O if i in (6, 7, 8, 9, 12) else c for i, c in enumerate(vk["selector_comms"])])   # no hash, no ecc gates
        keys = dict(real=vk, sparse=sparse, gneg=dict(vk, selector_comms=[G] * 13, sigma_comms=[NG] * 5))
        for log_n in [1, 2] + BIG_LOG_N[curve]:           # the statement needs no real circuit: any points, any k
            keys[f"dom{log_n}"] = dict(domain_size=1 << log_n, k=[f.to_limbs(x) for x in [1] + [rng.randrange(2, r) for _ in range(4)]],
                                       selector_comms=list(R13), sigma_comms=list(S5))
        cases = []

        def add(part, label, vkname, m, pts, evs, edge_pub=False, proof=None, pub_limbs=None):
            if pub_limbs is None:
                pub_limbs = f.vec_to_limbs([rng.choice((0, r - 1)) if edge_pub else rng.randrange(r) for _ in range(m)])
            cases.append(dict(label=f"{part}/{label}/{vkname}/{m}", part=part, vk=vkname, pub=pub_limbs,
                              proof=proof if proof is not None else _proof(curve, pts, evs), honest=proof is not None))

        shapes = [("all_G", [G] * 13, revs()), ("G_negG", [G if i % 2 == 0 else NG for i in range(13)], revs()), ("all_inf", [O] * 13, revs()),
                  ("evals_0", R13, [0] * 10), ("evals_r-1", R13, [r - 1] * 10), ("evals_1", R13, [1] * 10)]
        for si, (name, pts, evs) in enumerate(shapes):
            for ci, m in enumerate([0, 1, 3, 7]):
                add("degenerate", name, ("real", "gneg")[(si + ci) % 2], m, pts, evs, edge_pub=ci % 2 == 1)
        P = rp()
        sub = lambda changes: [changes.get(i, p) for i, p in enumerate(R13)]
        add("coincide", "Wz=Wzw", "real", 3, sub({12: R13[11]}), revs())
        add("coincide", "Wz=-Wzw", "real", 3, sub({12: _neg(curve, R13[11])}), revs())
        add("coincide", "all_P", "real", 3, [P] * 13, revs())
        add("coincide", "key_points", "real", 3, sub({0: vk["selector_comms"][0], 11: vk["sigma_comms"][4]}), revs())
        add("coincide", "neg_key_points", "real", 3, sub({0: _neg(curve, vk["selector_comms"][0]), 5: _neg(curve, vk["sigma_comms"][4])}), revs())
        for slot in range(13):
            add("one_inf", f"slot{slot}", ("real", "sparse")[slot % 2], COUNTS[slot % len(COUNTS)], sub({slot: O}), revs(), edge_pub=slot % 3 == 2)
        special = [0, 1, 2, r - 1, r - 2]
        for i, vkname in enumerate(["real", "sparse", "gneg"]):
            add("evals", f"mix{i}", vkname, 3, R13, [special[(i + j) % 5] if j % 3 != 2 else rng.randrange(r) for j in range(10)])
        for i in range(16):
            m = 3 if i in (0, 3, 6, 9, 15) else {13: 6, 14: 10}.get(i, COUNTS[i % len(COUNTS)])
            add("random", f"rec{i}", ("real", "sparse", "gneg")[i % 3], m, [rp() for _ in range(13)], revs(), edge_pub=i % 4 == 1)
        for i, pr in enumerate(proofs):
            add("honest", f"proof{i}", "real", 3, None, None, proof=pr, pub_limbs=np.asarray(pub, dtype=np.uint64))
        for log_n in [1, 2] + BIG_LOG_N[curve]:
            m = {1: 2, 2: 3}.get(log_n, 5)                # 2 public inputs on a domain of 2: the whole domain
            add("domains", "all_G", f"dom{log_n}", m, [G] * 13, revs())
            add("domains", "random", f"dom{log_n}", m, S5 + R13[:8], revs(), edge_pub=True)
        assert len({c["label"] for c in cases}) == len(cases)
        assert {c["pub"].shape[0] for c in cases if not c["vk"].startswith("dom")} == set(COUNTS)
        _SWEEP[curve] = (keys, cases)
    return (gpu_workers(curve),) + _SWEEP[curve]


PART_SIZES = dict(degenerate=24, coincide=5, one_inf=13, evals=3, random=16, honest=3)


def _reference(curve, keys, case):
    """Challenges and the integer statement of one case; computed once.  Nothing is caught: a case the reference cannot evaluate fails."""
    key = (curve, case["label"])
    if key not in _REF:
        B, V, cv, _ = _mods(curve)
        vk = keys[case["vk"]]
        ch = V.derive_challenges(PlonkTranscript(curve), vk, list(case["pub"]), case["proof"])
        s = V.folded_statement(cv, vk, case["pub"], case["proof"], ch)
        _REF[key] = dict(ch=ch, pi_eval=s["pi_eval"], lin_eval=s["lin_eval"], batch_eval=s["batch_eval"], A=s["A"], Bp=s["Bp"])
    return _REF[key]


def _scaled(curve, ref, rho):
    """[limbs of rho * Bp, limbs of rho * A]: the layout of the device's output pair."""
    B, V, cv, _ = _mods(curve)
    return [V.point_limbs(cv, B.scalar_mul(cv, rho, ref[k]))[0] for k in ("Bp", "A")]


def _rho_limbs(curve, rhos):
    return np.stack([_fr.FIELDS[curve].to_limbs(x) for x in rhos])


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("curve,cid", CURVES)
def test_sweep_matches_the_integer_statement(gpu_workers, oracle, curve, cid, part):
    B, V, cv, f = _mods(curve)
    w, keys, all_cases = _sweep(gpu_workers, oracle, curve, cid)
    cases = [c for c in all_cases if c["part"] == part]
    assert len(cases) == PART_SIZES.get(part, 2 * (2 + len(BIG_LOG_N[curve])))
    r = f.p
    rng = random.Random(51 + cid)
    groups = {}
    for c in cases:
        groups.setdefault((c["vk"], c["pub"].shape[0]), []).append(c)
    compared = 0
    for (vkname, m), group in groups.items():
        vk = keys[vkname]
        pubs, prfs = [c["pub"] for c in group], [c["proof"] for c in group]
        pts, status, dbg = VF.device_verify(w, vk, pubs, prfs, _rho_limbs(curve, [1] * len(group)), debug=True)
        rhos = [rng.randrange(2, r - 1) for _ in group]
        pts_rho, status_rho, _ = VF.device_verify(w, vk, pubs, prfs, _rho_limbs(curve, rhos))
        pts_neg, status_neg, _ = VF.device_verify(w, vk, pubs, prfs, _rho_limbs(curve, [r - 1] * len(group)))
        for j, c in enumerate(group):
            at = c["label"]
            assert status[j] == 0 and status_rho[j] == 0 and status_neg[j] == 0, at
            ref = _reference(curve, keys, c)
            for i, name in enumerate(NAMES):
                assert np.array_equal(dbg[j, i], ref["ch"][name]), (at, name)
            for i, name in enumerate(["pi_eval", "lin_eval", "batch_eval"]):
                assert V.fr_int(cv, dbg[j, 6 + i]) == ref[name], (at, name)
            assert np.array_equal(pts[j, 1], V.point_limbs(cv, ref["A"])[0]), (at, "A")
            assert np.array_equal(pts[j, 0], V.point_limbs(cv, ref["Bp"])[0]), (at, "B")
            for got, rho in ((pts_rho[j], rhos[j]), (pts_neg[j], r - 1)):
                want = _scaled(curve, ref, rho)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (at, "rho", rho)
            if c["honest"]:
                assert B.scalar_mul(cv, TAU, ref["A"]) == ref["Bp"], at
                assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), c["pub"], c["proof"]), at
            compared += 1
    assert compared == len(cases)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_domain_above_the_two_adicity_is_refused(gpu_workers, oracle, curve, cid):
    w, keys, _ = _sweep(gpu_workers, oracle, curve, cid)
    f = _fr.FIELDS[curve]
    assert f.two_adicity == {"bn254": 28, "bls12_381": 32}[curve]
    G = _mul(curve, 1)
    proof = _proof(curve, [G] * 13, [1] * 10)
    one = _rho_limbs(curve, [1])
    pub = [f.vec_to_limbs([5, 6])]
    for log_n, ok in ((f.two_adicity, True), (f.two_adicity + 1, False)):
        vk = dict(keys["dom2"], domain_size=1 << log_n)
        if ok:
            assert VF.device_verify(w, vk, pub, [proof], one)[1][0] == 0
        else:
            with pytest.raises(PlonkError):
                VF.device_verify(w, vk, pub, [proof], one)
    with pytest.raises(PlonkError):
        VF.device_verify(w, dict(keys["dom2"], domain_size=3 << 4), pub, [proof], one)


# ------------------------------------------------------------------------------------------------ the STROBE positions the counts are chosen for
@pytest.mark.parametrize("curve,cid", CURVES)
def test_public_input_counts_reach_the_strobe_wraps(monkeypatch, curve, cid):
    """Measured on the Python transcript (which the sweep pins the device's against): where the operations after the verifying-key state (the
    part the device replays) begin, and where the permutation runs between the "beta" label and its squeeze."""
    _, V, _, f = _mods(curve)
    log = []
    begin_op, run_f, squeeze = _tr.Strobe128._begin_op, _tr.Strobe128._run_f, _tr.Strobe128._squeeze
    monkeypatch.setattr(_tr.Strobe128, "_begin_op", lambda s, flags, more: (None if more else log.append(("begin", s.pos)), begin_op(s, flags, more))[1])
    monkeypatch.setattr(_tr.Strobe128, "_run_f", lambda s: (log.append(("run_f", s.pos)), run_f(s))[1])
    monkeypatch.setattr(_tr.Strobe128, "_squeeze", lambda s, n: (log.append(("squeeze", s.pos)), squeeze(s, n))[1])
    g = (VF.g1_generator(curve), False)
    vk = dict(domain_size=N, k=[f.to_limbs(i + 1) for i in range(5)], selector_comms=[g] * 13, sigma_comms=[g] * 5)
    proof = _proof(curve, [g] * 13, [3] * 10)
    straddle, at_165 = set(), set()
    for m in COUNTS:
        del log[:]
        PlonkTranscript(curve).append_vk_and_pub_input(N, m, vk["k"], vk["selector_comms"], vk["sigma_comms"], [])
        host_ops = len(log)
        del log[:]
        V.derive_challenges(PlonkTranscript(curve), vk, [f.to_limbs(7)] * m, proof)
        dev = log[host_ops:]
        assert {pos for what, pos in dev if what == "squeeze"} == {0}        # a squeeze never crosses the rate
        if any(what == "begin" and pos == 165 for what, pos in dev):
            at_165.add(m)
        first = next(i for i, e in enumerate(dev) if e[0] == "squeeze")
        label = [i for i in range(first) if dev[i][0] == "begin"][-2]         # meta_ad("beta"), then prf
        if ("run_f", _tr._STROBE_R) in dev[label:first]:
            straddle.add(m)
    assert straddle == STRADDLE[curve] and at_165 == BEGIN_165[curve]


# ------------------------------------------------------------------------------------------------ batch shapes and status words
def _off_curve(curve, pt):
    """pt with the lowest bit of x flipped: canonical, and (checked) not on the curve."""
    B, V, cv, _ = _mods(curve)
    xy = np.array(pt[0], dtype=np.uint64).copy()
    xy[0] ^= np.uint64(1)
    q = cv.fq.limbs64
    x, y = (cv.fq.from_mont(B.from_limbs([int(v) for v in xy[i * q:(i + 1) * q]])) for i in (0, 1))
    assert B.from_limbs([int(v) for v in xy[:q]]) < cv.fq.p and not B.on_curve(cv, (x, y))
    return xy, False


def _pool(gpu_workers, oracle, curve, cid):
    """The sweep's records under the real key with 3 public inputs, each with a rho of its own and the integer statement's rho * (Bp, A)."""
    w, keys, cases = _sweep(gpu_workers, oracle, curve, cid)
    if curve not in _POOL:
        r = _fr.FIELDS[curve].p
        pool = [c for c in cases if c["vk"] == "real" and c["pub"].shape[0] == 3]
        assert len(pool) == 17 and sum(c["honest"] for c in pool) == 3
        rng = random.Random(900 + cid)
        rhos = [rng.randrange(2, r) for _ in pool]
        _POOL[curve] = (pool, rhos, [_scaled(curve, _reference(curve, keys, c), rho) for c, rho in zip(pool, rhos)])
    return (w, keys["real"]) + _POOL[curve]


def _bad_records(curve, pool):
    """(proof, expected status): one off the curve, one non-canonical, built from records of the pool."""
    f = _fr.FIELDS[curve]
    a, b = pool[3]["proof"], pool[4]["proof"]
    return [(_with_point(a, 11, _off_curve(curve, _points_of(a)[11])), 1), (_with_eval(b, 9, _over(b["perm_next_eval"], f.p)), 8)]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 127, 129, 200])
@pytest.mark.parametrize("curve,cid", CURVES)
def test_batch_shapes(gpu_workers, oracle, curve, cid, K):
    w, vk, pool, rhos, want = _pool(gpu_workers, oracle, curve, cid)
    single = _SINGLE.setdefault(curve, {})
    bad = single.setdefault("bad", _bad_records(curve, pool))

    def alone(i, proof):                                   # the record of pool slot i (or a bad record in its place) in a batch of one
        key = (i, id(proof))
        if key not in single:
            pts, status, _ = VF.device_verify(w, vk, [pool[i]["pub"]], [proof], _rho_limbs(curve, [rhos[i]]))
            single[key] = (proof, pts[0], int(status[0]))  # the proof is kept alive: its id is the key
        return single[key][1:]

    idx = [i % len(pool) for i in range(K)]
    proofs = [pool[i]["proof"] for i in idx]
    expect = [0] * K
    for n, lane in enumerate(sorted({0, 63, 64, K - 1} & set(range(K)))):
        proofs[lane], expect[lane] = bad[n % 2]
    pts, status, _ = VF.device_verify(w, vk, [pool[i]["pub"] for i in idx], proofs, _rho_limbs(curve, [rhos[i] for i in idx]))
    assert [int(s) for s in status] == expect
    for lane, i in enumerate(idx):
        pts1, status1 = alone(i, proofs[lane])
        assert status1 == expect[lane], lane
        assert np.array_equal(pts[lane], pts1), lane
        if expect[lane]:
            assert not pts[lane].any(), lane
        else:
            assert np.array_equal(pts[lane, 0], want[i][0]) and np.array_equal(pts[lane, 1], want[i][1]), (lane, pool[i]["label"])


def _outside_subgroup(rng):
    """A point of BLS12-381's curve outside the r-subgroup, and its cofactor multiple (inside)."""
    B, V, cv, _ = _mods("bls12_381")
    q, r = cv.fq.p, cv.fr.p
    z = -0xd201000000010000
    h = (z - 1) ** 2 // 3                                  # the cofactor of G1: #E(Fq) = h * r
    assert q % 4 == 3
    while True:
        x = rng.randrange(q)
        rhs = (x * x * x + cv.b) % q
        y = pow(rhs, (q + 1) // 4, q)
        if y * y % q != rhs:
            continue
        P = (x, y)
        if B.scalar_mul(cv, r, P) is B.INF:               # the rare sample inside the subgroup
            continue
        hP = B.scalar_mul(cv, h, P)
        assert hP is not B.INF and B.scalar_mul(cv, r, hP) is B.INF
        return V.point_limbs(cv, P), V.point_limbs(cv, hP)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_status_words(gpu_workers, oracle, curve, cid):
    B, V, cv, f = _mods(curve)
    w, vk, pool, rhos, want = _pool(gpu_workers, oracle, curve, cid)
    w, keys, _ = _sweep(gpu_workers, oracle, curve, cid)
    r, q = f.p, cv.fq.p
    nq = cv.fq.limbs64
    K = 130
    # Lanes with status 0 are honest proofs, but for one crafted record (and, on BLS12-381, one cofactor multiple) at the end: batch_verify's
    # bisection then needs about 2 log2 K of the host's pairing checks (0.2 - 0.3 s each), not 2 log2 K for each wrong record
    honest_idx = [i for i, c in enumerate(pool) if c["honest"]]
    crafted = next(i for i, c in enumerate(pool) if c["label"] == "coincide/Wz=Wzw/real/3")
    idx = [honest_idx[lane % 3] for lane in range(K)]
    idx[K - 2] = crafted
    proofs = [pool[i]["proof"] for i in idx]
    pubs = [pool[i]["pub"] for i in idx]
    rho = _rho_limbs(curve, [rhos[i] for i in idx])
    expect = [0] * K
    points = [[want[i][0], want[i][1]] for i in idx]      # of the lanes with status 0
    free = [0, 63, 64, K - 1] + [lane for lane in range(1, K - 1, 3) if lane not in (63, 64)]     # K - 2 and K - 4 are not among them

    def take():
        lane = free.pop(0)
        return lane, proofs[lane]

    def coord(pt, which, ones=False):                      # x (0) or y (1) of an affine point written as value + q, or as all-ones limbs
        xy = np.array(pt[0], dtype=np.uint64).copy()
        xy[which * nq:(which + 1) * nq] = np.full(nq, 2 ** 64 - 1, dtype=np.uint64) if ones else _over(xy[which * nq:(which + 1) * nq], q)
        return xy, False

    # exactly 8: a coordinate >= q, an evaluation >= r, a public input >= r, rho >= r
    for slot, which, ones in ((0, 0, False), (12, 1, False), (5, 0, True)):
        lane, pr = take()
        proofs[lane], expect[lane] = _with_point(pr, slot, coord(_points_of(pr)[slot], which, ones)), 8
    for i, ones in ((0, False), (9, False), (4, True)):
        lane, pr = take()
        ev = (list(pr["wires_evals"]) + list(pr["wire_sigma_evals"]) + [pr["perm_next_eval"]])[i]
        proofs[lane], expect[lane] = _with_eval(pr, i, np.full(4, 2 ** 64 - 1, dtype=np.uint64) if ones else _over(ev, r)), 8
    for i in (0, 2):
        lane, _ = take()
        pubs[lane] = np.array(pubs[lane], dtype=np.uint64).copy()
        pubs[lane][i] = _over(pubs[lane][i], r)
        expect[lane] = 8
    for ones in (False, True):
        lane, _ = take()
        rho[lane] = np.full(4, 2 ** 64 - 1, dtype=np.uint64) if ones else _over(rho[lane], r)
        expect[lane] = 8
    lane, _ = take()
    rho[lane] = np.array([(r >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)     # rho == r itself
    expect[lane] = 8
    # exactly 1: a point off the curve, in each slot; 1 | 8 with a non-canonical value in another slot
    for slot in range(13):
        lane, pr = take()
        proofs[lane], expect[lane] = _with_point(pr, slot, _off_curve(curve, _points_of(pr)[slot])), 1
    for slot, other in ((2, 7), (12, 0)):
        lane, pr = take()
        pr = _with_point(pr, slot, _off_curve(curve, _points_of(pr)[slot]))
        proofs[lane], expect[lane] = _with_point(pr, other, coord(_points_of(pr)[other], 1)), 1 | 8
    lane, pr = take()
    proofs[lane], expect[lane] = _with_eval(_with_point(pr, 6, _off_curve(curve, _points_of(pr)[6])), 7, _over(pr["wire_sigma_evals"][2], r)), 1 | 8
    if curve == "bls12_381":
        rng = random.Random(381)
        for slot in range(13):                             # exactly 2: on the curve, outside the r-subgroup
            lane, pr = take()
            P, hP = _outside_subgroup(rng)
            proofs[lane], expect[lane] = _with_point(pr, slot, P), 2
            if slot == 3:                                  # the cofactor multiple of the same point passes, with the integer statement's pair
                l2 = K - 4
                case = dict(label=f"status/cofactor/{pool[idx[l2]]['label']}", vk="real", pub=pubs[l2], proof=_with_point(proofs[l2], slot, hP))
                proofs[l2] = case["proof"]
                points[l2] = _scaled(curve, _reference(curve, keys, case), rhos[idx[l2]])
        tor = (np.array(VF._fq_mont(curve, 0) + VF._fq_mont(curve, 2), dtype=np.uint64), False)     # order 3: (0, 2)
        for slot in (0, 12):
            lane, pr = take()
            proofs[lane], expect[lane] = _with_point(pr, slot, tor), 2
    assert K >= 70 and sum(1 for e in expect if e) >= (25 if curve == "bn254" else 40)

    pts, status, _ = VF.device_verify(w, vk, pubs, proofs, rho)
    assert [int(s) for s in status] == expect
    for lane in range(K):
        if expect[lane]:
            assert not pts[lane].any(), lane
        else:
            assert np.array_equal(pts[lane, 0], points[lane][0]) and np.array_equal(pts[lane, 1], points[lane][1]), lane
    st = {}
    verdict = VF.batch_verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pubs, proofs, stats=st, _rho=rho)
    assert st["status"] == expect
    honest = [expect[lane] == 0 and proofs[lane] is pool[idx[lane]]["proof"] and pool[idx[lane]]["honest"] for lane in range(K)]
    assert verdict == honest and sum(honest) >= 70
    assert sum(1 for lane in range(K) if expect[lane] == 0 and not honest[lane]) == (2 if curve == "bls12_381" else 1)
