"""KZG openings checked without the trapdoor (plonk_kzg_pairs_dev, csrc/kzg_kernels.hpp; kzg.verify / kzg.batch_verify through the batch
verifier's fold).  The honest openings are made by the reference of tests/kzg_ref.py — commitments [f(tau)] G and proofs
[(f(tau) - y) / (tau - z)] G by the oracle's group arithmetic —, never by the library under test.

The defect sweep runs every case the scheme has to tell apart (five defects x four position sets x K = 8 and 65).  Its cost is the host's
pairing check, 0.2 - 0.3 s each: a batch with b bad openings costs up to 1 + 2 b log2 P of them, and "everywhere" at K = 65 tests all 135
nodes that have a leaf below them — that one parameter takes tens of seconds, the others a few."""
import math
import random

import numpy as np
import pytest

from distributed_plonk_amd import kzg
from distributed_plonk_amd import verifier as VF
from tests import kzg_ref as R
from tests.kzg_ref import CURVES
from tests.test_gpu_batch_verify_edges import _off_curve, _outside_subgroup, _over

pytestmark = pytest.mark.gpu

DEFECTS = ["y_plus_1", "z_plus_1", "pi_swapped", "C_swapped", "pi_infinity"]
_POOL, _KEY = {}, {}


def open_key(curve):
    if curve not in _KEY:
        _KEY[curve] = VF.OpenKey.from_trapdoor(curve, R.TAU)
    return _KEY[curve]


def pool(curve, cid):
    """65 honest (commitment, Opening, z, y) of four polynomials (degrees 0, 1, 4 and 12) at distinct random points and at 0, 1 and p - 1;
    neighbours in the list belong to different polynomials, so swapping pi or C between them breaks both.  Made once per curve."""
    if curve not in _POOL:
        p = R.FR[curve]
        rng = random.Random(0x6b7a67 + cid)
        polys = [[rng.randrange(1, p) for _ in range(n)] for n in (1, 2, 5, 13)]
        comms = [R.commitment(curve, cid, f) for f in polys]
        zs = [0, 1, p - 1] + [rng.randrange(2, p - 1) for _ in range(62)]
        items = []
        for i, z in enumerate(zs):
            f = polys[1 + i % 3] if i != 5 else polys[0]                   # item 5: the constant polynomial, pi = infinity
            y = R.horner(curve, f, z)
            op = kzg.Opening(R.to_limbs(curve, z), R.to_limbs(curve, y), R.xy_of(R.proof(curve, cid, f, z)))
            items.append((comms[polys.index(f)], op, z, y))
        assert not items[5][1].proof_xy.any() and all(it[1].proof_xy.any() for i, it in enumerate(items) if i != 5)
        _POOL[curve] = items
    return _POOL[curve]


def batch(curve, cid, K):
    """K honest openings of the pool; from K = 3 on, one of them is there twice.  The constant polynomial's opening stays out of the first
    8: the defect "pi = infinity" needs honest proofs that are not."""
    items = pool(curve, cid)
    order = [0, 1, 2, 3, 4, 6, 7, 8, 5] + list(range(9, 65))
    sel = [items[order[i]] for i in range(K)]
    if K >= 3:
        sel[K - 1] = sel[1]
    return [it[0] for it in sel], [it[1] for it in sel]


def defective(curve, comms, ops, defect, where):
    comms, ops = list(comms), list(ops)
    K = len(ops)
    src_c, src_o = list(comms), list(ops)
    for j in where:
        o = ops[j]
        if defect == "y_plus_1":
            ops[j] = o._replace(value=R.to_limbs(curve, R.from_limbs(curve, o.value) + 1))
        elif defect == "z_plus_1":
            ops[j] = o._replace(point=R.to_limbs(curve, R.from_limbs(curve, o.point) + 1))
        elif defect == "pi_swapped":
            other = next(i for i in range(j + 1, j + K + 1) if not np.array_equal(src_o[i % K].proof_xy, o.proof_xy)) % K
            ops[j] = o._replace(proof_xy=src_o[other].proof_xy)
        elif defect == "C_swapped":
            other = next(i for i in range(j + 1, j + K + 1) if not np.array_equal(src_c[i % K][0], src_c[j][0])) % K
            comms[j] = src_c[other]
        elif defect == "pi_infinity":
            assert o.proof_xy.any()
            ops[j] = o._replace(proof_xy=np.zeros_like(o.proof_xy))
    return comms, ops


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("K", [1, 2, 3, 64, 65])
def test_honest_batches_take_one_pairing_check(gpu_workers, curve, cid, K):
    w = gpu_workers(curve)
    comms, ops = batch(curve, cid, K)
    st = {}
    assert kzg.batch_verify(w, open_key(curve), comms, ops, seed=K, stats=st) == [True] * K
    assert st["pairing_checks"] == 1 and st["status"] == [0] * K and set(st["kernel_ms"]) == {"verify", "tree"}
    assert kzg.batch_verify(w, open_key(curve), comms, ops) == [True] * K                 # rho from `secrets`


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("K", [8, 65])
@pytest.mark.parametrize("defect", DEFECTS)
def test_defects_are_found_where_they_are(gpu_workers, curve, cid, K, defect):
    w = gpu_workers(curve)
    comms, ops = batch(curve, cid, K)
    P = VF.tree_leaves(K)
    if defect == "C_swapped" and K == 8:
        assert len({c[0].tobytes() for c in comms}) == 3
    for where in ([0], [K - 1], [3, 4], list(range(K))):
        if defect in ("pi_infinity", "z_plus_1") and K == 65:
            # position 8 opens the constant polynomial: its honest pi IS infinity, and its opening holds at every z — neither is a defect there
            where = [j for j in where if ops[j].proof_xy.any()]
        bc, bo = defective(curve, comms, ops, defect, where)
        st = {}
        verdict = kzg.batch_verify(w, open_key(curve), bc, bo, seed=len(where), stats=st)
        assert verdict == [j not in where for j in range(K)], (defect, where)
        assert st["status"] == [0] * K
        assert st["pairing_checks"] <= 1 + 2 * len(where) * max(int(math.log2(P)), 1), (defect, where, st["pairing_checks"])


def pairs_on_device(w, curve, comms, ops, rho):
    K = len(ops)
    n64 = w.q64
    with w.scope() as s:
        d_recs = s.upload(np.stack([kzg.opening_record(curve, c, o) for c, o in zip(comms, ops)]))
        d_rho, d_out, d_st = s.upload(rho), s.alloc(K * 4 * n64 * 8), s.alloc(K * 4)
        w.memset_dev(d_out.ptr, 0xA5, K * 4 * n64 * 8)
        w.kzg_pairs_dev(K, d_recs.ptr, d_rho.ptr, VF.g1_generator(curve), d_out.ptr, d_st.ptr)
        return d_out.download((K, 2, 2 * n64)), d_st.download((K,), dtype=np.uint32)


def expected_pair(curve, cid, comm, op, rho):
    """[rho B, rho A] by the oracle's group arithmetic: A = pi, B = C + z pi - y G."""
    pi = (op.proof_xy, not op.proof_xy.any())
    z, y = R.from_limbs(curve, op.point), R.from_limbs(curve, op.value)
    from oracle import oracle as O
    b = R.lincomb(curve, cid, [(rho, comm), (rho * z, pi), (-rho * y, (O.generator(cid), False))])
    a = R.lincomb(curve, cid, [(rho, pi)])
    return R.xy_of(b), R.xy_of(a)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_pairs_against_the_integers(gpu_workers, curve, cid):
    """Each leaf pair is the reference's, and with the trapdoor tau * (rho A) = rho B for every leaf and for the root of the tree."""
    w = gpu_workers(curve)
    K = 10                                                 # holds the constant polynomial's opening (pi = infinity, position 8) and a duplicate
    comms, ops = batch(curve, cid, K)
    assert not ops[8].proof_xy.any()
    rng = random.Random(17)
    rhos = [1, R.FR[curve] - 1] + [rng.randrange(1, R.FR[curve]) for _ in range(K - 2)]
    pts, st = pairs_on_device(w, curve, comms, ops, R.vec_to_limbs(curve, rhos))
    assert not st.any()
    for j in range(K):
        want_b, want_a = expected_pair(curve, cid, comms[j], ops[j], rhos[j])
        assert np.array_equal(pts[j, 0], want_b) and np.array_equal(pts[j, 1], want_a), j
    tree = VF.g1_sum_tree(w, pts)
    for node in [0] + [VF.tree_leaves(K) - 1 + j for j in range(K)]:
        b, a = tree[node]
        assert np.array_equal(R.xy_of(R.lincomb(curve, cid, [(R.TAU, (a, not a.any()))])), b), node


@pytest.mark.parametrize("curve,cid", CURVES)
def test_status_words(gpu_workers, curve, cid):
    """1 for C or pi off the curve, 8 for a coordinate, z, y or rho that is not canonical, 2 (BLS12-381) for a curve point outside the
    r-subgroup; such an opening gets (0, 0) twice and a false verdict, the others their pairs and a true one."""
    from oracle import bigint_ref as B
    w = gpu_workers(curve)
    K = 24
    comms, ops = batch(curve, cid, K)
    q, r, nq = B.CURVES[curve].fq.p, R.FR[curve], w.q64
    expect = [0] * K

    def coord(xy, which, ones=False):
        xy = np.array(xy, dtype=np.uint64).copy()
        xy[which * nq:(which + 1) * nq] = np.full(nq, 2 ** 64 - 1, dtype=np.uint64) if ones else _over(xy[which * nq:(which + 1) * nq], q)
        return xy

    comms[0], expect[0] = _off_curve(curve, comms[0]), 1
    ops[2], expect[2] = ops[2]._replace(proof_xy=_off_curve(curve, (ops[2].proof_xy, False))[0]), 1
    comms[3], expect[3] = (coord(comms[3][0], 0), False), 8
    comms[4], expect[4] = (coord(comms[4][0], 1, ones=True), False), 8
    ops[6], expect[6] = ops[6]._replace(proof_xy=coord(ops[6].proof_xy, 1)), 8
    ops[7], expect[7] = ops[7]._replace(point=_over(ops[7].point, r)), 8
    ops[9], expect[9] = ops[9]._replace(value=_over(ops[9].value, r)), 8
    ops[10], expect[10] = ops[10]._replace(value=np.full(4, 2 ** 64 - 1, dtype=np.uint64)), 8
    comms[11], ops[11], expect[11] = _off_curve(curve, comms[11]), ops[11]._replace(point=_over(ops[11].point, r)), 1 | 8
    ops[K - 1], expect[K - 1] = ops[K - 1]._replace(point=R.plain_limbs(r)), 8                # lane K - 1: z = r itself
    if curve == "bls12_381":
        rng = random.Random(381)
        (p1, hp1), (p2, _) = _outside_subgroup(rng), _outside_subgroup(rng)
        comms[13], expect[13] = p1, 2
        ops[14], expect[14] = ops[14]._replace(proof_xy=p2[0]), 2
        comms[15] = hp1                                    # the cofactor multiple is in the subgroup: status 0, and a false verdict from the pairing
    rho = R.vec_to_limbs(curve, [random.Random(5).randrange(1, r) for _ in range(K)])
    rho[16], expect[16] = _over(rho[16], r), 8

    pts, st = pairs_on_device(w, curve, comms, ops, rho)
    assert [int(x) for x in st] == expect
    for j in range(K):
        if expect[j]:
            assert not pts[j].any(), j
        else:
            want_b, want_a = expected_pair(curve, cid, comms[j], ops[j], R.from_limbs(curve, rho[j]))
            assert np.array_equal(pts[j, 0], want_b) and np.array_equal(pts[j, 1], want_a), j
    stats = {}
    verdict = kzg.batch_verify(w, open_key(curve), comms, ops, stats=stats, _rho=rho)
    assert stats["status"] == expect
    assert verdict == [e == 0 and not (curve == "bls12_381" and j == 15) for j, e in enumerate(expect)]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_edge_cases(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    key = open_key(curve)
    items = pool(curve, cid)
    const_c, const_op = items[5][0], items[5][1]                                          # honest pi = infinity
    assert kzg.verify(w, key, const_c, const_op)
    zero_c = R.commitment(curve, cid, [0, 0, 0])
    zero_op = kzg.Opening(R.to_limbs(curve, 1234), R.to_limbs(curve, 0), np.zeros(2 * w.q64, np.uint64))
    assert zero_c[1] and kzg.verify(w, key, zero_c, zero_op)                              # C = infinity, y = 0
    assert not kzg.verify(w, key, zero_c, zero_op._replace(value=R.to_limbs(curve, 1)))
    for c, o in ((items[0][0], items[0][1]), (items[0][0], items[0][1]._replace(value=items[1][1].value))):
        one = R.to_limbs(curve, 1)[None, :]
        st1, st2 = {}, {}
        assert kzg.verify(w, key, c, o, stats=st1) == kzg.batch_verify(w, key, [c], [o], stats=st2, _rho=one)[0]
        assert st1["pairing_checks"] == st2["pairing_checks"] == 1
    calls = []
    real = w.kzg_pairs_dev
    w.kzg_pairs_dev = lambda *a: calls.append(a) or real(*a)
    try:
        st = {}
        assert kzg.batch_verify(w, key, [], [], stats=st) == [] and not calls and st["pairing_checks"] == 0
        assert kzg.verify(w, key, items[1][0], items[1][1]) and len(calls) == 1
    finally:
        del w.kzg_pairs_dev
    other = "bls12_381" if curve == "bn254" else "bn254"
    with pytest.raises(ValueError):
        kzg.batch_verify(w, open_key(other), [items[0][0]], [items[0][1]])
    with pytest.raises(ValueError):
        kzg.batch_verify(w, key, [], [items[0][1]])
