"""The ternary Rescue accumulator on the device (csrc/rescue_acc_kernels.hpp behind plonk_rescue_acc_build_dev, plonk_rescue_acc_paths_dev and
plonk_circuit_scatter_inputs_dev, distributed_plonk_amd/rescue.py and membership.py) against the pure-Python reference
tests/accumulator_ref.py, element for element: every node of every level, the root and the level counts of trees that are ragged at one and
two levels, cross a wave and a workgroup, and end in chains of 1, 30 and 40 links; the paths and the solver-input layout gathered on the
device; the level kernel against the permutation kernel; the fixtures; determinism; the input scatter; the argument errors; a solve from
device inputs against the same solve from host inputs — and the whole pipeline: a tree on the device, m = 4 memberships gathered, solved,
proved and verified without the witness visiting the host, and four ways to spoil it.

tests/test_hostemu_accumulator.py runs a selection of this file on the CPU."""
import json
import os
import random

import numpy as np
import pytest

from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import rescue as RS
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.membership import membership_circuit
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.transcript import PlonkTranscript
from tests import accumulator_ref as A
from tests.test_gpu_solve import TAU, trapdoor_key

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [("bn254", 0), ("bls12_381", 1)]
# (height, count): one leaf; a ragged and a full group; two levels, ragged and full; (3, 10) ragged at two levels with count mod 3 = 1; (4, 28);
# (5, 65): the leaves across a wave boundary, mod 3 = 2, a chain of 1; (6, 257): across a workgroup; chains of 30 and 40 links, jellyfish's height
TREES = [(1, 1), (1, 2), (1, 3), (2, 4), (2, 9), (3, 10), (4, 28), (5, 65), (6, 257), (32, 4), (40, 1)]


def to_limbs(curve, values) -> np.ndarray:
    f = _fr.FIELDS[curve]
    raw = b"".join((int(x) % f.p * f.R % f.p).to_bytes(32, "little") for x in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def from_limbs(curve, limbs) -> list:
    f = _fr.FIELDS[curve]
    return [int.from_bytes(row.tobytes(), "little") * f.R_inv % f.p for row in np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)]


_refs = {}


def elems_and_levels(curve, height, count):
    """seeded elems with elems[0] = 0 and elems[-1] = r - 1 (count 1: r - 1), and the reference's nodes per level, computed once"""
    key = (curve, height, count)
    if key not in _refs:
        p = A.MODULI[curve]
        rnd = random.Random(f"accumulator {curve} {count}")
        elems = [rnd.randrange(p) for _ in range(count)]
        elems[0], elems[-1] = 0, p - 1
        _refs[key] = (elems, A.acc_nodes(curve, height, elems))
    return _refs[key]


def host_layout(curve, levels, elems, uids) -> list:
    """the (2 + 4 height) x m solver inputs, row-major, as residues, from the reference's paths"""
    paths = [A.acc_path(levels, i) for i in uids]
    vals = list(uids) + [elems[i] for i in uids]
    for j in range(len(levels) - 1):
        vals += [p[0][j] for p in paths] + [p[1][j] for p in paths] + [int(p[2][j] == 0) for p in paths] + [int(p[2][j] == 2) for p in paths]
    return vals


# ---------------------------------------------------------------------------------------------- trees and paths
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("height,count", TREES, ids=[f"h{h}c{c}" for h, c in TREES])
def test_tree_matches_the_reference_at_every_node(gpu_workers, curve, cid, height, count):
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, height, count)
    acc = RS.Accumulator(w, RS.RescueParams.default(curve), to_limbs(curve, elems), height)
    try:
        assert acc.level_counts == [len(l) for l in levels] == A.level_counts(height, count)
        assert acc.level_offsets == [sum(acc.level_counts[:j]) for j in range(height + 1)]
        assert acc.nodes.shape == (sum(len(l) for l in levels), 4)
        for j, want in enumerate(levels):
            assert from_limbs(curve, acc.level(j)) == want, f"level {j}"
        assert from_limbs(curve, acc.root) == levels[-1]
    finally:
        acc.close()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("height,count", [(1, 2), (3, 10), (5, 65), (32, 4)], ids=lambda v: str(v))
def test_paths_and_solver_inputs_match_the_reference(gpu_workers, curve, cid, height, count):
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, height, count)
    root = levels[-1][0]
    uids = sorted({0, count // 2, count - 1})
    acc = RS.Accumulator(w, RS.RescueParams.default(curve), to_limbs(curve, elems), height)
    try:
        for i in uids:
            sib1, sib2, pos = acc.path(i)
            assert sib1.shape == sib2.shape == (height, 4)
            want = A.acc_path(levels, i)
            assert (from_limbs(curve, sib1), from_limbs(curve, sib2), pos) == want
            assert A.root_from_path(curve, i, elems[i], *want) == root
        with pytest.raises(ValueError):
            acc.path(count)
        for sel in (uids, [count - 1] * 3 + uids[::-1]):            # repeated and unordered uids too
            buf = acc.witness_inputs_dev(sel)
            try:
                got = buf.download(((2 + 4 * height) * len(sel), 4))
            finally:
                buf.free()
            assert from_limbs(curve, got) == host_layout(curve, levels, elems, sel)
    finally:
        acc.close()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_level_kernel_agrees_with_the_permutation_kernel(gpu_workers, curve, cid):
    """permute on the rows (x0, x1, x2, 0) of level 0 of the (3, 10) tree, zero beyond its 10 nodes, gives level 1; hash3 is that row's [0]"""
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, 3, 10)
    prm = RS.RescueParams.default(curve)
    acc = RS.Accumulator(w, prm, to_limbs(curve, elems), 3)
    try:
        level0, level1 = acc.level(0).copy(), acc.level(1).copy()
    finally:
        acc.close()
    padded = np.zeros((12, 4), dtype=np.uint64)
    padded[:10] = level0
    rows = np.zeros((4, 4, 4), dtype=np.uint64)
    rows[:, :3] = padded.reshape(4, 3, 4)
    assert np.array_equal(RS.permute(w, prm, rows)[:, 0], level1)
    assert np.array_equal(RS.hash3(w, prm, padded.reshape(4, 3, 4)), level1)
    uid_rows = [[0, i, e] for i, e in enumerate(elems)]
    assert from_limbs(curve, RS.hash3(w, prm, to_limbs(curve, [x for r in uid_rows for x in r]).reshape(10, 3, 4))) == levels[0]


def test_fixture_roots(gpu_workers):
    for curve, _ in CURVES:
        with open(os.path.join(ROOT, "tests", "golden", f"accumulator_{curve}.json")) as fh:
            g = json.load(fh)
        elems = to_limbs(curve, [int(x, 16) for x in g["elems"]])
        for height, root in ((g["height"], g["root"]), (g["tall_height"], g["tall_root"])):
            acc = RS.Accumulator(gpu_workers(curve), RS.RescueParams.default(curve), elems, height)
            try:
                assert from_limbs(curve, acc.root) == [int(root, 16)]
            finally:
                acc.close()
    w = gpu_workers("bn254")
    with pytest.raises(ValueError):
        RS.Accumulator(w, RS.RescueParams.default("bls12_381"), np.zeros((2, 4), dtype=np.uint64), 3)
    for height, count in ((0, 1), (41, 1), (1, 4), (3, 0)):
        with pytest.raises(ValueError):
            RS.Accumulator(w, RS.RescueParams.default("bn254"), np.zeros((count, 4), dtype=np.uint64), height)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_runs_give_identical_bytes(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    elems, _ = elems_and_levels(curve, 5, 65)
    runs = []
    for _ in range(2):
        acc = RS.Accumulator(w, RS.RescueParams.default(curve), to_limbs(curve, elems), 5)
        try:
            buf = acc.witness_inputs_dev([64, 0, 31])
            try:
                runs.append((acc.nodes.tobytes(), buf.download((22 * 3, 4)).tobytes()))
            finally:
                buf.free()
        finally:
            acc.close()
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------------- the input scatter
@pytest.mark.parametrize("curve,cid", CURVES)
def test_scatter_puts_inputs_at_their_ids(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    rnd = random.Random(11 + cid)
    num_vars, k = 1000, 300                             # more than one workgroup of ids
    ids = np.array([0, num_vars - 1] + rnd.sample(range(1, num_vars - 1), k - 2), dtype=np.uint32)
    values = np.arange(1, 4 * k + 1, dtype=np.uint64).reshape(k, 4) * np.uint64(0x9E3779B97F4A7C15)
    before = np.arange(4 * num_vars, dtype=np.uint64).reshape(num_vars, 4)
    d_ids, d_vals, d_wit = w.alloc(ids.nbytes).upload(ids), w.alloc(values.nbytes).upload(values), w.alloc(before.nbytes).upload(before)
    try:
        w.circuit_scatter_inputs_dev(d_ids.ptr, 0, d_vals.ptr, d_wit.ptr, num_vars)        # num_inputs = 0: untouched
        assert np.array_equal(d_wit.download(before.shape), before)
        w.circuit_scatter_inputs_dev(d_ids.ptr, k, d_vals.ptr, d_wit.ptr, num_vars)
        want = before.copy()
        want[ids] = values
        assert np.array_equal(d_wit.download(before.shape), want)
    finally:
        for b in (d_ids, d_vals, d_wit):
            b.free()


# ---------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("curve,cid", CURVES)
def test_argument_errors(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, 3, 10)
    prm = RS.RescueParams.default(curve).limbs()
    el = to_limbs(curve, elems)
    rows = 2 + 4 * 3
    d_el, d_nodes, d_out = w.alloc(el.nbytes).upload(el), w.alloc(17 * 32), w.alloc(32 * 32)        # d_out: 2 x 14 path rows, or 29 variables
    d_uids = w.alloc(16).upload(np.array([3, 10], dtype=np.uint64))
    d_ids = w.alloc(8).upload(np.array([1, 28], dtype=np.uint32))
    try:
        w.memset_dev(d_nodes.ptr, 0, 17 * 32)
        w.memset_dev(d_out.ptr, 0, 32 * 32)

        def fails(call, *mentions):
            with pytest.raises(PlonkError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for m in mentions:
                assert m in str(e.value), str(e.value)

        build, paths, scatter = "plonk_rescue_acc_build_dev", "plonk_rescue_acc_paths_dev", "plonk_circuit_scatter_inputs_dev"
        fails(lambda: w.rescue_acc_build_dev(None, d_el.ptr, 10, 3, d_nodes.ptr), build, "params")
        fails(lambda: w.rescue_acc_build_dev(prm, 0, 10, 3, d_nodes.ptr), build, "d_elems")
        fails(lambda: w.rescue_acc_build_dev(prm, d_el.ptr, 10, 3, 0), build, "d_nodes")
        fails(lambda: w.rescue_acc_build_dev(prm, d_el.ptr, 10, 0, d_nodes.ptr), build, "height = 0")
        fails(lambda: w.rescue_acc_build_dev(prm, d_el.ptr, 10, 41, d_nodes.ptr), build, "height = 41")
        fails(lambda: w.rescue_acc_build_dev(prm, d_el.ptr, 0, 3, d_nodes.ptr), build, "count = 0")
        fails(lambda: w.rescue_acc_build_dev(prm, d_el.ptr, 10, 2, d_nodes.ptr), build, "count = 10", "9")
        assert not d_nodes.download((17, 4)).any()
        fails(lambda: w.rescue_acc_paths_dev(0, 10, 3, d_el.ptr, d_uids.ptr, 1, d_out.ptr), paths, "d_nodes")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, 0, d_uids.ptr, 1, d_out.ptr), paths, "d_elems")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, d_el.ptr, 0, 1, d_out.ptr), paths, "d_uids")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, d_el.ptr, d_uids.ptr, 1, 0), paths, "d_inputs_out")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 0, d_el.ptr, d_uids.ptr, 1, d_out.ptr), paths, "height = 0")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 41, d_el.ptr, d_uids.ptr, 1, d_out.ptr), paths, "height = 41")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 0, 3, d_el.ptr, d_uids.ptr, 1, d_out.ptr), paths, "count = 0")
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 28, 3, d_el.ptr, d_uids.ptr, 1, d_out.ptr), paths, "count = 28", "27")
        w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, d_el.ptr, d_uids.ptr, 0, d_out.ptr)     # m = 0: a no-op
        assert not d_out.download((rows * 2, 4)).any()
        fails(lambda: w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, d_el.ptr, d_uids.ptr, 2, d_out.ptr), paths, "d_uids[1]", "count = 10")
        fails(lambda: w.circuit_scatter_inputs_dev(0, 2, d_el.ptr, d_out.ptr, 28), scatter, "d_input_vars")
        fails(lambda: w.circuit_scatter_inputs_dev(d_ids.ptr, 2, 0, d_out.ptr, 28), scatter, "d_inputs")
        fails(lambda: w.circuit_scatter_inputs_dev(d_ids.ptr, 2, d_el.ptr, 0, 28), scatter, "d_witness")
        fails(lambda: w.circuit_scatter_inputs_dev(d_ids.ptr, 2, d_el.ptr, d_out.ptr, 0), scatter, "num_vars = 0")
        fails(lambda: w.circuit_scatter_inputs_dev(d_ids.ptr, 2, d_el.ptr, d_out.ptr, 28), scatter, "d_input_vars[1]", "num_vars = 28")
        w.circuit_scatter_inputs_dev(d_ids.ptr, 2, d_el.ptr, d_out.ptr, 29)                # id 28 of 29 variables is the last one
        assert np.array_equal(d_out.download((29, 4))[[1, 28]], el[:2])
        # the worker still works
        w.rescue_acc_build_dev(prm, d_el.ptr, 10, 3, d_nodes.ptr)
        assert from_limbs(curve, d_nodes.download((17, 4))) == [x for l in levels for x in l]
        w.rescue_acc_paths_dev(d_nodes.ptr, 10, 3, d_el.ptr, d_uids.ptr, 1, d_out.ptr)
        assert from_limbs(curve, d_out.download((rows, 4))) == host_layout(curve, levels, elems, [3])
    finally:
        for b in (d_el, d_nodes, d_out, d_uids, d_ids):
            b.free()


# ---------------------------------------------------------------------------------------------- solving from device inputs; end to end
HEIGHT, MEMBERS = 3, [0, 4, 8, 9]
_built = {}


def built_circuit(curve):
    if curve not in _built:
        _built[curve] = membership_circuit(curve, HEIGHT, len(MEMBERS))
    return _built[curve]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_solving_from_device_inputs_gives_the_same_witness_bytes(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, HEIGHT, 10)
    built = built_circuit(curve)
    assert built.n == 4096 and built.has_hints
    root = to_limbs(curve, levels[-1])
    host = to_limbs(curve, host_layout(curve, levels, elems, MEMBERS))
    acc = RS.Accumulator(w, RS.RescueParams.default(curve), to_limbs(curve, elems), HEIGHT)
    buf = None
    try:
        buf = acc.witness_inputs_dev(MEMBERS)
        a = built.solve_dev(w, host, root)
        try:
            wa = a.witness()
        finally:
            a.close()
        b = built.solve_dev(w, public_inputs=root, d_inputs=buf.ptr)
        try:
            wb = b.witness()
            assert (a.levels, a.evaluations) == (b.levels, b.evaluations)
        finally:
            b.close()
        assert wa.tobytes() == wb.tobytes()
        assert np.array_equal(wb[built.input_vars], host)
        with pytest.raises(ValueError):
            built.solve_dev(w, host, root, d_inputs=buf.ptr)
    finally:
        if buf is not None:
            buf.free()
        acc.close()
        built.close()


def test_membership_in_a_device_accumulator_is_gathered_solved_proved_and_verified(gpu_workers, oracle):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    curve, cid, m = "bn254", 0, len(MEMBERS)
    w = gpu_workers(curve)
    elems, levels = elems_and_levels(curve, HEIGHT, 10)
    built = built_circuit(curve)
    assert built.n == 4096
    acc = RS.Accumulator(w, RS.RescueParams.default(curve), to_limbs(curve, elems), HEIGHT)
    d_in = None
    try:
        root = acc.root.copy().reshape(1, 4)
        assert from_limbs(curve, root) == levels[-1]
        d_in = acc.witness_inputs_dev(MEMBERS)
        inst = built.preprocess(w, public_inputs=root, check=True, d_inputs=d_in.ptr)
        ck = trapdoor_key(w, built.n)
        pv = Prover(w, built.log_n)
        try:
            pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
            pub = inst.public_inputs()
            assert np.array_equal(pub, root)
            blinders = dict(wires=oracle.rand_fr(cid, 96, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 97, 3))
            proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
            vk = pv.verifying_key()
            assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
            V.verify(B.CURVES[curve], vk, pub, proof, TAU, transcript=PlonkTranscript(curve))
        finally:
            pv.close()
            inst.close()
            ck.free()
        # spoiled inputs, each uploaded and solved from the device like the good ones.  Row t of the layout holds m values; column 1 is uid 4,
        # the middle member of its group at level 0
        good = d_in.download(((2 + 4 * HEIGHT) * m, 4)).reshape(2 + 4 * HEIGHT, m, 4)
        one, two = to_limbs(curve, [1])[0], to_limbs(curve, [2])[0]
        swapped = good.copy()
        swapped[2, 1], swapped[3, 1] = good[3, 1], good[2, 1]                              # sib1 and sib2 of level 0
        assert not np.array_equal(good[2, 1], good[3, 1])
        both = good.copy()
        both[4, 1] = both[5, 1] = one                                                       # is_left = is_right = 1
        flag2 = good.copy()
        flag2[4 + 4, 2] = two                                                               # is_left of level 1, uid 8
        wrong_uid = good.copy()
        wrong_uid[0, 3] = to_limbs(curve, [8])[0]                                           # uid 9's path under uid 8
        for bad in (swapped, both, flag2, wrong_uid):
            d_in.upload(bad)
            with pytest.raises(CI.UnsatisfiedCircuit):
                built.preprocess(w, public_inputs=root, check=True, d_inputs=d_in.ptr).close()
    finally:
        if d_in is not None:
            d_in.free()
        acc.close()
        built.close()
        w.trim()
