"""Rescue on the device (csrc/rescue_kernels.hpp behind plonk_rescue_permute_dev / plonk_rescue_merkle_dev and distributed_plonk_amd/rescue.py)
against the pure-Python reference tests/rescue_ref.py, element for element: the permutation at counts around the wave and workgroup sizes
with the fixtures' edge states (zero meets 0^(1/5), r - 1 a full-width reduction), determinism, count 0, trees of 1, 2, 8 and 32 leaves
with their paths, the level kernel against the permutation kernel, the argument errors — and the whole pipeline: a tree built on the
device, m = 4 memberships proved against its public root in a circuit of the builder's merkle_root, solved on the device, proved, verified.

tests/test_hostemu_rescue.py runs a selection of this file on the CPU."""
import json
import os
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import circuit as CI
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import rescue as RS
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.prover import Prover
from distributed_plonk_amd.transcript import PlonkTranscript
from tests import rescue_ref as R
from tests.test_gpu_solve import TAU, trapdoor_key

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [("bn254", 0), ("bls12_381", 1)]


def to_limbs(curve, values) -> np.ndarray:
    f = _fr.FIELDS[curve]
    raw = b"".join((int(x) % f.p * f.R % f.p).to_bytes(32, "little") for x in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def from_limbs(curve, limbs) -> list:
    f = _fr.FIELDS[curve]
    return [int.from_bytes(row.tobytes(), "little") * f.R_inv % f.p for row in np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)]


_states = {}


def states_and_images(curve):
    """257 states — the 8 of the fixture (all-zero, all r - 1, (1, 0, 0, 0), 5 random) first, at the FRONT and again at the END so that every
    count below meets the edge states in its first and last lanes — and their images under the reference, computed once"""
    if curve not in _states:
        with open(os.path.join(ROOT, "tests", "golden", f"rescue_{curve}.json")) as fh:
            g = json.load(fh)
        fixture = [[int(x, 16) for x in pair["in"]] for pair in g["states"]]
        want = {tuple(s): [int(x, 16) for x in pair["out"]] for s, pair in zip(fixture, g["states"])}
        p = R.MODULI[curve]
        rnd = random.Random("gpu rescue " + curve)
        states = fixture + [[rnd.choice([0, 1, p - 1, rnd.randrange(p)]) for _ in range(4)] for _ in range(257 - 8)]
        images = [want.get(tuple(s)) or R.permute(curve, s) for s in states]
        assert images[0] == R.permute(curve, states[0])            # the fixture is the reference's
        _states[curve] = (states, images)
    return _states[curve]


def pick(curve, count):
    """`count` of the 257 states: the edge states first, and (beyond 8) in the last lanes too"""
    states, images = states_and_images(curve)
    idx = list(range(count)) if count <= 8 else list(range(count - 3)) + [0, 1, 2]
    return [states[i] for i in idx], [images[i] for i in idx]


# ---------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", [1, 3, 63, 64, 65, 257], ids=lambda c: f"count{c}")
def test_permutation_matches_the_reference(gpu_workers, curve, cid, count):
    w = gpu_workers(curve)
    states, images = pick(curve, count)
    got = RS.permute(w, RS.RescueParams.default(curve), to_limbs(curve, [x for s in states for x in s]).reshape(count, 4, 4))
    assert got.shape == (count, 4, 4)
    assert from_limbs(curve, got) == [x for s in images for x in s]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_fixture_edge_states(gpu_workers, curve, cid):
    """all-zero, all r - 1 and (1, 0, 0, 0) in one launch, against the committed outputs"""
    w = gpu_workers(curve)
    states, images = pick(curve, 8)
    p = R.MODULI[curve]
    assert states[:3] == [[0] * 4, [p - 1] * 4, [1, 0, 0, 0]]
    got = RS.permute(w, RS.RescueParams.default(curve), to_limbs(curve, [x for s in states for x in s]))
    assert from_limbs(curve, got) == [x for s in images for x in s]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_injected_parameters_are_uploaded_when_they_change(gpu_workers, curve, cid):
    """other tables through RescueParams(curve, mds, round_keys), then the default ones again on the same context"""
    w = gpu_workers(curve)
    p = R.MODULI[curve]
    rnd = random.Random(7 + cid)
    M, K = R.default_params(curve)
    K2 = [[rnd.randrange(p) for _ in range(4)] for _ in range(25)]
    M2 = [list(row) for row in reversed(M)]
    states, images = pick(curve, 3)
    limbs = to_limbs(curve, [x for s in states for x in s])
    got = RS.permute(w, RS.RescueParams(curve, M2, K2), limbs)
    assert from_limbs(curve, got) == [x for s in states for x in R.permute(curve, s, (M2, K2))]
    got = RS.permute(w, RS.RescueParams.default(curve), limbs)
    assert from_limbs(curve, got) == [x for s in images for x in s]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_runs_give_identical_bytes(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    states, _ = pick(curve, 257)
    limbs = to_limbs(curve, [x for s in states for x in s])
    prm = RS.RescueParams.default(curve)
    assert RS.permute(w, prm, limbs).tobytes() == RS.permute(w, prm, limbs).tobytes()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_count_zero_leaves_the_buffer_untouched(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    prm = RS.RescueParams.default(curve)
    data = np.arange(2 * 4 * 4, dtype=np.uint64).reshape(2, 4, 4)
    buf = w.alloc(data.nbytes).upload(data)
    try:
        RS.permute_dev(w, prm, buf.ptr, 0)
        assert np.array_equal(buf.download(data.shape), data)
    finally:
        buf.free()
    assert RS.permute(w, prm, np.zeros((0, 4, 4), dtype=np.uint64)).shape == (0, 4, 4)


# ---------------------------------------------------------------------------------------------- Merkle trees
_trees = {}


def leaves_and_nodes(curve, log_leaves):
    if (curve, log_leaves) not in _trees:
        p = R.MODULI[curve]
        rnd = random.Random(f"tree {curve} {log_leaves}")
        leaves = [rnd.randrange(p) for _ in range(1 << log_leaves)]
        leaves[0], leaves[-1] = 0, p - 1
        _trees[(curve, log_leaves)] = (leaves, R.merkle(curve, leaves))
    return _trees[(curve, log_leaves)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_leaves", [0, 1, 3, 5], ids=lambda v: f"log{v}")
def test_merkle_tree_matches_the_reference_at_every_node(gpu_workers, curve, cid, log_leaves):
    w = gpu_workers(curve)
    leaves, nodes = leaves_and_nodes(curve, log_leaves)
    L = 1 << log_leaves
    tree = RS.MerkleTree(w, RS.RescueParams.default(curve), to_limbs(curve, leaves))
    try:
        assert tree.log_leaves == log_leaves and tree.nodes.shape == (2 * L - 1, 4)
        assert from_limbs(curve, tree.nodes) == nodes
        assert from_limbs(curve, tree.root) == [nodes[0]]
        for i in sorted({0, L // 2 - 1 if L > 2 else 0, L - 1}):
            sibs, bits = tree.path(i)
            assert sibs.shape == (log_leaves, 4) and bits == [(i >> j) & 1 for j in range(log_leaves)]
            assert R.root_from_path(curve, leaves[i], from_limbs(curve, sibs), bits) == nodes[0]
        with pytest.raises(ValueError):
            tree.path(L)
    finally:
        tree.close()


def test_fixture_tree_root(gpu_workers):
    for curve, _ in CURVES:
        with open(os.path.join(ROOT, "tests", "golden", f"rescue_{curve}.json")) as fh:
            g = json.load(fh)
        tree = RS.MerkleTree(gpu_workers(curve), RS.RescueParams.default(curve), to_limbs(curve, [int(x, 16) for x in g["leaves"]]))
        try:
            assert from_limbs(curve, tree.root) == [int(g["root"], 16)]
        finally:
            tree.close()
    with pytest.raises(ValueError):
        RS.MerkleTree(gpu_workers("bn254"), RS.RescueParams.default("bn254"), np.zeros((3, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        RS.MerkleTree(gpu_workers("bn254"), RS.RescueParams.default("bls12_381"), np.zeros((2, 4), dtype=np.uint64))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_level_kernel_agrees_with_the_permutation_kernel(gpu_workers, curve, cid):
    """permute on the rows (left, right, 0, 0) of level 4 gives level 3"""
    w = gpu_workers(curve)
    leaves, _ = leaves_and_nodes(curve, 5)
    prm = RS.RescueParams.default(curve)
    tree = RS.MerkleTree(w, prm, to_limbs(curve, leaves))
    try:
        nodes = tree.nodes
    finally:
        tree.close()
    level4 = nodes[15:31]                               # level l holds the 2^l nodes from 2^l - 1 on
    rows = np.zeros((8, 4, 4), dtype=np.uint64)
    rows[:, 0], rows[:, 1] = level4[0::2], level4[1::2]
    assert np.array_equal(RS.permute(w, prm, rows)[:, 0], nodes[7:15])


# ---------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("curve,cid", CURVES)
def test_argument_errors(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    prm = RS.RescueParams.default(curve).limbs()
    buf = w.alloc(15 * 32)
    try:
        w.memset_dev(buf.ptr, 0, 15 * 32)

        def fails(call, *mentions):
            with pytest.raises(PlonkError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for m in mentions:
                assert m in str(e.value), str(e.value)

        fails(lambda: w.rescue_permute_dev(None, buf.ptr, 1), "plonk_rescue_permute_dev", "null")
        fails(lambda: w.rescue_permute_dev(prm, 0, 1), "plonk_rescue_permute_dev", "null")
        fails(lambda: w.rescue_merkle_dev(None, buf.ptr, 3), "plonk_rescue_merkle_dev", "null")
        fails(lambda: w.rescue_merkle_dev(prm, 0, 3), "plonk_rescue_merkle_dev", "null")
        fails(lambda: w.rescue_merkle_dev(prm, buf.ptr, 32), "plonk_rescue_merkle_dev", "log_leaves = 32")
        # the no-ops return OK and touch nothing; the worker still works
        w.rescue_permute_dev(prm, buf.ptr, 0)
        w.rescue_merkle_dev(prm, buf.ptr, 0)
        assert not buf.download((15, 4)).any()
        w.rescue_merkle_dev(prm, buf.ptr, 3)
        assert from_limbs(curve, buf.download((15, 4))) == R.merkle(curve, [0] * 8)
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------- end to end
def membership_circuit(curve: str, m: int, depth: int):
    b = BD.CircuitBuilder(curve)
    root = b.public_input()
    leaf = b.input(m)
    bits = [b.input(m) for _ in range(depth)]
    sibs = [b.input(m) for _ in range(depth)]
    b.enforce_equal(b.merkle_root(leaf, bits, sibs), root)
    return b.build()


def test_membership_in_a_device_tree_is_built_solved_proved_and_verified(gpu_workers, oracle):
    from oracle import bigint_ref as B
    from oracle import verifier_ref as V
    curve, cid, m, depth = "bn254", 0, 4, 3
    w = gpu_workers(curve)
    prm = RS.RescueParams.default(curve)
    leaves, _ = leaves_and_nodes(curve, depth)
    leaf_limbs = to_limbs(curve, leaves)
    tree = RS.MerkleTree(w, prm, leaf_limbs)
    try:
        root = tree.root.copy()
        members = [0, 3, 6, 7]
        paths = [tree.path(i) for i in members]
    finally:
        tree.close()
    built = membership_circuit(curve, m, depth)
    log_n = built.log_n
    assert built.n == 2048 and built.has_hints
    one, zero = to_limbs(curve, [1])[0], np.zeros(4, dtype=np.uint64)

    def inputs(paths, bit_limbs=None):
        rows = [leaf_limbs[i] for i in members]
        for j in range(depth):
            rows += [(one if pth[1][j] else zero) for pth in paths]
        for j in range(depth):
            rows += [pth[0][j] for pth in paths]
        out = np.stack(rows)
        if bit_limbs is not None:
            out[m] = bit_limbs                          # index bit 0 of the first membership
        return out

    inst = built.preprocess(w, inputs(paths), root.reshape(1, 4), check=True)
    ck = trapdoor_key(w, built.n)
    pv = Prover(w, log_n)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        assert np.array_equal(pub, root.reshape(1, 4))
        blinders = dict(wires=oracle.rand_fr(cid, 94, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, 95, 3))
        proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
        vk = pv.verifying_key()
        assert VF.verify(w, vk, VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
        V.verify(B.CURVES[curve], vk, pub, proof, TAU, transcript=PlonkTranscript(curve))
    finally:
        pv.close()
        inst.close()
        ck.free()
    # one sibling replaced
    bad = [(p[0].copy(), p[1]) for p in paths]
    bad[2][0][1] = leaf_limbs[1]
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, inputs(bad), root.reshape(1, 4), check=True).close()
    # an index bit set to 2
    with pytest.raises(CI.UnsatisfiedCircuit):
        built.preprocess(w, inputs(paths, to_limbs(curve, [2])[0]), root.reshape(1, 4), check=True).close()
    built.close()
    w.trim()
