"""The Rescue sponge, the counter-mode stream and ElGamal encryption on the host: the properties of the definitions on the pure-Python
reference (tests/elgamal_ref.py) — decrypt after encrypt is the identity, the sponge separates lengths from zero padding and differs from
hash3 on three elements, stream blocks differ by their counter —, and every builder gadget — rescue_sponge, rescue_stream, elgamal_encrypt —
built, solved by the sequential big-integer solver (tests/hint_ref.py) and compared with the reference, with the gate and level counts that
the docstrings and DESIGN.md state; the tampered witnesses the encryption circuit refuses; the layout of elgamal_witness_inputs; the
argument errors.  No GPU.

The gadget circuits live in GADGET_CASES so that tests/test_gpu_elgamal_circuit.py solves the same ones on the device."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import elgamal as EG
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import rescue as RS
from tests import edwards_ref as E
from tests import elgamal_ref as G
from tests import rescue_ref as R
from tests.hint_ref import HintRefSolver
from tests.test_edwards_host import columns

CURVES = list(G.CURVES)
OTHER = {"bn254": "bls12_381", "bls12_381": "bn254"}
PERMUTATION_GATES, PERMUTATION_LEVELS = 148, 37
# per instance, with the default parameters, computed once from the builder; L = 4 for the encryption
ELGAMAL_GATES = {"bn254": 7287, "bls12_381": 7314}
ELGAMAL_LEVELS = {"bn254": 1079, "bls12_381": 1083}
SPONGE_SHAPES = [(L, n_out) for L in (1, 3, 4, 7) for n_out in (1, 3)]


def sponge_gates(L: int) -> int:
    return PERMUTATION_GATES * ((L + 2) // 3) + max(L - 3, 0)


def sponge_levels(L: int) -> int:
    return PERMUTATION_LEVELS + (PERMUTATION_LEVELS + 1) * ((L + 2) // 3 - 1)


# ---------------------------------------------------------------------------------------------- the definitions, on the reference
@pytest.mark.parametrize("curve", CURVES)
def test_decrypt_after_encrypt_is_the_identity(curve):
    rnd = random.Random("elgamal identity " + curve)
    r, l = G.MODULI[curve], E.PARAMS[curve]["l"]
    for L in (1, 3, 4):
        dk, rand = rnd.randrange(1, l), rnd.randrange(l)
        msg = [rnd.randrange(r) for _ in range(L)]
        ek = G.keygen(curve, dk)
        Ep, ct = G.encrypt(curve, ek, msg, rand)
        assert Ep == E.mul(curve, rand, E.PARAMS[curve]["G"]) and len(ct) == L and ct != msg
        assert G.decrypt(curve, dk, (Ep, ct)) == (msg, True)
        assert G.decrypt(curve, (dk + 1) % l, (Ep, ct))[0] != msg
    # an E of small order is decrypted and flagged; an E off the curve counts as the identity
    small = E.small_order_points(curve)[8]
    back, ok = G.decrypt(curve, dk, (small, ct))
    assert ok is False and len(back) == L
    off = (Ep[0], (Ep[1] + 1) % r)
    assert not E.on_curve(curve, off)
    assert G.decrypt(curve, dk, (off, ct)) == (G.stream(curve, R.permute(curve, [0, 1, 0, 0])[0], ct, True), False)


@pytest.mark.parametrize("curve", CURVES)
def test_sponge_separates_lengths_and_differs_from_hash3(curve):
    rnd = random.Random("sponge " + curve)
    r = G.MODULI[curve]
    a, b, c = (rnd.randrange(1, r) for _ in range(3))
    outs = [G.sponge(curve, xs, 3) for xs in ([a], [a, 0], [a, 0, 0], [a, 0, 0, 0])]
    assert len({tuple(o) for o in outs}) == 4 and len({o[0] for o in outs}) == 4
    assert G.sponge(curve, [a, b, c], 1) == [R.permute(curve, [a, b, c, 3])[0]]
    assert G.sponge(curve, [a, b, c], 1)[0] != R.permute(curve, [a, b, c, 0])[0]           # hash3 is another domain
    assert G.sponge(curve, [a, b, c, a], 2) == R.permute(curve, [(x + y) % r for x, y in zip(R.permute(curve, [a, b, c, 4]), [a, 0, 0, 0])])[:2]
    assert G.sponge(curve, [a, b], 3)[:1] == G.sponge(curve, [a, b], 1)


@pytest.mark.parametrize("curve", CURVES)
def test_stream_blocks_differ_by_their_counter(curve):
    r = G.MODULI[curve]
    k = random.Random("stream " + curve).randrange(r)
    blocks = [tuple(G.stream_block(curve, k, j)) for j in range(4)]
    assert len(set(blocks)) == 4 and len({x for blk in blocks for x in blk}) == 12
    assert blocks[1] == tuple(R.permute(curve, [k, 1, 0, r - 1])[:3])
    assert G.keystream(curve, k, 7) == list(blocks[0] + blocks[1] + blocks[2][:1])
    text = [5, 0, r - 1, 7]
    assert G.stream(curve, k, G.stream(curve, k, text), decrypt=True) == text
    assert tuple(G.stream_block(curve, (k + 1) % r, 0)) != blocks[0]


# ---------------------------------------------------------------------------------------------- the gadget circuits
def case_sponge(curve, m, L, n_out):
    r = G.MODULI[curve]
    rnd = random.Random(f"sponge case {curve} {L}")
    rows = ([[0] * L, [r - 1] * L] + [[rnd.randrange(r) for _ in range(L)] for _ in range(m)])[:m]
    b = BD.CircuitBuilder(curve)
    xs = [b.input(m) for _ in range(L)]
    b.constant(L)                                       # so that the count below is the gadget's alone
    g = b.num_gates
    outs = b.rescue_sponge(xs, n_out)
    counts = {"sponge": b.num_gates - g}
    want = [G.sponge(curve, row, n_out) for row in rows]
    return b.build(), columns(rows), [], dict(outs=[np.atleast_1d(o) for o in outs], want=want, counts=counts, m=m, L=L, n_out=n_out)


def case_stream(curve, m, nblocks=3):
    r = G.MODULI[curve]
    rnd = random.Random(f"stream case {curve}")
    keys = ([0, r - 1] + [rnd.randrange(r) for _ in range(m)])[:m]
    b = BD.CircuitBuilder(curve)
    key = b.input(m)
    for c in list(range(nblocks)) + [-1]:
        b.constant(c)
    g = b.num_gates
    blocks = b.rescue_stream(key, nblocks)
    counts = {"stream": b.num_gates - g}
    want = [[x for j in range(nblocks) for x in G.stream_block(curve, k, j)] for k in keys]
    return b.build(), keys, [], dict(outs=[np.atleast_1d(v) for blk in blocks for v in blk], want=want, counts=counts, m=m, nblocks=nblocks)


_made = {}


def ciphertexts(curve, count, L=4):
    """`count` (ek, r, msg, (E, ct), dk) of the reference, computed once"""
    have = _made.setdefault((curve, L), [])
    rnd = random.Random(f"elgamal {curve} {L} {len(have)}")
    r, l = G.MODULI[curve], E.PARAMS[curve]["l"]
    while len(have) < count:
        dk, rand = rnd.randrange(1, l), rnd.randrange(l)
        msg = [rnd.randrange(r) for _ in range(L)]
        if not have:
            msg[0], msg[-1] = 0, r - 1
        ek = G.keygen(curve, dk)
        have.append((ek, rand, msg, G.encrypt(curve, ek, msg, rand), dk))
    return have[:count]


def elgamal_values(cts):
    """-> (inputs, public inputs) as plain residues in elgamal_circuit's order"""
    return (columns([(rand, *msg) for _, rand, msg, _, _ in cts]),
            columns([(ek[0], ek[1], Ep[0], Ep[1], *ct) for ek, _, _, (Ep, ct), _ in cts]))


def case_elgamal(curve, m, L=4):
    """inputs ek.x, ek.y, r, msg_0 .. msg_{L-1} per instance; outputs E.x, E.y, ct_0 .. ct_{L-1}"""
    cts = ciphertexts(curve, m, L)
    b = BD.CircuitBuilder(curve)
    ekx, eky, rand = b.input(m), b.input(m), b.input(m)
    msg = [b.input(m) for _ in range(L)]
    for c in list(range((L + 2) // 3)) + [-1]:
        b.constant(c)
    g = b.num_gates
    Ep, ct = b.elgamal_encrypt((ekx, eky), msg, rand)
    counts = {"elgamal_encrypt": b.num_gates - g}
    values = columns([(ek[0], ek[1], rr, *mm) for ek, rr, mm, _, _ in cts])
    want = [[Ew[0], Ew[1], *ctw] for _, _, _, (Ew, ctw), _ in cts]
    return b.build(), values, [], dict(outs=[np.atleast_1d(v) for v in (Ep[0], Ep[1], *ct)], want=want, counts=counts, m=m, L=L)


GADGET_CASES = {f"sponge_L{L}_n{n}": (lambda curve, m, L=L, n=n: case_sponge(curve, m, L, n)) for L, n in SPONGE_SHAPES}
GADGET_CASES.update({"stream3": case_stream, "elgamal_L4": case_elgamal})


def solved(built, values, pub):
    ref = HintRefSolver(built, values, pub)
    wit, lvl = ref.solve()
    return ref, wit, lvl


def check_case(info, wit):
    for i in range(info["m"]):
        assert [wit[int(o[i])] for o in info["outs"]] == info["want"][i], i


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("L,n_out", SPONGE_SHAPES)
def test_sponge_gadget(curve, L, n_out):
    m = 3
    built, values, pub, info = GADGET_CASES[f"sponge_L{L}_n{n_out}"](curve, m)
    assert info["counts"]["sponge"] == sponge_gates(L) * m and len(info["outs"]) == n_out
    ref, wit, lvl = solved(built, values, pub)
    assert ref.unsatisfied_gates(wit) == []
    check_case(info, wit)
    assert lvl[int(info["outs"][0][0])] == sponge_levels(L) and ref.depth() == sponge_levels(L) + 1       # the constant L sits at level 0, below the gadget


@pytest.mark.parametrize("curve", CURVES)
def test_stream_gadget(curve):
    m = 3
    built, values, pub, info = GADGET_CASES["stream3"](curve, m)
    assert info["counts"]["stream"] == PERMUTATION_GATES * 3 * m and len(info["outs"]) == 9
    ref, wit, lvl = solved(built, values, pub)
    assert ref.unsatisfied_gates(wit) == []
    check_case(info, wit)
    assert {lvl[int(o[0])] for o in info["outs"]} == {PERMUTATION_LEVELS}         # every block at the same depth, above the constants' level 0


@pytest.mark.parametrize("curve", CURVES)
def test_elgamal_encrypt_gadget(curve):
    m = 3
    built, values, pub, info = GADGET_CASES["elgamal_L4"](curve, m)
    assert info["counts"]["elgamal_encrypt"] == ELGAMAL_GATES[curve] * m
    lbits = E.PARAMS[curve]["l"].bit_length()
    # to_bits, fixed_base_mul, scalar_mul, hash3, two stream blocks, four additions
    assert ELGAMAL_GATES[curve] == (lbits + (lbits - 4 + 2) // 3 + 1) + (7 * lbits - 5) + (19 * lbits - 17) + 148 + 2 * 148 + 4
    ref, wit, lvl = solved(built, values, pub)
    assert ref.unsatisfied_gates(wit) == []
    check_case(info, wit)
    assert lvl[int(info["outs"][-1][0])] == ELGAMAL_LEVELS[curve] - 1 and ELGAMAL_LEVELS[curve] == 4 * lbits + 2 * PERMUTATION_LEVELS + 1
    assert ref.depth() == ELGAMAL_LEVELS[curve]
    # r given as bits: the same ciphertext with enforce_bool instead of to_bits
    ek, rand, msg, (Ew, ctw), _ = ciphertexts(curve, 1)[0]
    b = BD.CircuitBuilder(curve)
    ekv, mv = (b.input(), b.input()), [b.input() for _ in range(4)]
    bits = [b.input() for _ in range(lbits)]
    Ep, ct = b.elgamal_encrypt(ekv, mv, bits)
    ref, wit, _ = solved(b.build(), [ek[0], ek[1], *msg] + [(rand >> k) & 1 for k in range(lbits)], [])
    assert ref.unsatisfied_gates(wit) == []
    assert [wit[int(v)] for v in (Ep[0], Ep[1], *ct)] == [Ew[0], Ew[1], *ctw]


@pytest.mark.parametrize("curve", CURVES)
def test_encryption_circuit_accepts_and_refuses(curve):
    L = 4
    built = EG.elgamal_circuit(curve, 1, L)
    assert built.n == 1 << 13 and built.num_public == 4 + L and len(built.input_vars) == 1 + L
    assert built.num_gates_unpadded == ELGAMAL_GATES[curve] + 2 + (4 + L) + 1 + (2 + L)       # zero, one; IO gates; the stream's constant -1; enforce_equal
    (ek, rand, msg, (Ep, ct), dk), = ciphertexts(curve, 1)
    values, pub = elgamal_values([(ek, rand, msg, (Ep, ct), dk)])
    ref, wit, _ = solved(built, values, pub)
    assert ref.unsatisfied_gates(wit) == []
    r, l, Gp = G.MODULI[curve], E.PARAMS[curve]["l"], E.PARAMS[curve]["G"]
    other_r = (rand + 1) % l
    other_ek, other_E = E.mul(curve, 3, ek), E.mul(curve, 5, Gp)
    assert other_E != Ep and E.on_curve(curve, other_E)
    bad_ct = list(ct)
    bad_ct[2] = (ct[2] + 1) % r
    cases = {"a ciphertext element + 1": (values, [ek[0], ek[1], Ep[0], Ep[1], *bad_ct]),
             "another r": ([other_r, *msg], pub),
             "another ek": (values, [other_ek[0], other_ek[1], Ep[0], Ep[1], *ct]),
             "E replaced by another curve point": (values, [ek[0], ek[1], other_E[0], other_E[1], *ct]),
             "another message": ([rand, msg[0], (msg[1] + 1) % r, *msg[2:]], pub)}
    for name, (vals, pubs) in cases.items():
        ref, wit, _ = solved(built, vals, pubs)
        assert ref.unsatisfied_gates(wit) != [], name
    # an r of bit_length(l) bits that is >= l is accepted by the circuit (the docstring says so) and names the same E
    if rand + l < 1 << l.bit_length():
        Ew, ctw = Ep, G.stream(curve, G.dh_key(curve, rand + l, ek), msg)
        ref, wit, _ = solved(built, [rand + l, *msg], [ek[0], ek[1], Ew[0], Ew[1], *ctw])
        assert ref.unsatisfied_gates(wit) == [] and ctw == ct


@pytest.mark.parametrize("m,L,log_n", [(2, 4, 14), (1, 1, 13), (1, 4, 13)])
def test_witness_inputs_layout_and_circuit_sizes(m, L, log_n):
    curve = "bn254"
    f = _fr.FIELDS[curve]
    cts = ciphertexts(curve, m, L)
    values, pub = elgamal_values(cts)
    pts = lambda ps: np.stack([np.stack([f.to_limbs(P[0]), f.to_limbs(P[1])]) for P in ps])
    texts = lambda ts: np.stack([f.vec_to_limbs(list(t)) for t in ts])
    inputs, public = EG.elgamal_witness_inputs(pts([c[0] for c in cts]), f.vec_to_limbs([c[1] for c in cts]), texts([c[2] for c in cts]),
                                               (pts([c[3][0] for c in cts]), texts([c[3][1] for c in cts])))
    assert inputs.shape == ((1 + L) * m, 4) and public.shape == ((4 + L) * m, 4)
    assert [f.from_limbs(x) for x in inputs] == values and [f.from_limbs(x) for x in public] == pub
    built = EG.elgamal_circuit(curve, m, L)
    assert len(built.input_vars) == (1 + L) * m and built.num_public == (4 + L) * m and built.n == 1 << log_n
    ref, wit, _ = solved(built, values, pub)                # the order of the values IS the order in which the circuit creates its inputs
    assert ref.unsatisfied_gates(wit) == []
    with pytest.raises(ValueError):
        EG.elgamal_witness_inputs(pts([c[0] for c in cts]), f.vec_to_limbs([c[1] for c in cts]), texts([c[2] for c in cts]),
                                  (pts([c[3][0] for c in cts]), texts([c[3][1][:-1] + [0, 0] for c in cts])))


def test_sixteen_encryptions_fill_two_to_the_seventeen():
    built = EG.elgamal_circuit("bn254", 16, 4)
    assert built.n == 1 << 17 and built.num_gates_unpadded == 16 * (ELGAMAL_GATES["bn254"] + 4 + 4 + 2 + 4) + 2 + 1


# ---------------------------------------------------------------------------------------------- arguments
class _NoDevice:
    """stands where a worker would: the checks below are refused before anything reaches the device"""

    def __init__(self, curve):
        self.curve_name = curve


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors(curve):
    b = BD.CircuitBuilder(curve)
    x, y, rr = b.input(), b.input(), b.input()
    two, three = b.input(2), b.input(3)
    other_ed, other_rs = ED.EdwardsParams.default(OTHER[curve]), RS.RescueParams.default(OTHER[curve])
    g = b.num_gates
    for call in (lambda: b.rescue_sponge([]), lambda: b.rescue_sponge([x], n_out=0), lambda: b.rescue_sponge([x], n_out=4), lambda: b.rescue_sponge([two, three]),
                 lambda: b.rescue_sponge([x], params=other_rs), lambda: b.rescue_sponge([x, b.num_vars]),
                 lambda: b.rescue_stream(x, 0), lambda: b.rescue_stream(x, 1.5), lambda: b.rescue_stream(x, 1, params=other_rs), lambda: b.rescue_stream(-1, 1),
                 lambda: b.elgamal_encrypt((x, y), [], rr), lambda: b.elgamal_encrypt((x, y), [two, three], rr), lambda: b.elgamal_encrypt((x, y), [x], [rr] * 5),
                 lambda: b.elgamal_encrypt((x, y), [x], rr, prm=other_ed), lambda: b.elgamal_encrypt((x, y), [x], rr, rescue=other_rs),
                 lambda: b.elgamal_encrypt(x, [x], rr), lambda: b.elgamal_encrypt((two, y), [three], rr)):
        with pytest.raises(ValueError):
            call()
    assert b.num_gates == g                              # a refused call emits nothing
    for call in (lambda: EG.elgamal_circuit(curve, 0, 4), lambda: EG.elgamal_circuit(curve, 1, 0), lambda: EG.elgamal_circuit(curve, 1, 1, params=other_ed),
                 lambda: EG.elgamal_circuit(curve, 1, 1, rescue=other_rs)):
        with pytest.raises(ValueError):
            call()
    # the module's own checks come before any device call: an r >= l, mismatched counts, L = 0, parameters of the other curve
    w, prm, f = _NoDevice(curve), ED.EdwardsParams.default(curve), _fr.FIELDS[curve]
    ek = np.zeros((2, 2, 4), dtype=np.uint64)
    msg = np.zeros((2, 3, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="r\\[1\\] >= l"):
        EG.encrypt(w, prm, ek, msg, f.vec_to_limbs([prm.order - 1, prm.order]))
    with pytest.raises(ValueError, match="mismatched"):
        EG.encrypt(w, prm, ek, msg, f.vec_to_limbs([1, 2, 3]))
    with pytest.raises(ValueError):
        EG.encrypt(w, prm, ek, np.zeros((2, 0, 4), dtype=np.uint64), f.vec_to_limbs([1, 2]))
    with pytest.raises(ValueError):
        EG.encrypt(w, other_ed, ek, msg, f.vec_to_limbs([1, 2]))
    with pytest.raises(ValueError):
        EG.encrypt(w, prm, ek, msg, f.vec_to_limbs([1, 2]), rescue=other_rs)
    with pytest.raises(ValueError, match="mismatched"):
        EG.decrypt(w, prm, f.vec_to_limbs([1]), (ek, msg))
    with pytest.raises(ValueError):
        RS.sponge(w, RS.RescueParams.default(curve), np.zeros((2, 0, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        RS.sponge(w, RS.RescueParams.default(curve), msg, n_out=4)
    with pytest.raises(ValueError):
        RS.sponge(w, other_rs, msg)
    with pytest.raises(ValueError, match="mismatched"):
        RS.stream(w, RS.RescueParams.default(curve), f.vec_to_limbs([1, 2, 3]), msg)
    with pytest.raises(ValueError):
        RS.sponge_dev(w, RS.RescueParams.default(curve), 1, 0, 1, 1, 1)
    with pytest.raises(ValueError):
        RS.stream_dev(w, RS.RescueParams.default(curve), 1, 1, 1 << 32, 1, 1)
