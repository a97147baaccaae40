"""The embedded Edwards curves on the host: the default parameters (G on the curve, l prime, l G = (0, 1), a a square, d a non-square —
the conditions of the complete addition law), circomlib's published Baby Jubjub answers against the pure-Python reference
(tests/edwards_ref.py), and every builder gadget — point_add on the exceptional-looking pairs, point_double, point_select, point_neg,
enforce_on_curve, to_bits_strict, scalar_mul, fixed_base_mul, schnorr_verify — built, solved by the sequential big-integer solver
(tests/hint_ref.py) and compared with the reference, with the gate and level counts the docstrings state.  No GPU.

The gadget circuits live in GADGET_CASES so that tests/test_gpu_edwards_circuit.py solves the same ones on the device."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import fr as _fr
from tests import edwards_ref as E
from tests.hint_ref import HintRefSolver

CURVES = list(E.CURVES)
OTHER = {"bn254": "bls12_381", "bls12_381": "bn254"}
SCHNORR_GATES = {"bn254": 7798, "bls12_381": 7827}
STRICT_GATES = {"bn254": 592, "bls12_381": 594}


def is_prime(n: int) -> bool:
    """Miller-Rabin with 40 seeded bases (error below 4^-40 for a composite)"""
    if n < 2 or n % 2 == 0:
        return n == 2
    q, s = n - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    rnd = random.Random(n)
    for _ in range(40):
        x = pow(rnd.randrange(2, n - 1), q, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ---------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("curve", CURVES)
def test_default_parameters(curve):
    prm, c, r = ED.EdwardsParams.default(curve), E.PARAMS[curve], E.MODULI[curve]
    assert _fr.FIELDS[curve].p == r
    assert (prm.a, prm.d, prm.generator, prm.order, prm.cofactor) == (c["a"], c["d"], c["G"], c["l"], 8)
    assert E.on_curve(curve, c["G"]) and c["G"] != E.IDENTITY
    assert is_prime(c["l"]) and c["l"] < r and c["l"].bit_length() == {"bn254": 251, "bls12_381": 252}[curve]
    assert E.mul(curve, c["l"], c["G"]) == E.IDENTITY
    assert pow(c["a"], (r - 1) // 2, r) == 1 and pow(c["d"], (r - 1) // 2, r) == r - 1
    # the package's own integer arithmetic (the constants of fixed_base_mul) is the reference's
    assert prm.mul_int(12345, c["G"]) == E.mul(curve, 12345, c["G"]) and prm.add_int(c["G"], c["G"]) == E.add(curve, c["G"], c["G"])
    limbs = prm.limbs()
    f = _fr.FIELDS[curve]
    assert limbs.shape == (20,) and limbs.dtype == np.uint64
    assert [f.from_limbs(limbs[4 * i:4 * i + 4]) for i in range(4)] == [c["a"], c["d"], c["G"][0], c["G"][1]]
    assert int.from_bytes(limbs[16:].tobytes(), "little") == c["l"]
    if curve == "bls12_381":                           # G = 8 x the point with y = 3 and the smaller x
        assert E.mul(curve, 8, E.point_with_y(curve, 3)) == c["G"]


@pytest.mark.parametrize("curve", CURVES)
def test_constructor_refuses_an_incomplete_law(curve):
    c, r = E.PARAMS[curve], E.MODULI[curve]
    G2 = E.mul(curve, 7, c["G"])
    again = ED.EdwardsParams(curve, c["a"], c["d"], G2, c["l"], 8)
    assert again.generator == G2 and not np.array_equal(again.limbs(), ED.EdwardsParams.default(curve).limbs())
    nonsquare = next(x for x in range(2, 50) if pow(x, (r - 1) // 2, r) == r - 1)
    with pytest.raises(ValueError, match="a is not"):
        ED.EdwardsParams(curve, nonsquare, c["d"], c["G"], c["l"], 8)
    with pytest.raises(ValueError, match="a is not"):
        ED.EdwardsParams(curve, 0, c["d"], c["G"], c["l"], 8)
    with pytest.raises(ValueError, match="d is not"):
        ED.EdwardsParams(curve, c["a"], 4, c["G"], c["l"], 8)
    with pytest.raises(ValueError, match="not on the curve"):
        ED.EdwardsParams(curve, c["a"], c["d"], (c["G"][0], c["G"][1] + 1), c["l"], 8)
    with pytest.raises(ValueError):
        ED.EdwardsParams("secp256k1", 1, 2, (0, 1), 7, 1)


def test_baby_jubjub_known_answers():
    """circomlib's test vectors"""
    P = (17777552123799933955779906779655732241715742912184938656739573121738514868268,
         2626589144620713026669568689430873010625803728049924121243784502389097019475)
    assert E.on_curve("bn254", P)
    assert E.add("bn254", P, P) == (6890855772600357754907169075114257697580319025794532037257385534741338397365,
                                    4338620300185947561074059802482547481416142213883829469920100239455078257889)
    base = (995203441582195749578291179787384436505546430278305826713579947235728471134,
            5472060717959818805561601436314318772137091100104008585924551046643952123905)
    assert E.mul("bn254", 8, base) == E.PARAMS["bn254"]["G"]


@pytest.mark.parametrize("curve", CURVES)
def test_reference_group_structure(curve):
    c, r = E.PARAMS[curve], E.MODULI[curve]
    small = E.small_order_points(curve)
    for order, T in small.items():
        assert E.on_curve(curve, T) and E.mul(curve, order, T) == E.IDENTITY and E.mul(curve, order // 2, T) != E.IDENTITY
        assert not E.in_subgroup(curve, T)
    rnd = random.Random(5)
    P, Q = E.random_point(curve, rnd), E.random_point(curve, rnd)
    assert E.add(curve, P, E.neg(curve, P)) == E.IDENTITY and E.add(curve, P, E.IDENTITY) == P
    assert E.add(curve, E.add(curve, P, Q), c["G"]) == E.add(curve, P, E.add(curve, Q, c["G"]))
    assert E.mul(curve, 8 * c["l"], P) == E.IDENTITY and E.in_subgroup(curve, E.mul(curve, 8, P))
    assert E.mul(curve, r - 1, c["G"]) == E.mul(curve, (r - 1) % c["l"], c["G"])


# ---------------------------------------------------------------------------------------------- the gadget circuits
def point_pairs(curve):
    """(P, Q) pairs for point_add: generic, P + P, P + (-P), P + identity, identity + identity, and the points of order 2, 4 and 8"""
    rnd = random.Random("pairs " + curve)
    G = E.PARAMS[curve]["G"]
    small = E.small_order_points(curve)
    P, Q = E.random_point(curve, rnd), E.mul(curve, rnd.randrange(1 << 64), G)
    return [(P, Q), (P, P), (P, E.neg(curve, P)), (P, E.IDENTITY), (E.IDENTITY, E.IDENTITY), (small[2], small[2]), (small[4], P), (small[8], small[8]),
            (small[8], small[4]), (G, E.neg(curve, G))]


def columns(rows):
    """per-instance tuples -> the values in input order: the first component of every instance, then the second, ..."""
    return [row[k] for k in range(len(rows[0])) for row in rows]


def case_point_ops(curve, m):
    """inputs P, Q, bit per instance; outputs P + Q, 2 P, bit ? P : Q, -P; enforce_on_curve on both"""
    pairs = point_pairs(curve)[:m] if m <= 3 else point_pairs(curve)
    m = len(pairs)
    b = BD.CircuitBuilder(curve)
    px, py, qx, qy, bit = (b.input(m) for _ in range(5))
    counts = {}
    g = b.num_gates
    s = b.point_add((px, py), (qx, qy)); counts["add"] = b.num_gates - g; g = b.num_gates
    d = b.point_double((px, py)); counts["double"] = b.num_gates - g; g = b.num_gates
    sel = b.point_select(bit, (px, py), (qx, qy)); counts["select"] = b.num_gates - g; g = b.num_gates
    n = b.point_neg((px, py)); counts["neg"] = b.num_gates - g; g = b.num_gates
    b.enforce_on_curve((px, py)); counts["on_curve"] = b.num_gates - g; g = b.num_gates
    b.enforce_point_equal(b.point_add((px, py), n), b.point_constant(0, 1))
    bits = [i % 2 for i in range(m)]
    values = columns([(P[0], P[1], Q[0], Q[1], bt) for (P, Q), bt in zip(pairs, bits)])
    want = [(E.add(curve, P, Q), E.add(curve, P, P), P if bt else Q, E.neg(curve, P)) for (P, Q), bt in zip(pairs, bits)]
    return b.build(), values, [], dict(outs=(s, d, sel, n), want=want, counts=counts, m=m)


def case_scalar_mul(curve, m, nbits):
    """inputs k, P per instance; outputs [k] P (bits from to_bits, or to_bits_strict at full width) and [k] G"""
    r, G = E.MODULI[curve], E.PARAMS[curve]["G"]
    rnd = random.Random(f"scalar {curve} {nbits}")
    full = nbits == r.bit_length()
    top = r if full else 1 << nbits
    ks = ([top - 1, 0, 1] + [rnd.randrange(top) for _ in range(m)])[:m]
    small = E.small_order_points(curve)
    Ps = ([E.random_point(curve, rnd), small[8], G] + [E.random_point(curve, rnd) for _ in range(m)])[:m]
    b = BD.CircuitBuilder(curve)
    k, px, py = (b.input(m) for _ in range(3))
    g = b.num_gates
    bits = b.to_bits_strict(k) if full else b.to_bits(k, nbits)
    counts = {"bits": b.num_gates - g}; g = b.num_gates
    var = b.scalar_mul(bits, (px, py)); counts["scalar_mul"] = b.num_gates - g; g = b.num_gates
    fix = b.fixed_base_mul(bits); counts["fixed_base_mul"] = b.num_gates - g
    values = columns([(kk, P[0], P[1]) for kk, P in zip(ks, Ps)])
    want = [(E.mul(curve, kk, P), E.mul(curve, kk, G)) for kk, P in zip(ks, Ps)]
    return b.build(), values, [], dict(outs=(var, fix), want=want, counts=counts, m=m, nbits=nbits)


_signed = {}


def signatures(curve, count):
    """`count` (pk, message, (R, s)) of the reference, computed once"""
    have = _signed.setdefault(curve, [])
    rnd = random.Random(f"schnorr {curve} {len(have)}")
    c = E.PARAMS[curve]
    while len(have) < count:
        sk, nonce, msg = rnd.randrange(1, E.MODULI[curve]), rnd.randrange(1, E.MODULI[curve]), rnd.randrange(E.MODULI[curve])
        have.append((E.mul(curve, sk, c["G"]), msg, E.schnorr_sign(curve, sk, nonce, msg)))
    return have[:count]


def schnorr_values(sigs):
    """-> (inputs, public inputs) as plain residues in schnorr_circuit's order"""
    return columns([(R[0], R[1], s) for _, _, (R, s) in sigs]), columns([(pk[0], pk[1], msg) for pk, msg, _ in sigs])


def case_schnorr(curve, m):
    sigs = signatures(curve, m)
    values, pub = schnorr_values(sigs)
    return ED.schnorr_circuit(curve, m), values, pub, dict(m=m, sigs=sigs)


GADGET_CASES = {"point_ops": case_point_ops, "scalar_mul8": lambda curve, m: case_scalar_mul(curve, m, 8),
                "scalar_mul_full": lambda curve, m: case_scalar_mul(curve, m, E.MODULI[curve].bit_length()), "schnorr": case_schnorr}


def out_values(wit, outs, i):
    return tuple((wit[int(np.atleast_1d(x)[i])], wit[int(np.atleast_1d(y)[i])]) for x, y in outs)


@pytest.mark.parametrize("curve", CURVES)
def test_point_gadgets_on_every_kind_of_pair(curve):
    built, values, pub, info = case_point_ops(curve, 99)
    assert info["counts"] == {"add": 9 * info["m"], "double": 8 * info["m"], "select": 2 * info["m"], "neg": info["m"], "on_curve": 3 * info["m"]}
    ref = HintRefSolver(built, values, pub)
    wit, lvl = ref.solve()
    assert ref.unsatisfied_gates(wit) == []
    for i in range(info["m"]):
        assert out_values(wit, info["outs"], i) == info["want"][i], i
    s, d = info["outs"][0], info["outs"][1]
    assert lvl[int(s[0][0])] == 3 and lvl[int(d[0][0])] == 2            # 4 and 3 levels, counted from 0
    # a point off the curve fails enforce_on_curve
    wrong = list(values)
    wrong[info["m"]] = (wrong[info["m"]] + 1) % E.MODULI[curve]          # P.y of the first instance
    ref = HintRefSolver(built, wrong, pub)
    assert ref.unsatisfied_gates(ref.solve()[0]) != []


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("width", ["8", "full"])
def test_scalar_mul_gadgets(curve, width):
    m = 3
    built, values, pub, info = GADGET_CASES[f"scalar_mul{'8' if width == '8' else '_full'}"](curve, m)
    nbits = info["nbits"]
    assert info["counts"]["scalar_mul"] == (19 * nbits - 17) * m and info["counts"]["fixed_base_mul"] == (7 * nbits - 5) * m
    if width == "full":
        assert info["counts"]["bits"] == STRICT_GATES[curve] * m
    ref = HintRefSolver(built, values, pub)
    wit, lvl = ref.solve()
    assert ref.unsatisfied_gates(wit) == []
    for i in range(m):
        assert out_values(wit, info["outs"], i) == info["want"][i], i
    var, fix = info["outs"]
    # depth, counted from 0 with the bits at level 0: the docstrings' 4 nbits levels (the second addend waits for one doubling: level 3, then
    # 4 levels per addition) and 1 + 3 (nbits - 1) + 1 (two lc gates at level 1, then 3 levels per constant addition)
    assert lvl[int(var[0][0])] == 4 * nbits - 1 and lvl[int(fix[0][0])] == 1 + 3 * (nbits - 1)


@pytest.mark.parametrize("curve", CURVES)
def test_to_bits_strict(curve):
    r = E.MODULI[curve]
    L = r.bit_length()
    xs = [0, 1, r - 1, 1 << (L - 1), random.Random(9).randrange(r)]
    b = BD.CircuitBuilder(curve)
    x = b.input(len(xs))
    g = b.num_gates
    bits = b.to_bits_strict(x)
    assert b.num_gates - g == STRICT_GATES[curve] * len(xs) and len(bits) == L
    built = b.build()
    ref = HintRefSolver(built, xs)
    wit, _ = ref.solve()
    assert ref.unsatisfied_gates(wit) == []
    for i, v in enumerate(xs):
        assert sum(wit[int(bits[k][i])] << k for k in range(L)) == v
    # the other decomposition of 0 and of 1 — the bits of r and of r + 1 — recomposes mod r and is refused by the comparison alone
    for i, pattern in ((0, r), (1, r + 1)):
        assert pattern.bit_length() == L
        ref = HintRefSolver(built, xs)
        for k in range(L):
            ref.val[int(bits[k][i])], ref.lvl[int(bits[k][i])] = (pattern >> k) & 1, 0
        bad = ref.unsatisfied_gates(ref.solve()[0])
        assert bad, pattern
        for gate in bad:                                # none of them is a bit gate or a recomposition gate: only run * bit = 0 fails
            q = ref.selectors(gate)
            assert q[4] == 1 and q[10] == 0 and not any(q[:4]), (gate, q)
    with pytest.raises(ValueError):
        b.to_bits(x, L)                                 # to_bits itself still stops one bit short


@pytest.mark.parametrize("curve", CURVES)
def test_schnorr_gadget_accepts_and_refuses(curve):
    m = 1
    b = BD.CircuitBuilder(curve)
    pk, msg, Rp, s = (b.input(), b.input()), b.input(), (b.input(), b.input()), b.input()
    g = b.num_gates
    b.schnorr_verify(pk, msg, Rp, s)
    assert b.num_gates - g == SCHNORR_GATES[curve]
    built, values, pub, info = case_schnorr(curve, m)
    assert built.num_gates_unpadded == SCHNORR_GATES[curve] + 2 + 3 and built.n == 1 << 13 and built.num_public == 3
    (pk_v, msg_v, (R_v, s_v)), = info["sigs"]
    assert E.schnorr_verify(curve, pk_v, msg_v, (R_v, s_v))
    ref = HintRefSolver(built, values, pub)
    wit, _ = ref.solve()
    assert ref.unsatisfied_gates(wit) == []
    r, l = E.MODULI[curve], E.PARAMS[curve]["l"]
    other_pk = E.mul(curve, 3, pk_v)
    off = (R_v[0], (R_v[1] + 1) % r)
    for name, (vals, pubs) in {"s + 1": ([R_v[0], R_v[1], (s_v + 1) % l], pub), "another message": (values, [pk_v[0], pk_v[1], (msg_v + 1) % r]),
                               "another pk": (values, [other_pk[0], other_pk[1], msg_v]), "R off the curve": ([off[0], off[1], s_v], pub)}.items():
        ref = HintRefSolver(built, vals, pubs)
        assert ref.unsatisfied_gates(ref.solve()[0]) != [], name
    # s given as bits: the same equation with enforce_bool instead of to_bits
    lb = l.bit_length()
    b = BD.CircuitBuilder(curve)
    pk, msg, Rp = (b.input(), b.input()), b.input(), (b.input(), b.input())
    s_bits = [b.input() for _ in range(lb)]
    b.schnorr_verify(pk, msg, Rp, s_bits)
    ref = HintRefSolver(b.build(), [pk_v[0], pk_v[1], msg_v, R_v[0], R_v[1]] + [(s_v >> k) & 1 for k in range(lb)])
    assert ref.unsatisfied_gates(ref.solve()[0]) == []


def test_schnorr_witness_inputs_layout():
    curve, m = "bn254", 2
    f = _fr.FIELDS[curve]
    sigs = signatures(curve, m)
    values, pub = schnorr_values(sigs)
    pks = np.stack([np.stack([f.to_limbs(pk[0]), f.to_limbs(pk[1])]) for pk, _, _ in sigs])
    Rs = np.stack([np.stack([f.to_limbs(R[0]), f.to_limbs(R[1])]) for _, _, (R, _) in sigs])
    inputs, public = ED.schnorr_witness_inputs(pks, f.vec_to_limbs([msg for _, msg, _ in sigs]), (Rs, f.vec_to_limbs([s for _, _, (_, s) in sigs])))
    assert [f.from_limbs(x) for x in inputs] == values and [f.from_limbs(x) for x in public] == pub
    built = ED.schnorr_circuit(curve, m)
    assert len(built.input_vars) == 3 * m and built.num_public == 3 * m and built.n == 1 << 14
    with pytest.raises(ValueError):
        ED.schnorr_circuit(curve, 0)


# ---------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors(curve):
    b = BD.CircuitBuilder(curve)
    x, y, bit = b.input(), b.input(), b.input()
    two, three = b.input(2), b.input(3)
    other = ED.EdwardsParams.default(OTHER[curve])
    g = b.num_gates
    for call in (lambda: b.point_add(x, (x, y)), lambda: b.point_add((x, y, x), (x, y)), lambda: b.point_add((two, y), (three, y)),
                 lambda: b.point_add((x, y), (x, y), prm=other), lambda: b.point_double((x, y), prm=other), lambda: b.point_double([x]),
                 lambda: b.point_select(two, (three, y), (x, y)), lambda: b.point_neg(x), lambda: b.enforce_on_curve((x, 10 ** 9)),
                 lambda: b.enforce_on_curve((x, y), prm="bn254"), lambda: b.enforce_point_equal((two, y), (three, y)),
                 lambda: b.scalar_mul([], (x, y)), lambda: b.scalar_mul([two, three], (x, y)), lambda: b.scalar_mul([bit], (x, y), prm=other),
                 lambda: b.fixed_base_mul([]), lambda: b.fixed_base_mul([two, three]), lambda: b.fixed_base_mul([bit], prm=other),
                 lambda: b.point_constant(1, 1), lambda: b.schnorr_verify((x, y), x, (x, y), [bit] * 5),
                 lambda: b.schnorr_verify((x, y), x, (x, y), x, prm=other), lambda: b.schnorr_verify((x, y), x, (x, y), x, rescue=other),
                 lambda: b.schnorr_verify((x, y), two, (three, y), x)):
        with pytest.raises(ValueError):
            call()
    assert b.num_gates == g                              # a refused call emits nothing
    # the facts the builder pins about q_ecc and to_bits stay as they were
    with pytest.raises(ValueError, match="unknown selector"):
        b.gate([x, y, x, y], {"q_ecc": 1})
    assert "q_ecc" not in BD.SELECTOR_INDEX
