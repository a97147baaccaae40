"""The reference of the KZG tests: polynomials on Python integers mod r, and the scheme restated with the trapdoor of the synthetic SRS
(`plonk_synth_srs` with tests/circuit_cases.TAU): the commitment of f is [f(tau)] G, and the opening (C, pi, z, y) holds iff
pi = [(f(tau) - y) (tau - z)^-1] G.  Points come from the oracle's group arithmetic (`oracle.msm` on the single base G); nothing here calls
the library under test — residues go to and from Montgomery limbs by integer arithmetic."""
import numpy as np

from oracle import oracle as O
from tests.circuit_cases import TAU

CURVES = [("bn254", 0), ("bls12_381", 1)]
FR = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
      "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
FR_GENERATOR = {"bn254": 5, "bls12_381": 7}               # multiplicative generators (ark-ff's GENERATOR)
TWO_ADICITY = {"bn254": 28, "bls12_381": 32}
MASK = 2 ** 64 - 1


def to_limbs(curve, x):
    """The residue x as Montgomery limbs (x * 2^256 mod r)."""
    v = x % FR[curve] * pow(2, 256, FR[curve]) % FR[curve]
    return np.array([(v >> (64 * i)) & MASK for i in range(4)], dtype=np.uint64)


def plain_limbs(x):
    return np.array([(x >> (64 * i)) & MASK for i in range(4)], dtype=np.uint64)


def from_limbs(curve, l):
    return sum(int(v) << (64 * i) for i, v in enumerate(l)) * pow(2, -256, FR[curve]) % FR[curve]


def vec_to_limbs(curve, xs):
    return np.stack([to_limbs(curve, x) for x in xs]) if len(xs) else np.zeros((0, 4), np.uint64)


def root_of_unity(curve, n):
    """A primitive n-th root of unity, n a power of two."""
    p = FR[curve]
    assert n & (n - 1) == 0 and n <= 1 << TWO_ADICITY[curve]
    w = pow(FR_GENERATOR[curve], (p - 1) // n, p)
    assert pow(w, n, p) == 1 and (n == 1 or pow(w, n // 2, p) == p - 1)
    return w


def horner(curve, coeffs, z):
    p, acc = FR[curve], 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % p
    return acc


def synth_div(curve, coeffs, z):
    """(quotient of len - 1 coefficients, remainder): q_(len-2) = f_(len-1), q_(i-1) = f_i + z q_i, y = f_0 + z q_0."""
    p = FR[curve]
    if not coeffs:
        return [], 0
    q, acc = [0] * (len(coeffs) - 1), 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (coeffs[i] + z * acc) % p
        q[i - 1] = acc
    return q, (coeffs[0] + z * acc) % p


def g_times(curve, cid, s):
    """[s] G as (xy Montgomery limbs, is_infinity), by the oracle's MSM on the single base G."""
    xy, inf = O.jac_to_affine(cid, O.msm(cid, O.generator(cid).reshape(1, -1), plain_limbs(s % FR[curve]).reshape(1, 4)))
    return (np.zeros_like(xy), True) if inf else (xy, False)


def lincomb(curve, cid, terms):
    """sum s_k P_k for (scalar, (xy, inf)) pairs, by the oracle's MSM."""
    terms = [(s % FR[curve], pt) for s, pt in terms if not pt[1]]
    if not terms:
        return np.zeros(2 * O.FQ_LIMBS[cid], np.uint64), True
    xy, inf = O.jac_to_affine(cid, O.msm(cid, np.stack([pt[0] for _, pt in terms]), np.stack([plain_limbs(s) for s, _ in terms])))
    return (np.zeros_like(xy), True) if inf else (xy, False)


def commitment(curve, cid, coeffs, tau=TAU):
    return g_times(curve, cid, horner(curve, coeffs, tau))


def proof(curve, cid, coeffs, z, y=None, tau=TAU):
    """[(f(tau) - y) / (tau - z)] G; y defaults to f(z)."""
    p = FR[curve]
    y = horner(curve, coeffs, z) if y is None else y
    return g_times(curve, cid, (horner(curve, coeffs, tau) - y) * pow((tau - z) % p, -1, p))


def holds(curve, cid, comm, pi, z, y, tau=TAU):
    """The verifying equation with the trapdoor in G1: tau pi == C - y G + z pi, i.e. (tau - z) pi + y G == C."""
    lhs = lincomb(curve, cid, [((tau - z), pi), (y, (O.generator(cid), False))])
    return lhs[1] == comm[1] and (lhs[1] or np.array_equal(lhs[0], np.asarray(comm[0], dtype=np.uint64).reshape(-1)))


def xy_of(pt):
    """(xy, inf) -> x || y with zeros for infinity, the form of Opening.proof_xy."""
    return np.zeros_like(pt[0]) if pt[1] else np.asarray(pt[0], dtype=np.uint64).reshape(-1)
