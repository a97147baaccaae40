"""G2 and the pairing of the library's host entries (plonk_g2_*, plonk_pairing_check) on the CPU, both curves: group law and subgroup check
against repeated addition, bilinearity and non-degeneracy of the optimal ate pairing, rejection of perturbed products and of twist points
outside the order-r subgroup.  Python integers (oracle/bigint_ref.py) build the G1 points and the Fq2 arithmetic of the test's own points."""
import ctypes as C
import random

import numpy as np
import pytest

from distributed_plonk_amd import _ffi
from oracle import bigint_ref as B
from oracle import verifier_ref as V

CURVES = ["bn254", "bls12_381"]


def _cid(curve):
    return _ffi.CURVES[curve]


def _q(curve):
    return _ffi.FQ_LIMBS64[_cid(curve)]


def g2_gen(curve):
    out = np.zeros(4 * _q(curve), np.uint64)
    _ffi.check(_ffi.lib().plonk_g2_generator(_cid(curve), out.ctypes.data))
    return out


def g2_mul(curve, s, pt):
    cv = B.CURVES[curve]
    sl = V.fr_limbs(cv, s)
    out = np.zeros(4 * _q(curve), np.uint64)
    _ffi.check(_ffi.lib().plonk_g2_mul(_cid(curve), sl.ctypes.data, pt.ctypes.data, out.ctypes.data))
    return out


def g2_ok(curve, pt):
    ok = C.c_int(-1)
    _ffi.check(_ffi.lib().plonk_g2_check(_cid(curve), np.ascontiguousarray(pt, np.uint64).ctypes.data, C.byref(ok)))
    return ok.value


def g1(curve, s):
    cv = B.CURVES[curve]
    return V.point_limbs(cv, B.scalar_mul(cv, s % cv.fr.p, (cv.gx, cv.gy)) if s % cv.fr.p else B.INF)[0]


def pairing_is_one(curve, pairs):
    g1s = np.concatenate([p for p, _ in pairs]).astype(np.uint64)
    g2s = np.concatenate([q for _, q in pairs]).astype(np.uint64)
    r = C.c_int(-1)
    _ffi.check(_ffi.lib().plonk_pairing_check(_cid(curve), len(pairs), g1s.ctypes.data, g2s.ctypes.data, C.byref(r)))
    return r.value


# ------------------------------------------------------------------------------------------ the test's own Fq2 (u^2 = -1) in integers
def _fq2(curve):
    p = B.CURVES[curve].fq.p
    mul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)
    return p, mul


def g2_decode(curve, pt):
    cv = B.CURVES[curve]
    q = _q(curve)
    c = [cv.fq.from_mont(B.from_limbs([int(x) for x in pt[i * q:(i + 1) * q]])) for i in range(4)]
    return (c[0], c[1]), (c[2], c[3])


def g2_encode(curve, x, y):
    cv = B.CURVES[curve]
    q = _q(curve)
    return np.array(sum((B.to_limbs(cv.fq.to_mont(c), q) for c in (x[0], x[1], y[0], y[1])), []), dtype=np.uint64)


def twist_b(curve):
    p, mul = _fq2(curve)
    x, y = g2_decode(curve, g2_gen(curve))
    x3 = mul(mul(x, x), x)
    yy = mul(y, y)
    return ((yy[0] - x3[0]) % p, (yy[1] - x3[1]) % p)


def fq2_sqrt(curve, a):
    """a square root in Fq2 (p = 3 mod 4 for both curves), or None."""
    p, mul = _fq2(curve)

    def pw(x, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = mul(r, x)
            x = mul(x, x)
            e >>= 1
        return r
    a1 = pw(a, (p - 3) // 4)
    alpha = mul(mul(a1, a1), a)
    x0 = mul(a1, a)
    if alpha == ((p - 1) % p, 0):
        x = mul((0, 1), x0)
    else:
        x = mul(pw(((1 + alpha[0]) % p, alpha[1]), (p - 1) // 2), x0)
    return x if mul(x, x) == (a[0] % p, a[1] % p) else None


def neg_g1(curve, pt):
    cv = B.CURVES[curve]
    q = _q(curve)
    if not pt.any():
        return pt
    y = cv.fq.from_mont(B.from_limbs([int(v) for v in pt[q:]]))
    return np.concatenate([pt[:q], np.array(B.to_limbs(cv.fq.to_mont((-y) % cv.fq.p), q), dtype=np.uint64)])


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("curve", CURVES)
def test_g2_generator_on_twist_and_in_subgroup(curve):
    p, mul = _fq2(curve)
    x, y = g2_decode(curve, g2_gen(curve))
    b = twist_b(curve)
    cv = B.CURVES[curve]
    expect = ((3 * pow(82, -1, p) * 9) % p, (-3 * pow(82, -1, p)) % p) if curve == "bn254" else (4, 4)      # 3/(9+u) and 4(1+u)
    assert b == expect
    assert g2_ok(curve, g2_gen(curve)) == 1
    assert g2_ok(curve, np.zeros(4 * _q(curve), np.uint64)) == 1          # infinity
    assert cv.fr.p.bit_length() in (254, 255)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_mul_matches_repeated_addition_and_r_minus_one_negates(curve):
    H = g2_gen(curve)
    p, mul = _fq2(curve)
    r = B.CURVES[curve].fr.p
    # 2H by the tangent, 3H by the chord, computed here in integers
    x, y = g2_decode(curve, H)
    lam = mul(mul((3, 0), mul(x, x)), _fq2_inv(curve, mul((2, 0), y)))
    x2 = ((mul(lam, lam)[0] - 2 * x[0]) % p, (mul(lam, lam)[1] - 2 * x[1]) % p)
    y2 = _sub(p, mul(lam, _sub(p, x, x2)), y)
    assert np.array_equal(g2_mul(curve, 2, H), g2_encode(curve, x2, y2))
    lam = mul(_sub(p, y2, y), _fq2_inv(curve, _sub(p, x2, x)))
    x3 = _sub(p, _sub(p, mul(lam, lam), x), x2)
    y3 = _sub(p, mul(lam, _sub(p, x, x3)), y)
    assert np.array_equal(g2_mul(curve, 3, H), g2_encode(curve, x3, y3))
    acc = H
    for s in range(2, 6):                     # s H == (s-1) H + H, through the library's own doubling/addition at every step
        nxt = g2_mul(curve, s, H)
        assert g2_ok(curve, nxt) == 1
        acc = nxt
    assert np.array_equal(g2_mul(curve, 1, H), H)
    assert not g2_mul(curve, 0, H).any() and not g2_mul(curve, r, H).any()
    xn, yn = g2_decode(curve, g2_mul(curve, r - 1, H))
    assert xn == x and yn == ((-y[0]) % p, (-y[1]) % p)


def _sub(p, a, b):
    return ((a[0] - b[0]) % p, (a[1] - b[1]) % p)


def _fq2_inv(curve, a):
    p, _ = _fq2(curve)
    t = pow(a[0] * a[0] + a[1] * a[1], -1, p)
    return (a[0] * t % p, (-a[1] * t) % p)


@pytest.mark.parametrize("curve", CURVES)
def test_pairing_bilinear_and_nondegenerate(curve):
    rng = random.Random(7 + len(curve))
    r = B.CURVES[curve].fr.p
    H = g2_gen(curve)
    a, b = rng.randrange(1, r), rng.randrange(1, r)
    # e(aP, bQ) * e(-abP, Q) == 1
    assert pairing_is_one(curve, [(g1(curve, a), g2_mul(curve, b, H)), (g1(curve, -a * b), H)]) == 1
    # e(aP, Q) * e(-P, aQ) == 1
    assert pairing_is_one(curve, [(g1(curve, a), H), (g1(curve, -1), g2_mul(curve, a, H))]) == 1
    # non-degenerate: e(G, H) != 1, and a perturbed product is rejected
    assert pairing_is_one(curve, [(g1(curve, 1), H)]) == 0
    assert pairing_is_one(curve, [(g1(curve, a + 1), g2_mul(curve, b, H)), (g1(curve, -a * b), H)]) == 0
    assert pairing_is_one(curve, [(g1(curve, a), g2_mul(curve, b + 1, H)), (g1(curve, -a * b), H)]) == 0
    # infinity on either side contributes 1; negation in G1 inverts
    assert pairing_is_one(curve, [(np.zeros(2 * _q(curve), np.uint64), H), (g1(curve, 5), np.zeros(4 * _q(curve), np.uint64))]) == 1
    assert pairing_is_one(curve, [(g1(curve, a), H), (neg_g1(curve, g1(curve, a)), H)]) == 1


@pytest.mark.parametrize("curve", CURVES)
def test_twist_point_outside_the_subgroup_is_rejected(curve):
    rng = random.Random(11)
    p, mul = _fq2(curve)
    b = twist_b(curve)
    while True:
        x = (rng.randrange(p), rng.randrange(p))
        y = fq2_sqrt(curve, ((mul(mul(x, x), x)[0] + b[0]) % p, (mul(mul(x, x), x)[1] + b[1]) % p))
        if y is not None:
            break
    pt = g2_encode(curve, x, y)
    assert g2_ok(curve, pt) == 0               # on the twist (the library accepts it as a point), of order not dividing r
    out = g2_mul(curve, 1, pt)                 # plonk_g2_mul accepts twist points: it only checks the equation
    assert np.array_equal(out, pt)
    bad = pt.copy()
    bad[0] ^= np.uint64(1)
    assert g2_ok(curve, bad) == 0              # not on the twist
    r = C.c_int()
    g = g1(curve, 1)
    assert _ffi.lib().plonk_pairing_check(_cid(curve), 1, g.ctypes.data, bad.ctypes.data, C.byref(r)) == -1


def test_bad_arguments_are_refused():
    lib = _ffi.lib()
    r = C.c_int()
    H = g2_gen("bn254")
    assert lib.plonk_g2_generator(7, H.ctypes.data) == -1
    assert lib.plonk_g2_check(0, None, C.byref(r)) == -1
    assert lib.plonk_pairing_check(0, 1, None, H.ctypes.data, C.byref(r)) == -1
    off = g1("bn254", 1)
    off[0] ^= np.uint64(1)
    assert lib.plonk_pairing_check(0, 1, off.ctypes.data, H.ctypes.data, C.byref(r)) == -1
    assert pairing_is_one("bn254", [(g1("bn254", 1), H), (g1("bn254", -1), H)]) == 1
