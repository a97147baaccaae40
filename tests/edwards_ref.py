"""A pure-Python reference of the embedded twisted Edwards curves and of Schnorr signatures over them (a helper of the Edwards tests, not a
test; imports no project code — the hash is tests/rescue_ref.py's).

    E:  a x^2 + y^2 = 1 + d x^2 y^2  over Fr;   (x1, y1) + (x2, y2) = ( (x1 y2 + y1 x2) / (1 + d t),  (y1 y2 - a x1 x2) / (1 - d t) ),  t = x1 x2 y1 y2

written from the definition with Python integers and pow: the affine law for everything, double-and-add for [k] P.  Baby Jubjub over
BN254's Fr, Jubjub over BLS12-381's; both have cofactor 8 and a generator G of prime order l.

    Schnorr:  pk = [sk] G;  R = [nonce] G,  c = hash3(hash3(R.x, R.y, pk.x), pk.y, m),  s = nonce + c sk mod l;
              verify: s < l, R and pk on E, [s] G = R + [c] pk          (c multiplies as the integer in [0, r))"""
import random

from tests import rescue_ref as R

MODULI = R.MODULI
CURVES = R.CURVES
IDENTITY = (0, 1)

PARAMS = {
    "bn254": dict(a=168700, d=168696, cofactor=8,
                  l=2736030358979909402780800718157159386076813972158567259200215660948447373041,
                  G=(5299619240641551281634865583518297030282874472190772894086521144482721001553,
                     16950150798460657717958625567821834550301663161624707787222815936182638968203)),
    "bls12_381": dict(a=MODULI["bls12_381"] - 1, d=-10240 * pow(10241, -1, MODULI["bls12_381"]) % MODULI["bls12_381"], cofactor=8,
                      l=0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7,
                      G=(26425721312295396735536009845259662215154440146657062145727563247428679108070,
                         33870355149453697655464584064870436861767017640968433840972803788419917420560)),
}


def params(curve, prm=None):
    return prm or PARAMS[curve]


def on_curve(curve, P, prm=None) -> bool:
    r, c = MODULI[curve], params(curve, prm)
    x, y = P
    return (c["a"] * x * x + y * y - 1 - c["d"] * x * x * y * y) % r == 0


def add(curve, P, Q, prm=None):
    r, c = MODULI[curve], params(curve, prm)
    (x1, y1), (x2, y2) = P, Q
    t = c["d"] * x1 * x2 * y1 * y2 % r
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, r) % r, (y1 * y2 - c["a"] * x1 * x2) * pow(1 - t, -1, r) % r


def neg(curve, P):
    return (-P[0]) % MODULI[curve], P[1]


def mul(curve, k: int, P, prm=None):
    assert k >= 0
    acc, base = IDENTITY, P
    while k:
        if k & 1:
            acc = add(curve, acc, base, prm)
        base = add(curve, base, base, prm)
        k >>= 1
    return acc


def in_subgroup(curve, P, prm=None) -> bool:
    return on_curve(curve, P, prm) and mul(curve, params(curve, prm)["l"], P, prm) == IDENTITY


def sqrt(curve, n: int):
    """a square root of n mod r, or None (Tonelli-Shanks)"""
    r = MODULI[curve]
    n %= r
    if n == 0:
        return 0
    if pow(n, (r - 1) // 2, r) != 1:
        return None
    q, s = r - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (r - 1) // 2, r) != r - 1:
        z += 1
    m, c, t, x = s, pow(z, q, r), pow(n, q, r), pow(n, (q + 1) // 2, r)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % r, i + 1
        b = pow(c, 1 << (m - i - 1), r)
        m, c = i, b * b % r
        t, x = t * c % r, x * b % r
    return x


def point_with_y(curve, y: int, prm=None):
    """the curve point with this y and the smaller x, or None: x^2 = (1 - y^2) / (a - d y^2)"""
    r, c = MODULI[curve], params(curve, prm)
    den = (c["a"] - c["d"] * y * y) % r
    if den == 0:
        return None
    x = sqrt(curve, (1 - y * y) * pow(den, -1, r))
    return None if x is None else (min(x, r - x), y % r)


def random_point(curve, rnd: random.Random, prm=None):
    """a point of E, uniform up to the choice of x's sign: in the subgroup of order l with probability 1 / 8"""
    r = MODULI[curve]
    while True:
        P = point_with_y(curve, rnd.randrange(r), prm)
        if P is not None:
            return P if rnd.random() < 0.5 else neg(curve, P)


def small_order_points(curve, prm=None):
    """-> {2: (0, -1), 4: a point of order 4, 8: a point of order 8}"""
    r, c = MODULI[curve], params(curve, prm)
    out = {2: (0, r - 1)}
    rnd = random.Random("small order " + curve)
    while 8 not in out:
        T = mul(curve, c["l"], random_point(curve, rnd, prm), prm)
        if mul(curve, 4, T, prm) != IDENTITY:
            out[8] = T
    out[4] = add(curve, out[8], out[8], prm)
    assert add(curve, out[4], out[4], prm) == out[2]
    return out


def challenge(curve, Rp, pk, m: int, rescue=None) -> int:
    h = R.permute(curve, [Rp[0], Rp[1], pk[0], 0], rescue)[0]
    return R.permute(curve, [h, pk[1], m, 0], rescue)[0]


def schnorr_sign(curve, sk: int, nonce: int, m: int, prm=None, rescue=None):
    """-> (R, s)"""
    c = params(curve, prm)
    pk, Rp = mul(curve, sk, c["G"], prm), mul(curve, nonce, c["G"], prm)
    return Rp, (nonce + challenge(curve, Rp, pk, m, rescue) * sk) % c["l"]


def schnorr_verify(curve, pk, m: int, sig, prm=None, rescue=None) -> bool:
    c = params(curve, prm)
    Rp, s = sig
    if not (0 <= s < c["l"] and on_curve(curve, Rp, prm) and on_curve(curve, pk, prm)):
        return False
    return mul(curve, s, c["G"], prm) == add(curve, Rp, mul(curve, challenge(curve, Rp, pk, m, rescue), pk, prm), prm)
