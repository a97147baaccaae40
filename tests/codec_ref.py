"""Pure-Python reference of the byte codec (distributed_plonk_amd/codec.py, csrc/codec_kernels.hpp, plonk_g2_*_bytes): ark-serialize 0.3's
encodings of G1Affine (compressed and uncompressed), Fr and G2Affine over plain integers, with the status word the library reports for every
input.  It decides: the kernels and the host G2 code are compared with it, never with themselves.

    status 1   no point has this x / the uncompressed pair is off the curve
           2   outside the r-subgroup (G1: BLS12-381 with check_subgroup; G2: always)
           8   non-canonical: a coordinate >= q or scalar >= r, both flags, the infinity flag with a non-zero coordinate, the sign flag in
               an uncompressed element

Points are (x, y) integer pairs (G2: pairs of (c0, c1) pairs), None for infinity.  A decode returns (point or None, status); with a non-zero
status the point is None.
"""
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd.transcript import FQ_MODULI

G1_B = {"bn254": 3, "bls12_381": 4}
NBYTES = {"bn254": 32, "bls12_381": 48}
SIGN, INF = 0x80, 0x40


def fr_modulus(curve):
    return _fr.FIELDS[curve].p


def limbs_of(curve, x, field="q"):
    """the Montgomery limbs (u64, little-endian) the library holds for the residue x"""
    p, n = (FQ_MODULI[curve], NBYTES[curve] // 8) if field == "q" else (fr_modulus(curve), 4)
    v = x * pow(2, 64 * n, p) % p
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)]


def g1_limbs(curve, pt):
    n = NBYTES[curve] // 8
    return [0] * (2 * n) if pt is None else limbs_of(curve, pt[0]) + limbs_of(curve, pt[1])


# ------------------------------------------------------------------------------------------------ G1
def _g1_add(q, p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, q) % q
    x3 = (lam * lam - x1 - x2) % q
    return x3, (lam * (x1 - x3) - y1) % q


def g1_mul(curve, k, pt):
    q, acc = FQ_MODULI[curve], None
    for bit in bin(k)[2:] if k else "":
        acc = _g1_add(q, acc, acc)
        if bit == "1":
            acc = _g1_add(q, acc, pt)
    return acc


def g1_in_subgroup(curve, pt):
    return pt is None or g1_mul(curve, fr_modulus(curve), pt) is None


def g1_encode(curve, pt, encoding="compressed"):
    q, nb = FQ_MODULI[curve], NBYTES[curve]
    if encoding == "compressed":
        if pt is None:
            return bytes(nb - 1) + bytes([INF])
        out = bytearray(pt[0].to_bytes(nb, "little"))
        if pt[1] > (q - pt[1]) % q:
            out[-1] |= SIGN
        return bytes(out)
    if pt is None:
        return bytes(2 * nb - 1) + bytes([INF])
    return pt[0].to_bytes(nb, "little") + pt[1].to_bytes(nb, "little")


def g1_decode(curve, data, encoding="compressed", check_subgroup=True):
    q, nb, b = FQ_MODULI[curve], NBYTES[curve], G1_B[curve]
    unc = encoding == "uncompressed"
    data = bytearray(data)
    assert len(data) == nb * (2 if unc else 1)
    flags = data[-1] & 0xC0
    data[-1] &= 0x3F
    x = int.from_bytes(data[:nb], "little")
    y = int.from_bytes(data[nb:], "little") if unc else 0
    if flags == SIGN | INF or (unc and flags & SIGN):
        return None, 8
    if flags & INF:
        return None, 8 if (x or y) else 0
    if x >= q or y >= q:
        return None, 8
    rhs = (x * x * x + b) % q
    if unc:
        if y * y % q != rhs:
            return None, 1
    else:
        y = pow(rhs, (q + 1) // 4, q)
        if y * y % q != rhs:
            return None, 1
        if (y > (q - y) % q) != bool(flags & SIGN):
            y = (q - y) % q
    if check_subgroup and curve == "bls12_381" and not g1_in_subgroup(curve, (x, y)):
        return None, 2
    return (x, y), 0


# ------------------------------------------------------------------------------------------------ Fr
def fr_encode(curve, v):
    return v.to_bytes(32, "little")


def fr_decode(curve, data):
    v = int.from_bytes(data, "little")
    return (None, 8) if v >= fr_modulus(curve) else (v, 0)


# ------------------------------------------------------------------------------------------------ Fq2 = Fq[u]/(u^2 + 1) and G2 on the twist
def f2_add(q, a, b):
    return (a[0] + b[0]) % q, (a[1] + b[1]) % q


def f2_sub(q, a, b):
    return (a[0] - b[0]) % q, (a[1] - b[1]) % q


def f2_mul(q, a, b):
    return (a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q


def f2_inv(q, a):
    t = pow(a[0] * a[0] + a[1] * a[1], -1, q)
    return a[0] * t % q, -a[1] * t % q


def f2_pow(q, a, e):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = f2_mul(q, acc, acc)
        if bit == "1":
            acc = f2_mul(q, acc, a)
    return acc


def f2_sqrt(q, a):
    """a square root of a, or None: Euler's criterion decides, the norm route finds it"""
    if a == (0, 0):
        return 0, 0
    if f2_pow(q, a, (q * q - 1) // 2) != (1, 0):
        return None
    rt = lambda v: pow(v, (q + 1) // 4, q)
    c0, c1 = a
    if c1 == 0:
        s = rt(c0)
        if s * s % q == c0:
            return s, 0
        s = rt(-c0 % q)
        return 0, s
    alpha = rt((c0 * c0 + c1 * c1) % q)
    half = pow(2, -1, q)
    delta = (c0 + alpha) * half % q
    x0 = rt(delta)
    if x0 * x0 % q != delta:
        delta = (c0 - alpha) * half % q
        x0 = rt(delta)
    r = (x0, c1 * pow(2 * x0, -1, q) % q)
    assert f2_mul(q, r, r) == a
    return r


def g2_b(curve):
    q = FQ_MODULI[curve]
    return f2_mul(q, (3, 0), f2_inv(q, (9, 1))) if curve == "bn254" else (4, 4)


def f2_larger(q, y):
    """y > -y in ark-ff 0.3's ordering of a quadratic extension: c1 first, c0 on a tie"""
    ny = (-y[0] % q, -y[1] % q)
    return (y[1], y[0]) > (ny[1], ny[0])


def _g2_add(q, p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if f2_add(q, y1, y2) == (0, 0):
            return None
        xx = f2_mul(q, x1, x1)
        lam = f2_mul(q, f2_add(q, f2_add(q, xx, xx), xx), f2_inv(q, f2_add(q, y1, y1)))
    else:
        lam = f2_mul(q, f2_sub(q, y2, y1), f2_inv(q, f2_sub(q, x2, x1)))
    x3 = f2_sub(q, f2_sub(q, f2_mul(q, lam, lam), x1), x2)
    return x3, f2_sub(q, f2_mul(q, lam, f2_sub(q, x1, x3)), y1)


def g2_mul(curve, k, pt):
    q, acc = FQ_MODULI[curve], None
    for bit in bin(k)[2:] if k else "":
        acc = _g2_add(q, acc, acc)
        if bit == "1":
            acc = _g2_add(q, acc, pt)
    return acc


def g2_encode(curve, pt, encoding="compressed"):
    q, nb = FQ_MODULI[curve], NBYTES[curve]
    nc = 2 if encoding == "compressed" else 4
    if pt is None:
        return bytes(nc * nb - 1) + bytes([INF])
    (x, y) = pt
    out = bytearray(x[0].to_bytes(nb, "little") + x[1].to_bytes(nb, "little"))
    if nc == 4:
        return bytes(out + y[0].to_bytes(nb, "little") + y[1].to_bytes(nb, "little"))
    if f2_larger(q, y):
        out[-1] |= SIGN
    return bytes(out)


def g2_decode(curve, data):
    q, nb = FQ_MODULI[curve], NBYTES[curve]
    data = bytearray(data)
    nc = len(data) // nb
    assert nc in (2, 4) and len(data) == nc * nb
    flags = data[-1] & 0xC0
    data[-1] &= 0x3F
    c = [int.from_bytes(data[i * nb:(i + 1) * nb], "little") for i in range(nc)]
    if flags == SIGN | INF or (nc == 4 and flags & SIGN):
        return None, 8
    if flags & INF:
        return None, 8 if any(c) else 0
    if any(v >= q for v in c):
        return None, 8
    x = (c[0], c[1])
    rhs = f2_add(q, f2_mul(q, f2_mul(q, x, x), x), g2_b(curve))
    if nc == 4:
        y = (c[2], c[3])
        if f2_mul(q, y, y) != rhs:
            return None, 1
    else:
        y = f2_sqrt(q, rhs)
        if y is None:
            return None, 1
        if f2_larger(q, y) != bool(flags & SIGN):
            y = (-y[0] % q, -y[1] % q)
    if g2_mul(curve, fr_modulus(curve), (x, y)) is not None:
        return None, 2
    return (x, y), 0


def g2_limbs(curve, pt):
    n = NBYTES[curve] // 8
    if pt is None:
        return [0] * (4 * n)
    return limbs_of(curve, pt[0][0]) + limbs_of(curve, pt[0][1]) + limbs_of(curve, pt[1][0]) + limbs_of(curve, pt[1][1])
