"""Vectors and checks of the hot path's limb arithmetic against Python integers, shared by every build of it:

    tests/test_fp29_host.py, tests/test_ec_lazy_host.py   csrc/fp29.hpp, flimb.hpp, ec_lazy.hpp as g++ compiles them (tests/host_cpp)
    tests/test_limb_harness_emu.py                        tests/device_cpp/limb_dev.hip on the emulated HIP runtime (the harness itself)
    tests/test_gpu_limb_arith.py                          tests/device_cpp/limb_dev.hip as gfx950 code

Every check takes the library under test as its first argument: a HostLibs or a DeviceLib below, which give the host files' single-element
entry points and the device harness's batched ones the same (batched) call shapes.  The reference is Python integers throughout; the
acceptance conditions are exact: congruence mod p, normalised limbs, the result bounds the headers state, equality for canonical outputs."""
import ctypes as C
import random

# ------------------------------------------------------------------------------------------------ the libraries under test
U32 = C.c_uint32


def _at(arr, index):
    """pointer to element `index` of a ctypes uint32 array"""
    return C.byref(arr, 4 * index)


class HostLibs:
    """tests/host_cpp/fp29_host.cpp and / or ec_lazy_host.cpp (g++): one element per call where the file has no batch argument"""

    def __init__(self, fp29=None, ecl=None):
        self.fp29, self.ecl = fp29, ecl
        if ecl is not None:
            ecl.ecl_curve_op.restype = C.c_int

    def get_pbar(self, curve, out):
        self.fp29.get_pbar(curve, out)

    def shoup_const(self, curve, c_mont, c29, cq29, n):
        for k in range(n):
            self.fp29.shoup_const(curve, _at(c_mont, 8 * k), _at(c29, 9 * k), _at(cq29, 9 * k))

    def shoup_mul(self, curve, x, c, cq, r, n):
        self.fp29.shoup_mul(curve, x, c, cq, r, C.c_long(n))

    def mont_mul(self, curve, x, cm, r, n):
        self.fp29.mont_mul(curve, x, cm, r, C.c_long(n))

    def canon_lazy(self, curve, x, r, n):
        self.fp29.canon_lazy(curve, x, r, C.c_long(n))

    def ecl_params(self, curve, out):
        self.ecl.ecl_params(curve, out)

    def ecl_field_op(self, curve, op, a, b, c, d, r, n):
        self.ecl.ecl_field_op(curve, op, a, b, c, d, r, C.c_long(n))

    def ecl_curve_op(self, F, op, a, b, out, flag, n):
        bs = curve_b_limbs(F, op)
        for k in range(n):
            flag[k] = self.ecl.ecl_curve_op(F.curve, op, _at(a, 4 * F.NL * k), _at(b, bs * k), _at(out, 4 * F.NL * k))

    def ecl_from_std(self, F, s, out, n):
        for k in range(n):
            self.ecl.ecl_from_std(F.curve, _at(s, F.N * k), _at(out, F.NL * k))

    def ecl_to_std(self, F, s, out, n):
        for k in range(n):
            self.ecl.ecl_to_std(F.curve, _at(s, F.NL * k), _at(out, F.N * k))


class DeviceLib:
    """tests/device_cpp/limb_dev.hip: every entry point is batched, takes the device ordinal first and returns the HIP status"""

    def __init__(self, lib, device=0):
        self.lib, self.device = lib, device
        for name in ("shoup_const", "get_pbar", "shoup_mul", "mont_mul", "canon_lazy", "ecl_params", "ecl_field_op", "ecl_curve_op", "ecl_from_std",
                     "ecl_to_std"):
            getattr(lib, name).restype = C.c_int

    def _call(self, name, *args):
        status = getattr(self.lib, name)(self.device, *args)
        assert status == 0, f"{name}: HIP status {status}"

    def get_pbar(self, curve, out):
        self._call("get_pbar", curve, out)

    def shoup_const(self, curve, c_mont, c29, cq29, n):
        self._call("shoup_const", curve, c_mont, c29, cq29, C.c_long(n))

    def shoup_mul(self, curve, x, c, cq, r, n):
        self._call("shoup_mul", curve, x, c, cq, r, C.c_long(n))

    def mont_mul(self, curve, x, cm, r, n):
        self._call("mont_mul", curve, x, cm, r, C.c_long(n))

    def canon_lazy(self, curve, x, r, n):
        self._call("canon_lazy", curve, x, r, C.c_long(n))

    def ecl_params(self, curve, out):
        self._call("ecl_params", curve, out)

    def ecl_field_op(self, curve, op, a, b, c, d, r, n):
        self._call("ecl_field_op", curve, op, a, b, c, d, r, C.c_long(n))

    def ecl_curve_op(self, F, op, a, b, out, flag, n):
        self._call("ecl_curve_op", F.curve, op, a, b, out, flag, C.c_long(n))

    def ecl_from_std(self, F, s, out, n):
        self._call("ecl_from_std", F.curve, s, out, C.c_long(n))

    def ecl_to_std(self, F, s, out, n):
        self._call("ecl_to_std", F.curve, s, out, C.c_long(n))


# ================================================================================================ Fr: csrc/fp29.hpp
P = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
MASK = (1 << 29) - 1
R256 = 1 << 256


def limbs29(v, top_free=False):
    out = [(v >> (29 * k)) & MASK for k in range(9)]
    if top_free:
        out[8] = v >> (29 * 8)
    return out


def value(l):
    return sum(int(x) << (29 * k) for k, x in enumerate(l))


def lazy_limbs(rng, bound):
    """a value below `bound` written with un-normalised limbs below 2^31 (what a butterfly hands to its product)"""
    v = rng.randrange(bound)
    l = limbs29(v, top_free=True)
    for k in range(8):
        d = min(l[k + 1], 3, ((1 << 31) - 1 - l[k]) >> 29)
        d = rng.randrange(d + 1) if d > 0 else 0
        l[k] += d << 29
        l[k + 1] -= d
    assert value(l) == v and all(0 <= x < (1 << 31) for x in l)
    return l, v


# operands that have failed on some build join these lists, so that every build carries them
SHOUP_EDGE_C = lambda p: [0, 1, 2, p - 1, p - 2, (p + 1) // 2, 1 << 253]
SHOUP_EDGE_X = lambda p, bound: [0, 1, p - 1, p, 2 * p, bound - 1]


def check_shoup_multiplier_against_integers(lib, curve, n, mont_stride=7):
    """n operand pairs: the first 64 are the edge grid, the rest random.  The Montgomery product is checked on every `mont_stride`-th pair
    (7 where n is large and the Python integers are the cost; 1 checks every result)."""
    p = P[curve]
    rng = random.Random(0x5A0F + curve)
    # BN254: f29_mul's documented contract.  BLS12-381 (p = 2^254.86): the Shoup butterflies reach 1.6p + 4p * 9 < 38p there, so both
    # multipliers are checked up to 40p = 2^260.2 (the Shoup quotient estimate needs x < 2^261; the Montgomery result is < x*p/2^261 + p < 2p)
    bound = int(2 ** 259.4) if curve == 0 else 40 * p
    pbar = (U32 * 9)()
    lib.get_pbar(curve, pbar)
    assert value(pbar) == (1 << 261) - p and all(x <= MASK for x in pbar)
    edge_c = SHOUP_EDGE_C(p)
    edge_x = SHOUP_EDGE_X(p, bound)
    xs, cs, vals = [], [], []
    for i in range(n):
        c = edge_c[i % len(edge_c)] if i < 64 else rng.randrange(p)
        if i < 64:
            xv = edge_x[(i // len(edge_c)) % len(edge_x)]
            xl = limbs29(xv, top_free=True)
        else:
            xl, xv = lazy_limbs(rng, bound)
        xs.append(xl); cs.append(c); vals.append(xv)
    A = (U32 * (9 * n))(*[w for l in xs for w in l])
    c29, cq29 = (U32 * (9 * n))(), (U32 * (9 * n))()
    # the reference's Montgomery form, as the tables are built from
    c8 = (U32 * (8 * n))(*[((c * R256 % p) >> (32 * i)) & 0xffffffff for c in cs for i in range(8)])
    lib.shoup_const(curve, c8, c29, cq29, n)
    for k, c in enumerate(cs):
        assert value(c29[9 * k:9 * k + 9]) == c and value(cq29[9 * k:9 * k + 9]) == (c << 261) // p, "prepared constant"
    R = (U32 * (9 * n))()
    lib.shoup_mul(curve, A, c29, cq29, R, n)
    for k in range(n):
        r = R[9 * k:9 * k + 9]
        assert all(x <= MASK for x in r), "normalised limbs"
        rv = value(r)
        assert rv % p == vals[k] * cs[k] % p, (curve, k)
        assert 0 <= rv < 3 * p, (curve, k, rv / p)
    cm = (U32 * (9 * n))(*[w for c in cs for w in limbs29((c << 261) % p)])
    M = (U32 * (9 * n))()
    lib.mont_mul(curve, A, cm, M, n)
    for k in range(0, n, mont_stride):
        mv = value(M[9 * k:9 * k + 9])
        assert mv % p == vals[k] * cs[k] % p and mv < 2 * p


def check_canon_lazy_up_to_48p(lib, curve, n):
    p = P[curve]
    rng = random.Random(77 + curve)
    top = min(48 * p, (1 << 261) - 1)
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 24 * p, 36 * p + 5, top - 1] + [k * p + d for k in range(1, 48) for d in (-1, 0, 1) if 0 <= k * p + d < top]
    vals += [rng.randrange(top) for _ in range(n - len(vals))]
    A = (U32 * (9 * len(vals)))(*[w for v in vals for w in limbs29(v, top_free=True)])
    Rr = (U32 * (9 * len(vals)))()
    lib.canon_lazy(curve, A, Rr, len(vals))
    for k, v in enumerate(vals):
        r = Rr[9 * k:9 * k + 9]
        assert value(r) == v % p and all(x <= MASK for x in r), (curve, v // p)


# ================================================================================================ Fq and the curve: csrc/flimb.hpp, ec_lazy.hpp
GEOM = {
    0: dict(name="bn254", NL=9, B=29, N=8, b=3, g=(1, 2),
            p=21888242871839275222246405745257275088696311157297823662689037894645226208583),
    1: dict(name="bls12_381", NL=14, B=28, N=12, b=4,
            g=(0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
               0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
            p=0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab),
}
# ec_lazy.hpp's accumulator invariants, in units of p
BOUND = dict(x=5.2, y=3.3, zz=2.0, zzz=2.0)


class Field:
    def __init__(self, curve):
        g = GEOM[curve]
        self.curve, self.NL, self.B, self.N, self.p = curve, g["NL"], g["B"], g["N"], g["p"]
        self.Rp = 1 << (self.B * self.NL)              # R'
        self.R = 1 << (32 * self.N)                    # the reference's Montgomery radix
        self.mask = (1 << self.B) - 1

    def limbs(self, v):
        """normalised limbs: B bits each, the excess in the top limb"""
        out = [(v >> (self.B * k)) & self.mask for k in range(self.NL - 1)]
        top = v >> (self.B * (self.NL - 1))
        assert top < (1 << 32), "value does not fit the limb form"
        return out + [top]

    def value(self, l):
        return sum(int(x) << (self.B * k) for k, x in enumerate(l))

    def normalised(self, l):
        return all(int(x) <= self.mask for x in l[:-1])

    def enc(self, x, lift=0):
        """x (plain residue) -> limbs of x*R' mod p + lift*p"""
        return self.limbs(x * self.Rp % self.p + lift * self.p)

    def dec(self, l):
        return self.value(l) * pow(self.Rp, -1, self.p) % self.p

    def arr(self, rows):
        flat = [w for r in rows for w in r]
        return (U32 * len(flat))(*flat)


# ------------------------------------------------------------------------------------------------ affine integers
def ec_add(F, P, Q):
    p = F.p
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def ec_neg(F, P):
    return None if P is None else (P[0], (-P[1]) % F.p)


def ec_mul(F, k, P):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(F, acc, P)
        P = ec_add(F, P, P)
        k >>= 1
    return acc


def points(F, rng, count):
    g = GEOM[F.curve]
    assert (g["g"][1] ** 2 - g["g"][0] ** 3 - g["b"]) % F.p == 0
    return [ec_mul(F, rng.randrange(1, 1 << 64), g["g"]) for _ in range(count)]


# ------------------------------------------------------------------------------------------------ limb-form points
def aff_limbs(F, P, lift_y=0):
    if P is None:
        return [0] * (2 * F.NL)
    return F.enc(P[0]) + F.enc(P[1], lift_y)


def acc_limbs(F, P, rng=None, lift=None):
    """an XYZZ accumulator of the group element P with a random Z (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2); `lift` = (kx, ky, kzz, kzzz)
    multiples of p added to the canonical residues"""
    if P is None:
        return [0] * (4 * F.NL)
    z = rng.randrange(1, F.p) if rng else 1
    zz, zzz = z * z % F.p, z * z * z % F.p
    kx, ky, kzz, kzzz = lift or (0, 0, 0, 0)
    return F.enc(P[0] * zz % F.p, kx) + F.enc(P[1] * zzz % F.p, ky) + F.enc(zz, kzz) + F.enc(zzz, kzzz)


def acc_point(F, l, where=""):
    """checks the invariants of ec_lazy.hpp on an accumulator and returns its group element"""
    NL, p = F.NL, F.p
    X, Y, ZZ, ZZZ = (l[i * NL:(i + 1) * NL] for i in range(4))
    if all(int(w) == 0 for w in ZZ):
        return None
    for name, c in (("x", X), ("y", Y), ("zz", ZZ), ("zzz", ZZZ)):
        assert F.normalised(c), (where, name, "limbs not normalised")
        assert F.value(c) < BOUND[name] * p, (where, name, F.value(c) / p)
    zz, zzz = F.dec(ZZ), F.dec(ZZZ)
    assert zz % p != 0 and pow(zz, 3, p) == zzz * zzz % p, (where, "ZZ^3 != ZZZ^2")
    return F.dec(X) * pow(zz, -1, p) % p, F.dec(Y) * pow(zzz, -1, p) % p


MADD_FAST, MADD_FUSED, MADD, ADD, ADD_FAST, DBL, DBL_AFF, NEG = range(8)


def curve_b_limbs(F, op):
    """limbs of a curve operation's second operand: an accumulator for add, add_fast and dbl, an affine point otherwise"""
    return (4 if op in (ADD, ADD_FAST, DBL) else 2) * F.NL


def run_batch(lib, F, op, a_rows, b_rows):
    """one operation on len(a_rows) operand sets -> (flags, result rows of 4 NL limbs)"""
    n = len(a_rows)
    assert len(b_rows) == n and all(len(r) == 4 * F.NL for r in a_rows) and all(len(r) >= curve_b_limbs(F, op) for r in b_rows)
    out = (U32 * (4 * F.NL * n))()
    flag = (C.c_int32 * n)(*([-2] * n))
    lib.ecl_curve_op(F, op, F.arr(a_rows), F.arr([r[:curve_b_limbs(F, op)] for r in b_rows]), out, flag, n)
    assert all(f >= 0 for f in flag)
    return list(flag), [list(out[4 * F.NL * k:4 * F.NL * (k + 1)]) for k in range(n)]


def run(lib, F, op, a, b):
    flags, outs = run_batch(lib, F, op, [a], [b])
    return flags[0], outs[0]


# ------------------------------------------------------------------------------------------------ checks
def check_limb_parameters(lib, curve):
    F = Field(curve)
    NL, p = F.NL, F.p
    raw = (U32 * (8 * NL + 1))()
    lib.ecl_params(curve, raw)
    row = lambda i: [int(x) for x in raw[i * NL:(i + 1) * NL]]
    pl, p2, c2, c4, c8, one, r_std, r2fix = (row(i) for i in range(8))
    assert F.value(pl) == p and F.normalised(pl) and F.value(p2) == 2 * p and F.normalised(p2)
    for k, c in ((2, c2), (4, c4), (8, c8)):
        assert F.value(c) == k * p                      # the lift moves 2^31 into every limb without changing the value
        # a + C - b must not underflow in any limb for b limbs < 3 * 2^B (PPP + 2Q is the widest subtrahend of ec_lazy.hpp)
        assert all(x >= 3 << F.B for x in c[:-1]) and c[-1] < (1 << 31)
    assert F.value(one) == F.Rp % p and F.value(r_std) == F.R % p
    assert F.value(r2fix) == F.Rp * F.Rp * pow(F.R, -1, p) % p
    assert (int(raw[8 * NL]) * pl[0] + 1) % (1 << F.B) == 0          # inv = -p^-1 mod 2^B


# operand ranges of the curve formulas: P < 9.2p, T < 9.1p, R < 5.2p, accumulator X < 5.2p, (4p - Y) < 4p + ...
FIELD_EDGE = lambda p: [0, 1, p - 1, p, p + 1, 2 * p, int(9.2 * p) - 1, int(5.2 * p) - 1]


def check_field_products_up_to_the_lazy_bounds(lib, curve, n):
    F = Field(curve)
    p, NL = F.p, F.NL
    rng = random.Random(0xF1 + curve)
    Rinv = pow(F.Rp, -1, p)
    top = int(9.2 * p)
    edge = FIELD_EDGE(p)

    def operands(k, bound):
        return [edge[(i // (len(edge) ** k)) % len(edge)] % bound if i < len(edge) ** 2 else rng.randrange(bound) for i in range(n)]

    a, b = operands(0, top), operands(1, top)
    out = (U32 * (NL * n))()
    lib.ecl_field_op(curve, 0, F.arr([F.limbs(v) for v in a]), F.arr([F.limbs(v) for v in b]), None, None, out, n)
    for k in range(n):
        r = out[NL * k:NL * k + NL]
        v = F.value(r)
        assert F.normalised(r) and v % p == a[k] * b[k] * Rinv % p and v < a[k] * b[k] // F.Rp + p + 1, ("mul", k)
    lib.ecl_field_op(curve, 1, F.arr([F.limbs(v) for v in a]), None, None, None, out, n)
    for k in range(n):
        r = out[NL * k:NL * k + NL]
        v = F.value(r)
        assert F.normalised(r) and v % p == a[k] * a[k] * Rinv % p and v < a[k] * a[k] // F.Rp + p + 1, ("sqr", k)
    # Y3 = R*T + (4p - Y1)*PPP under one reduction: R < 5.2p, T < 9.1p, 4p - Y1 < 4p (lifted: up to 4p + 2^31 in the limbs' slack), PPP < 1.1p
    r_, t_ = [rng.randrange(int(5.2 * p)) for _ in range(n)], [rng.randrange(int(9.1 * p)) for _ in range(n)]
    ny, pp_ = [rng.randrange(4 * p + 1) for _ in range(n)], [rng.randrange(int(1.1 * p)) for _ in range(n)]
    r_[0], t_[0], ny[0], pp_[0] = int(5.2 * p) - 1, int(9.1 * p) - 1, 4 * p, int(1.1 * p) - 1
    lib.ecl_field_op(curve, 2, F.arr([F.limbs(v) for v in r_]), F.arr([F.limbs(v) for v in t_]), F.arr([F.limbs(v) for v in ny]),
                     F.arr([F.limbs(v) for v in pp_]), out, n)
    for k in range(n):
        r = out[NL * k:NL * k + NL]
        v = F.value(r)
        s = r_[k] * t_[k] + ny[k] * pp_[k]
        assert F.normalised(r) and v % p == s * Rinv % p and v < s // F.Rp + p + 1, ("dot2", k)
        assert v < 1.4 * p                                                            # the bound xyzzl_madd_fast<FUSED_Y3> relies on


def check_standard_form_round_trip(lib, curve, count):
    """bases_to_limbs_kernel / store_std: the reference's R = 2^(32N) Montgomery residues <-> the resident R' limb form"""
    F = Field(curve)
    rng = random.Random(5 + curve)
    xs = [0, 1, F.p - 1] + [rng.randrange(F.p) for _ in range(count)]
    n = len(xs)
    stds = [x * F.R % F.p for x in xs]
    s = (U32 * (F.N * n))(*[(std >> (32 * i)) & 0xffffffff for std in stds for i in range(F.N)])
    l = (U32 * (F.NL * n))()
    lib.ecl_from_std(F, s, l, n)
    rows = [l[F.NL * k:F.NL * (k + 1)] for k in range(n)]
    for x, row in zip(xs, rows):
        assert F.value(row) == x * F.Rp % F.p and F.normalised(row)
    for lift in (0, 1):                                                                # store_std takes lazy values
        back = (U32 * (F.N * n))()
        lib.ecl_to_std(F, F.arr([F.limbs(F.value(row) + lift * F.p) for row in rows]), back, n)
        for k, std in enumerate(stds):
            assert sum(int(w) << (32 * i) for i, w in enumerate(back[F.N * k:F.N * (k + 1)])) == std


def check_bucket_accumulation_chain(lib, curve):
    """What one lane of msm_accumulate_kernel does: a run of mixed additions of +/- bases into an XYZZ accumulator, both Y3
    formulations, invariants after every step; the same-x cases abort untouched and are finished by the complete formula."""
    F = Field(curve)
    rng = random.Random(0xACC + curve)
    pts = points(F, rng, 24)
    for fused in (MADD_FAST, MADD_FUSED):
        acc, want = [0] * (4 * F.NL), None
        for step in range(160):
            P = pts[rng.randrange(len(pts))]
            q = aff_limbs(F, P)
            if rng.random() < 0.5:                                                     # a negative digit: y -> 2p - y, in (p, 2p]
                _, qn = run(lib, F, NEG, acc, q)
                q = qn[:2 * F.NL]
                assert F.value(q[F.NL:]) == 2 * F.p - P[1] * F.Rp % F.p and F.normalised(q[F.NL:])
                P = ec_neg(F, P)
            ok, new = run(lib, F, fused, acc, q)
            if want is not None and want[0] == P[0]:                                   # P + P or P + (-P): the fast path must refuse
                assert ok == 0 and new == acc, "same-x addition must leave the accumulator untouched"
                ok, new = run(lib, F, MADD, acc, q)                                    # msm_accumulate_redo_kernel
            assert ok == 1
            want = ec_add(F, want, P)
            acc = new
            assert acc_point(F, acc, (fused, step)) == want
        assert want is not None


def check_exceptional_cases(lib, curve):
    F = Field(curve)
    rng = random.Random(0xE + curve)
    P, Q = points(F, rng, 2)
    inf_acc, inf_aff = [0] * (4 * F.NL), [0] * (2 * F.NL)
    a = acc_limbs(F, P, rng)
    # mixed: acc + infinity base (complete path only; the kernel filters infinity for the fast one), infinity acc + base
    assert acc_point(F, run(lib, F, MADD, a, inf_aff)[1]) == P
    for op in (MADD_FAST, MADD_FUSED, MADD):
        ok, o = run(lib, F, op, inf_acc, aff_limbs(F, Q))
        assert ok == 1 and acc_point(F, o) == Q
    # mixed doubling and cancellation
    for op in (MADD_FAST, MADD_FUSED):
        assert run(lib, F, op, a, aff_limbs(F, P))[0] == 0
        assert run(lib, F, op, a, aff_limbs(F, ec_neg(F, P)))[0] == 0
    assert acc_point(F, run(lib, F, MADD, a, aff_limbs(F, P))[1]) == ec_add(F, P, P)
    assert acc_point(F, run(lib, F, MADD, a, aff_limbs(F, ec_neg(F, P)))[1]) is None
    assert acc_point(F, run(lib, F, DBL_AFF, inf_acc, aff_limbs(F, P))[1]) == ec_add(F, P, P)
    # accumulator + accumulator (the pyramid, the heavy-bucket tree, msm_points_sum_kernel)
    b = acc_limbs(F, Q, rng)
    same, opp = acc_limbs(F, P, rng), acc_limbs(F, ec_neg(F, P), rng)           # other Z: a different representation of the same x
    assert acc_point(F, run(lib, F, ADD, a, b)[1]) == ec_add(F, P, Q)
    ok, o = run(lib, F, ADD_FAST, a, b)
    assert ok == 1 and acc_point(F, o) == ec_add(F, P, Q)
    assert acc_point(F, run(lib, F, ADD, a, same)[1]) == ec_add(F, P, P)
    assert acc_point(F, run(lib, F, ADD, a, opp)[1]) is None
    for other in (same, opp):
        ok, o = run(lib, F, ADD_FAST, a, other)
        assert ok == 0 and o == a
    assert acc_point(F, run(lib, F, ADD, a, inf_acc)[1]) == P and acc_point(F, run(lib, F, ADD, inf_acc, b)[1]) == Q
    for x, y, w in ((a, inf_acc, P), (inf_acc, b, Q), (inf_acc, inf_acc, None)):
        ok, o = run(lib, F, ADD_FAST, x, y)
        assert ok == 1 and acc_point(F, o) == w
    assert acc_point(F, run(lib, F, DBL, a, a)[1]) == ec_add(F, P, P)
    assert acc_point(F, run(lib, F, DBL, inf_acc, inf_acc)[1]) is None


# (kx, ky, kzz, kzzz): canonical residue plus the largest multiple of p that fits the invariants, and partial lifts
LIFTS = [(4, 2, 1, 1), (4, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 1), (3, 1, 1, 0)]


def check_operands_at_the_top_of_their_ranges(lib, curve):
    """The bound bookkeeping of ec_lazy.hpp: accumulators whose coordinates sit just under the stated invariants (X < 5.2p, Y < 3.3p,
    ZZ, ZZZ < 2p — canonical residue plus the largest multiple of p that fits) and negated bases (y in (p, 2p]) still give the right
    group element and results INSIDE the invariants: no column accumulator wrapped, no lifted subtraction underflowed."""
    F = Field(curve)
    rng = random.Random(0xB0 + curve)
    pts = points(F, rng, 12)
    lifts = LIFTS
    for trial in range(40):
        P, Q = rng.sample(pts, 2)
        la, lb = lifts[trial % len(lifts)], lifts[(trial // len(lifts)) % len(lifts)]
        a, b = acc_limbs(F, P, rng, la), acc_limbs(F, Q, rng, lb)
        assert acc_point(F, a, "lifted a") == P and acc_point(F, b, "lifted b") == Q
        q = aff_limbs(F, Q)
        if trial & 1:
            q = run(lib, F, NEG, a, q)[1][:2 * F.NL]
        Qs = ec_neg(F, Q) if trial & 1 else Q
        for op in (MADD_FAST, MADD_FUSED, MADD):
            ok, o = run(lib, F, op, a, q)
            assert ok == 1 and acc_point(F, o, (op, trial)) == ec_add(F, P, Qs)
        for op in (ADD, ADD_FAST):
            ok, o = run(lib, F, op, a, b)
            assert ok == 1 and acc_point(F, o, (op, trial)) == ec_add(F, P, Q)
        assert acc_point(F, run(lib, F, DBL, a, a)[1], ("dbl", trial)) == ec_add(F, P, P)
        assert acc_point(F, run(lib, F, MADD, a, aff_limbs(F, P, lift_y=0))[1], ("madd dbl", trial)) == ec_add(F, P, P)
        same = acc_limbs(F, P, rng, lb)
        assert acc_point(F, run(lib, F, ADD, a, same)[1], ("add dbl", trial)) == ec_add(F, P, P)


def check_reduction_pyramid_chunk(lib, curve):
    """One lane of msm_reduce_level_kernel: over a strided chunk E_0 .. E_(K-1) it emits acc = sum_t t * E_t and S = sum_t E_t
    with 2K additions; the identity  sum_j (j+1) E_j = sum_ch (ch+1) S_ch + nch * sum_ch acc_ch  the host's Horner relies on is
    checked on a small window of buckets."""
    F = Field(curve)
    rng = random.Random(0x9e + curve)
    K, nch = 4, 3
    nb = K * nch
    pts = points(F, rng, nb)
    pts[5] = None                                                                      # an empty bucket
    E = [acc_limbs(F, P, rng) for P in pts]
    inf = [0] * (4 * F.NL)
    S, A = [], []
    for ch in range(nch):
        running, acc = inf, inf
        for d in reversed(range(K)):
            ok, acc = run(lib, F, ADD_FAST, acc, running)
            assert ok == 1
            ok, running = run(lib, F, ADD_FAST, running, E[ch + d * nch])
            assert ok == 1
        S.append(acc_point(F, running, ("S", ch)))
        A.append(acc_point(F, acc, ("A", ch)))
        want_s, want_a = None, None
        for t in range(K):
            want_s = ec_add(F, want_s, pts[ch + t * nch])
            want_a = ec_add(F, want_a, ec_mul(F, t, pts[ch + t * nch]) if pts[ch + t * nch] else None)
        assert S[ch] == want_s and A[ch] == want_a
    lhs = None
    for j, P in enumerate(pts):
        lhs = ec_add(F, lhs, ec_mul(F, j + 1, P) if P else None)
    rhs = None
    for ch in range(nch):
        rhs = ec_add(F, rhs, ec_mul(F, ch + 1, S[ch]) if S[ch] else None)
        rhs = ec_add(F, rhs, ec_mul(F, nch, A[ch]) if A[ch] else None)
    assert lhs == rhs


def check_random_curve_ops_in_batches(lib, curve, op, n):
    """`n` operand sets of one curve operation in ONE call (the device harness: one set per lane): random group elements from a pool that
    repeats (so P + P and P - P occur), random Z, lifts up to the top of the invariants, negated bases (y in (p, 2p]) and points at
    infinity where the kernels allow them.  Result, flag and invariants of every set against the affine integer group law; a fast path
    that refuses must hand its accumulator back untouched."""
    F = Field(curve)
    rng = random.Random(0xBA7C4 + 16 * op + curve)
    pts = points(F, rng, 48)
    second_is_acc = op in (ADD, ADD_FAST, DBL)
    a_rows, b_rows, want = [], [], []
    for k in range(n):
        P = None if rng.random() < 0.03 else rng.choice(pts)
        Q = rng.choice(pts)
        if rng.random() < 0.04 and P is not None:                  # the same x on purpose: Q = P or Q = -P
            Q = P
        if rng.random() < 0.5:
            Q = ec_neg(F, Q)
        a = acc_limbs(F, P, rng, rng.choice(LIFTS + [None]))
        if second_is_acc:
            if op == ADD_FAST or op == ADD:
                Q = None if rng.random() < 0.03 else Q
            b = a if op == DBL else acc_limbs(F, Q, rng, rng.choice(LIFTS + [None]))
        else:
            if op == MADD and rng.random() < 0.03:
                Q = None                                           # an infinity base: the complete path only
            b = aff_limbs(F, Q)
            if Q is not None and op != NEG and rng.random() < 0.5:  # the form affl_neg leaves: y = 2p - (-y) in (p, 2p]
                b = b[:F.NL] + F.limbs(2 * F.p - F.value(aff_limbs(F, ec_neg(F, Q))[F.NL:]))
        a_rows.append(a); b_rows.append(b); want.append((P, Q))
    flags, outs = run_batch(lib, F, op, a_rows, b_rows)
    for k, ((P, Q), a, b, ok, o) in enumerate(zip(want, a_rows, b_rows, flags, outs)):
        where = (op, k)
        if op == NEG:
            assert ok == 1 and o[:F.NL] == b[:F.NL] and F.normalised(o[F.NL:2 * F.NL]), where
            assert F.value(o[F.NL:2 * F.NL]) == 2 * F.p - Q[1] * F.Rp % F.p, where
        elif op == DBL:
            assert ok == 1 and acc_point(F, o, where) == ec_add(F, P, P), where
        elif op == DBL_AFF:
            assert ok == 1 and acc_point(F, o, where) == ec_add(F, Q, Q), where
        elif op in (MADD, ADD):
            assert ok == 1 and acc_point(F, o, where) == ec_add(F, P, Q), where
        elif P is not None and Q is not None and P[0] == Q[0]:    # the fast paths refuse the same x
            assert ok == 0 and o == a, where
        else:
            assert ok == 1 and acc_point(F, o, where) == ec_add(F, P, Q), where
