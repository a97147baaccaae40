"""poly_ops.hip where uniformly random data at small sizes does not reach: the second level of every kernel at the smallest size that has one
(two scan tiles per lane of scan_top_kernel, a second trip of fr_sum_kernel, three division tiles per lane of poly_div_top_kernel, the third
level of a SCALED power table), lengths on either side of every tile seam, the largest values the lazy 29-bit arithmetic is specified for,
evaluation points at which whole constant tables collapse to one, a vanishing numerator, and plonk_class_interleave_dev on its own.

Every comparison is bit-exact against the CPU oracle (oracle/oracle.py), with the moduli taken from oracle/bigint_ref.py.  Two readings of
"p - 1" are used side by side: the field element -1 (Montgomery limbs of p - 1) and the limb pattern p - 1 itself, the largest canonical
word a kernel can load (what tests/test_gpu_ntt.py and tests/test_gpu_quotient.py call p - 1)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
PIECE = 1 << 18          # gates per piece of the host-side reference of the large permutation products


class _Field:
    """Montgomery-limb arithmetic on (k, 4) uint64 arrays through oracle.field_op; a (4,) operand is broadcast."""

    def __init__(self, oracle, curve, cid):
        from oracle import bigint_ref as B
        self.o, self.cid, self.p = oracle, cid, B.CURVES[curve].fr.p
        self.zero = np.zeros(4, dtype=np.uint64)
        self.one = oracle.field_const(cid, 0, 1)[:4].copy()
        self.minus_one = self.sub(self.zero, self.one)                                     # the field element p - 1
        self.top = np.array(B.to_limbs(self.p - 1, 4), dtype=np.uint64)                    # the limb pattern p - 1
        assert B.from_limbs(oracle.from_mont(cid, self.minus_one.reshape(1, 4))[0]) == self.p - 1
        assert B.from_limbs(oracle.from_mont(cid, self.one.reshape(1, 4))[0]) == 1

    def _op(self, op, a, b=None):
        a = np.asarray(a, dtype=np.uint64)
        single = a.ndim == 1 and (b is None or np.ndim(b) == 1)
        a = a.reshape(-1, 4)
        if b is not None:
            b = np.asarray(b, dtype=np.uint64).reshape(-1, 4)
            k = max(a.shape[0], b.shape[0])
            a, b = np.broadcast_to(a, (k, 4)), np.broadcast_to(b, (k, 4))
        out = self.o.field_op(self.cid, 0, op, a, b)
        return out[0] if single else out

    def mul(self, a, b): return self._op("mul", a, b)
    def add(self, a, b): return self._op("add", a, b)
    def sub(self, a, b): return self._op("sub", a, b)
    def inv(self, a): return self._op("inv", a)

    def pow(self, base, e):
        """square and multiply"""
        r, b = self.one, np.asarray(base, dtype=np.uint64)
        while e:
            if e & 1:
                r = self.mul(r, b)
            b = self.mul(b, b)
            e >>= 1
        return r

    def full(self, v, n):
        return np.tile(np.asarray(v, dtype=np.uint64), (n, 1))

    def canonical(self, a):
        """every row < p as a 256-bit integer"""
        pl = [(self.p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        a = a.reshape(-1, 4)
        lt, eq = np.zeros(a.shape[0], dtype=bool), np.ones(a.shape[0], dtype=bool)
        for i in (3, 2, 1, 0):
            lt |= eq & (a[:, i] < np.uint64(pl[i]))
            eq &= a[:, i] == np.uint64(pl[i])
        return bool(lt.all())

    def root_of_unity(self, order):
        """a primitive root of the given power-of-two order: oracle.ntt of [0, 1, 0, ...] is [w^k]"""
        e1 = np.zeros((order, 4), dtype=np.uint64)
        e1[1] = self.one
        z = self.o.ntt(self.cid, e1)[1]
        assert np.array_equal(self.pow(z, order), self.one) and np.array_equal(self.pow(z, order // 2), self.minus_one), order
        return z


_fields = {}


def _field(oracle, curve, cid):
    if cid not in _fields:
        _fields[cid] = _Field(oracle, curve, cid)
    return _fields[cid]


def _fill(F, oracle, cid, kind, seed, n):
    if kind == "random":
        return oracle.rand_fr(cid, seed, n)
    return F.full({"minus_one": F.minus_one, "top_limbs": F.top}[kind], n)


def _perm_inputs(F, oracle, cid, n, seed, kind="random"):
    """(wires (5, n, 4), id_perm, perm_idx, beta, gamma)"""
    wires = _fill(F, oracle, cid, kind, seed, 5 * n).reshape(5, n, 4)
    id_perm = _fill(F, oracle, cid, kind, seed + 1, 5 * n)
    perm_idx = np.random.RandomState(seed).permutation(5 * n).astype(np.uint64)
    ch = oracle.rand_fr(cid, seed + 2, 2)
    return wires, id_perm, perm_idx, ch[0], ch[1]


def _perm_terms(F, wires, id_perm, perm_idx, beta, gamma, n, lo, hi):
    """numerators and denominators of the gates [lo, hi) (dispatcher2.rs:333-341), vectorised; wires: five (n, 4) arrays.  Above 2^18 gates
    the range is cut into pieces computed on a few threads (the oracle's calls and numpy's gathers release the interpreter lock)."""
    if hi - lo > PIECE:
        from concurrent.futures import ThreadPoolExecutor
        cuts = list(range(lo, hi, PIECE)) + [hi]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            parts = list(ex.map(lambda c: _perm_terms(F, wires, id_perm, perm_idx, beta, gamma, n, c[0], c[1]), zip(cuts[:-1], cuts[1:])))
        return np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    num = den = None
    be, ga = F.full(beta, hi - lo), F.full(gamma, hi - lo)
    for i in range(5):
        e = slice(i * n + lo, i * n + hi)
        t = F.add(wires[i][lo:hi], ga)
        s = F.add(t, F.mul(id_perm[e], be))
        d = F.add(t, F.mul(id_perm[perm_idx[e].astype(np.intp)], be))
        num = s if num is None else F.mul(num, s)
        den = d if den is None else F.mul(den, d)
    return num, den


def _assert_product_vector(F, z, num, den):
    """z[0] = 1 and z[j+1] * den_j = z[j] * num_j with every den_j != 0 and every z[j] canonical: exactly one vector satisfies this, the
    reference's (z[j+1] = z[j] * num_j / den_j) — checked for EVERY j"""
    assert z.shape[0] == num.shape[0] + 1 == den.shape[0] + 1
    assert np.array_equal(z[0], F.one)
    assert F.canonical(z)
    assert den.any(axis=1).all()
    lhs, rhs = F.mul(z[1:], den), F.mul(z[:-1], num)
    bad = np.flatnonzero((lhs != rhs).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {lhs.shape[0]} steps of the recurrence fail, the first at gate {bad[:1]}"


def _run_perm(w, wires, id_perm, perm_idx, beta, gamma, n, first=None, count=None):
    """wires: (5, n, 4), or one (n, 4) vector used for all five wires"""
    shared = wires.ndim == 2
    dw = w.alloc(wires.size * 8).upload(wires)
    di = w.alloc(5 * n * 32).upload(id_perm)
    dp = w.alloc(5 * n * 8).upload(perm_idx)
    cnt = n if count is None else count
    out = w.alloc(cnt * 32)
    try:
        ptrs = [dw.ptr + (0 if shared else i * n * 32) for i in range(5)]
        if first is None:
            w.perm_product_dev(ptrs, di.ptr, dp.ptr, beta, gamma, n, out.ptr)
        else:
            w.perm_product_range_dev(ptrs, di.ptr, dp.ptr, beta, gamma, n, first, cnt, out.ptr)
        return out.download((cnt, 4))
    finally:
        for b in (dw, di, dp, out):
            b.free()


# ---------------------------------------------------------------------------------------------- A: the second level of each kernel
@pytest.mark.parametrize("n", [(1 << 21) + 1, (1 << 22) + 1])
def test_perm_product_with_runs_of_scan_tiles_per_top_lane(gpu_workers, oracle, n):
    """n = 2^21 + 1 gates are 1025 scan tiles: scan_top_kernel's lanes own runs of two tiles, in the prefix scan of the numerators and in
    the suffix scan of the denominators; 2^22 + 1 gates are 2049 tiles in runs of three, the smallest at which a run has a tile that is
    neither its first nor its last (the benchmark's 2^24 gates run at eight; no other exact test goes above 2^20).  One vector serves
    as all five wires; every one of the n outputs is checked, through the recurrence."""
    curve, cid = "bn254", 0
    F = _field(oracle, curve, cid)
    wire = oracle.rand_fr(cid, 811, n)
    id_perm = oracle.rand_fr(cid, 812, 5 * n)
    perm_idx = np.random.RandomState(813).permutation(5 * n).astype(np.uint64)
    beta, gamma = oracle.rand_fr(cid, 814, 2)
    z = _run_perm(gpu_workers(curve), wire, id_perm, perm_idx, beta, gamma, n)
    num, den = _perm_terms(F, [wire] * 5, id_perm, perm_idx, beta, gamma, n, 0, n - 1)
    _assert_product_vector(F, z, num, den)


@pytest.mark.parametrize("log_n", [21, 22])
def test_perm_product_range_with_runs_of_scan_tiles_per_top_lane(gpu_workers, oracle, log_n):
    """A slice of 2^21 + 2 gates starting at gate 5 of 2^21 + 8 (1025 scan tiles again; 2049 for 2^22), BLS12-381: loc[0] = 1 and the
    recurrence inside the slice."""
    curve, cid, n, j0, cnt = "bls12_381", 1, (1 << log_n) + 8, 5, (1 << log_n) + 2
    F = _field(oracle, curve, cid)
    wire = oracle.rand_fr(cid, 821, n)
    id_perm = oracle.rand_fr(cid, 822, 5 * n)
    perm_idx = np.random.RandomState(823).permutation(5 * n).astype(np.uint64)
    beta, gamma = oracle.rand_fr(cid, 824, 2)
    loc = _run_perm(gpu_workers(curve), wire, id_perm, perm_idx, beta, gamma, n, first=j0, count=cnt)
    num, den = _perm_terms(F, [wire] * 5, id_perm, perm_idx, beta, gamma, n, j0, j0 + cnt - 1)
    _assert_product_vector(F, loc, num, den)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_eval_and_div_above_the_single_trip_sizes(gpu_workers, oracle, curve, cid):
    """2^21 + 8193 coefficients: 258 evaluation tiles, so fr_sum_kernel's lanes 0 and 1 take a second partial sum; 2056 division tiles, so
    poly_div_top_kernel's lanes own three tiles each and its lane-level multipliers are powers of W^3 (two is the most any other test reaches)."""
    w = gpu_workers(curve)
    length = (1 << 21) + 8193
    F = _field(oracle, curve, cid)
    dpoly, dq = w.alloc(length * 32), w.alloc(length * 32)
    try:
        # random coefficients at a random point; then every coefficient the limb pattern p - 1 at z = 1, where W = 1 and all 1024 lanes of the
        # top kernel add up terms of one sign (its "< 16 p after the ten steps")
        for what, poly, z in (("random", oracle.rand_fr(cid, 831, length), oracle.rand_fr(cid, 832, 1)[0]), ("top_limbs at 1", F.full(F.top, length), F.one)):
            dpoly.upload(poly)
            assert np.array_equal(w.poly_eval_dev(dpoly.ptr, length, z), oracle.poly_eval(cid, poly, z)), what
            w.poly_div_linear_dev(dpoly.ptr, length, z, dq.ptr)
            got, want = dq.download((length - 1, 4)), oracle.poly_div_linear(cid, poly, z)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"{what}: {bad.size} quotient coefficients differ, the first at {bad[:1]}"
    finally:
        dpoly.free(); dq.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("i0", [(1 << 20) - 8, 1024 - 8, 0])
def test_coset_interp_across_the_seams_of_a_scaled_power_table(gpu_workers, oracle, curve, cid, i0):
    """out[t] = scale * shift^-(i0 + t) * iNTT_16(evals)[(i0 + t) mod 16] for sixteen indices that straddle 2^20 (levels 2 | 3 of the
    power table, whose level 0 carries `scale`), 1024 (levels 1 | 2), and from 0 (one level).  The power is taken by square and multiply."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    size = count = 16
    evals = oracle.rand_fr(cid, 841, size)
    shift, scale = oracle.rand_fr(cid, 842, 2)
    E = oracle.ntt(cid, evals, True, False)
    hinv = F.inv(shift)
    pw = F.mul(scale, F.pow(hinv, i0))
    want = np.empty((count, 4), dtype=np.uint64)
    for t in range(count):
        want[t] = F.mul(pw, E[(i0 + t) % size])
        pw = F.mul(pw, hinv)
    de, out = w.alloc(size * 32).upload(evals), w.alloc(count * 32)
    try:
        w.coset_interp_dev(de.ptr, size, shift, scale, i0, count, out.ptr)
        assert np.array_equal(out.download((count, 4)), want)
    finally:
        de.free(); out.free()


# ---------------------------------------------------------------------------------------------- B, C: tile seams and extreme values
# evaluation: PO_LANES = 256 lanes, EV_TILE = 8192, two tiles and one; division: len - 1 quotient coefficients at DV_TILE * k and DV_TILE * k + 1
SEAM_LENGTHS = [3, 255, 256, 257, 1026, 2049, 2050, 8191, 8192, 8193, 16385]


def _assert_eval_and_div(w, oracle, cid, dpoly, dq, poly, z, what):
    length = poly.shape[0]
    assert np.array_equal(w.poly_eval_dev(dpoly.ptr, length, z), oracle.poly_eval(cid, poly, z)), ("eval",) + what
    w.poly_div_linear_dev(dpoly.ptr, length, z, dq.ptr)
    assert np.array_equal(dq.download((length - 1, 4)), oracle.poly_div_linear(cid, poly, z)), ("div",) + what


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("length", SEAM_LENGTHS)
def test_eval_and_div_at_tile_seams_and_on_extreme_values(gpu_workers, oracle, curve, cid, length):
    """Random coefficients at a random point; every coefficient p - 1 (as a field element, and as a limb pattern) at a random point, at
    p - 1 and at 1 — the sums the comments of poly_eval_kernel and poly_div_*_kernel bound by 2.4 p and 16 p, at their largest operands."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    zr = oracle.rand_fr(cid, 851, 1)[0]
    dpoly, dq = w.alloc(length * 32), w.alloc(length * 32)
    try:
        for kind, points in (("random", [("random", zr)]),
                             ("minus_one", [("random", zr), ("minus_one", F.minus_one), ("one", F.one)]),
                             ("top_limbs", [("random", zr), ("top_limbs", F.top), ("minus_one", F.minus_one), ("one", F.one)])):
            poly = _fill(F, oracle, cid, kind, 852 + length, length)
            dpoly.upload(poly)
            for zname, z in points:
                _assert_eval_and_div(w, oracle, cid, dpoly, dq, poly, z, (length, kind, zname))
    finally:
        dpoly.free(); dq.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("kind", ["random", "minus_one", "top_limbs"])
@pytest.mark.parametrize("n", [2, 3, 2047])
def test_perm_product_at_the_smallest_sizes_and_one_short_of_a_tile(gpu_workers, oracle, curve, cid, n, kind):
    F = _field(oracle, curve, cid)
    wires, id_perm, perm_idx, beta, gamma = _perm_inputs(F, oracle, cid, n, 860 + n, kind)
    want = oracle.perm_product(cid, wires, id_perm, perm_idx, beta, gamma)
    assert np.array_equal(_run_perm(gpu_workers(curve), wires, id_perm, perm_idx, beta, gamma, n), want)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("kind", ["random", "minus_one"])
@pytest.mark.parametrize("n", [4, 4097])
def test_perm_product_range_slices_of_one_and_two_gates(gpu_workers, oracle, curve, cid, n, kind):
    """Slices of one and two gates at gate 0, in the middle and ending at gate n - 1, whose terms are stored as one; n = 4 in slices of one gate is the class prover's split among G = 4 ranks.  loc[t] = z[j0 + t] / z[j0]."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    wires, id_perm, perm_idx, beta, gamma = _perm_inputs(F, oracle, cid, n, 870 + n, kind)
    z = oracle.perm_product(cid, wires, id_perm, perm_idx, beta, gamma)
    assert z.any(axis=1).all()
    dw = w.alloc(5 * n * 32).upload(wires)
    di = w.alloc(5 * n * 32).upload(id_perm)
    dp = w.alloc(5 * n * 8).upload(perm_idx)
    out = w.alloc(2 * 32)
    try:
        starts = {1: sorted({0, 1, 2, n // 2 - 1, n // 2, n - 1}), 2: sorted({0, 1, n // 2 - 2, n // 2 - 1, n // 2, n - 2})}
        for cnt in (1, 2):
            for j0 in starts[cnt]:
                w.memset_dev(out.ptr, 0xA5, 2 * 32)
                w.perm_product_range_dev([dw.ptr + i * n * 32 for i in range(5)], di.ptr, dp.ptr, beta, gamma, n, j0, cnt, out.ptr)
                loc = out.download((cnt, 4))
                assert np.array_equal(loc[0], F.one), (j0, cnt)
                assert np.array_equal(loc, F.mul(z[j0:j0 + cnt], F.inv(z[j0]))), (j0, cnt)
    finally:
        for b in (dw, di, dp, out):
            b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_lincomb_of_32_terms_at_the_largest_sum(gpu_workers, oracle, curve, cid):
    """32 terms with every coefficient and every value p - 1 (the "< 44 p" sum of poly_lincomb_kernel at its maximum), one term, an output longer
    than every input (the tail is written as zero) and shorter than some."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    length = 300
    out = w.alloc(340 * 32)

    def check(polys, coeffs, out_len, what):
        own = {}                                                   # one device copy per distinct host array
        for q in polys:
            if id(q) not in own:
                own[id(q)] = w.alloc(max(q.shape[0], 1) * 32)
                if q.shape[0]:
                    own[id(q)].upload(q)
        bufs = [own[id(q)] for q in polys]
        try:
            w.memset_dev(out.ptr, 0xA5, 340 * 32)
            w.poly_lincomb_dev([(b.ptr, q.shape[0]) for b, q in zip(bufs, polys)], coeffs, out.ptr, out_len)
            ref = oracle.poly_lincomb(cid, polys, coeffs)
            want = np.zeros((out_len, 4), dtype=np.uint64)
            m = min(out_len, ref.shape[0])
            want[:m] = ref[:m]
            got = out.download((340, 4))
            assert np.array_equal(got[:out_len], want), what
            assert (got[out_len:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), what + ("wrote past out_len",)
        finally:
            for b in own.values():
                b.free()

    for name, v in (("minus_one", F.minus_one), ("top_limbs", F.top)):
        for k in (32, 1):
            for out_len in (length, length + 33, 257, 256, 1):
                check([F.full(v, length)] * k, F.full(v, k), out_len, (name, k, out_len))
    # ragged random terms, the output longer than some inputs and shorter than others
    lens = [300, 10, 257, 256, 1, 0, 299]
    polys = [oracle.rand_fr(cid, 880 + i, max(L, 1))[:L] for i, L in enumerate(lens)]
    coeffs = oracle.rand_fr(cid, 879, len(lens))
    coeffs[2] = F.minus_one
    for out_len in (260, 340, 5):
        check(polys, coeffs, out_len, ("ragged", out_len))
    out.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_perm_product_of_extreme_values(gpu_workers, oracle, curve, cid):
    """Every wire and every id_perm value p - 1 with (beta, gamma) in {(p-1, p-1), (1, p-1), (p-1, 1)}: each factor w + gamma + beta * id is
    -1, -3 or 1, so nothing divides by zero; and the same with p - 1 read as a limb pattern."""
    F = _field(oracle, curve, cid)
    n = 5000
    perm_idx = np.random.RandomState(890).permutation(5 * n).astype(np.uint64)
    for name, v, challenges in (("minus_one", F.minus_one, [(F.minus_one, F.minus_one), (F.one, F.minus_one), (F.minus_one, F.one)]),
                                ("top_limbs", F.top, [(F.top, F.top), (F.one, F.top), (F.top, F.one)])):
        wires, id_perm = F.full(v, 5 * n).reshape(5, n, 4), F.full(v, 5 * n)
        for k, (beta, gamma) in enumerate(challenges):
            want = oracle.perm_product(cid, wires, id_perm, perm_idx, beta, gamma)          # raises on a zero denominator
            got = _run_perm(gpu_workers(curve), wires, id_perm, perm_idx, beta, gamma, n)
            assert np.array_equal(got, want), (name, k)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_blinders_of_p_minus_one_wrap_both_ways(gpu_workers, oracle, curve, cid):
    """0 - (p - 1) and (p - 1) + (p - 1): the subtraction borrows and the addition carries past p on every blinded coefficient"""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    n = 8
    for k in (2, 3):
        for name, v in (("minus_one", F.minus_one), ("top_limbs", F.top)):
            base = F.full(v, n + k)
            base[:k] = 0
            bl = F.full(v, k)
            d = w.alloc((n + k) * 32).upload(base)
            w.blind_dev(d.ptr, n, bl)
            got = d.download((n + k, 4))
            d.free()
            assert np.array_equal(got, oracle.blind(cid, base, n, bl)), (k, name)
            assert np.array_equal(got[:k], F.sub(F.zero, bl)) and np.array_equal(got[n:], F.add(bl, bl)) and np.array_equal(got[k:n], base[k:n])


# ---------------------------------------------------------------------------------------------- D: structured points
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("order", [2, 8, 128, 1024, 2048])
def test_eval_and_div_at_roots_of_unity(gpu_workers, oracle, curve, cid, order):
    """z of order 2, 8 (z^DV_CH = 1: both lane tables of the division are all ones), 128 (z^DV_LANES = 1), 1024 (z^DV_TILE = 1: W = 1 in
    poly_div_top_kernel, and levels 1 and 2 of the power table are all ones) and 2048 (W = -1)."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    length = 5000
    poly = oracle.rand_fr(cid, 900 + cid, length)
    z = F.root_of_unity(order)
    dpoly, dq = w.alloc(length * 32).upload(poly), w.alloc(length * 32)
    try:
        _assert_eval_and_div(w, oracle, cid, dpoly, dq, poly, z, (order,))
    finally:
        dpoly.free(); dq.free()


# ---------------------------------------------------------------------------------------------- E: a zero numerator is not an error
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("j", [0, 2100, 4998])
def test_perm_product_with_a_vanishing_numerator(gpu_workers, oracle, curve, cid, j):
    """id_perm[i * n + j] = -(w[i][j] + gamma) / beta makes num_j = 0 and, as the permutation moves that slot, no denominator: the reference
    carries on with z[j + 1:] = 0 and so must the device (PLONK_OK; only a zero DENOMINATOR is an error)."""
    F = _field(oracle, curve, cid)
    n = 5000
    wires, id_perm, perm_idx, beta, gamma = _perm_inputs(F, oracle, cid, n, 910)
    i = next(i for i in range(5) if int(perm_idx[i * n + j]) != i * n + j)
    id_perm[i * n + j] = F.mul(F.sub(F.zero, F.add(wires[i, j], gamma)), F.inv(beta))
    want = oracle.perm_product(cid, wires, id_perm, perm_idx, beta, gamma)                # no ZeroDivisionError
    got = _run_perm(gpu_workers(curve), wires, id_perm, perm_idx, beta, gamma, n)         # no PlonkError
    assert np.array_equal(got, want)
    assert not got[j + 1:].any() and got[:j + 1].any(axis=1).all()


# ---------------------------------------------------------------------------------------------- F: class interleave on its own
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_class_interleave_alone(gpu_workers, oracle, curve, cid, G):
    """out[t * G + s] = scale * in[s * stride + ((L - t) mod L if reverse else t)] for L = 1, 255 and 257 values per class (one lane, a
    workgroup less one, a workgroup and one), packed and padded class strides, no scale, one and p - 1."""
    w = gpu_workers(curve)
    F = _field(oracle, curve, cid)
    for L in (1, 255, 257):
        for stride in (L, L + 3):
            src = oracle.rand_fr(cid, 920 + G + L, G * stride)
            src[0], src[G * stride - 1] = F.top, F.top
            d_in, d_out = w.alloc(G * stride * 32).upload(src), w.alloc((G * L + 1) * 32)
            try:
                for reverse in (False, True):
                    t = np.arange(L)
                    col = (L - t) % L if reverse else t
                    plain = src.reshape(G, stride, 4)[:, col].transpose(1, 0, 2).reshape(G * L, 4)          # [t * G + s]
                    for name, scale in (("none", None), ("one", F.one), ("minus_one", F.minus_one), ("top_limbs", F.top)):
                        want = plain if scale is None else F.mul(plain, scale)
                        w.memset_dev(d_out.ptr, 0xA5, (G * L + 1) * 32)
                        w.class_interleave_dev(d_in.ptr, G, L, reverse, scale, d_out.ptr, in_stride=stride)
                        got = d_out.download((G * L + 1, 4))
                        assert np.array_equal(got[:G * L], want), (L, stride, reverse, name)
                        assert (got[G * L] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), (L, stride, reverse, name, "wrote past the output")
                        if stride == L:                                                                       # in_stride 0 means packed
                            w.class_interleave_dev(d_in.ptr, G, L, reverse, scale, d_out.ptr)
                            assert np.array_equal(d_out.download((G * L, 4)), want), (L, "stride 0", reverse, name)
            finally:
                d_in.free(); d_out.free()
