"""One polynomial opened at many device-resident points (plonk_poly_open_many_dev, csrc/kzg_kernels.hpp) and `kzg.open_many` on top of it:
values and quotient rows bit for bit against the integer reference of tests/kzg_ref.py, proofs against the trapdoor expression.

T is the coefficient tile of the kernels and TOP the lane count of the per-point top scan, both read from the library (`kzg.tile()`,
`kzg.top_lanes()`), so the lengths below follow a change of shape.  Lengths are named, not numbers, because they are resolved when a test
runs: Tm1 = T - 1, 2Tp1 = 2 T + 1, ...  Every call of the sweep holds M points (1, 2, 5) taken as windows of one list that has 0, 1, p - 1,
a primitive root of unity of the smallest order 2^k >= len, a repeated point and random ones; the windows of 5 put 0 next to random points."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import kzg
from distributed_plonk_amd._ffi import PlonkError
from tests import kzg_ref as R
from tests.kzg_ref import CURVES

pytestmark = pytest.mark.gpu

LENS = {"len0": lambda T: 0, "len1": lambda T: 1, "len2": lambda T: 2, "len3": lambda T: 3, "Tm1": lambda T: T - 1, "T": lambda T: T,
        "Tp1": lambda T: T + 1, "Tp2": lambda T: T + 2, "2Tp1": lambda T: 2 * T + 1, "5Tp7": lambda T: 5 * T + 7}
PATTERN = 0xA5
_SRS, _POLY = {}, {}


def srs_worker(gpu_workers, curve):
    """The curve's worker with the trapdoor SRS of 5 T + 7 points resident (made once; installed again whenever another key took its place)."""
    w = gpu_workers(curve)
    n = 5 * kzg.tile() + 7
    if curve not in _SRS:
        d = w.alloc(n * 2 * w.q64 * 8)
        w.synth_srs(R.to_limbs(curve, R.TAU), n, d.ptr)
        w.sync()
        _SRS[curve] = d
    w.init_dev(_SRS[curve].ptr, n, 0, 0)
    return w


def poly(curve, length):
    """(residues, limbs) of the test polynomial of that length: a prefix of one random vector per curve, the last coefficient non-zero."""
    if curve not in _POLY:
        rng = random.Random(0x4b5a47 + len(curve))
        _POLY[curve] = [rng.randrange(1, R.FR[curve]) for _ in range(5 * kzg.tile() + 7)]
    c = _POLY[curve][:length]
    return c, R.vec_to_limbs(curve, c)


def point_list(curve, length, seed):
    p = R.FR[curve]
    rng = random.Random(seed)
    k = 1
    while k < max(length, 2):
        k <<= 1
    r1 = rng.randrange(2, p - 1)
    return [0, 1, p - 1, R.root_of_unity(curve, k), r1, rng.randrange(2, p - 1), r1, rng.randrange(2, p - 1)]


def windows(n, M):
    """index windows of M consecutive entries covering range(n), the last one flush with the end"""
    return [list(range(min(lo, n - M), min(lo, n - M) + M)) for lo in range(0, n, M)]


def run_open(w, d_poly, length, pts_limbs, q_stride, quotients=True):
    """plonk_poly_open_many_dev on pre-filled outputs -> (values [M, 4], rows [M, q_stride, 4] or None, status [M])."""
    M = pts_limbs.shape[0]
    with w.scope() as s:
        d_pts = s.upload(pts_limbs)
        d_val, d_st = s.alloc(M * 32), s.alloc(M * 4)
        nq = max(M * q_stride, 1)
        d_q = s.alloc(nq * 32)
        for d, nbytes in ((d_val, M * 32), (d_st, M * 4), (d_q, nq * 32)):
            w.memset_dev(d.ptr, PATTERN, nbytes)
        w.poly_open_many_dev(d_poly, length, d_pts.ptr, M, d_val.ptr, d_q.ptr if quotients else 0, q_stride, d_st.ptr)
        return d_val.download((M, 4)), d_q.download((M, q_stride, 4)) if quotients else None, d_st.download((M,), dtype=np.uint32)


def check_rows(curve, length, rows, want_rows):
    """rows [M, q_stride, 4]: the first len - 1 words of row j are want_rows[j], the rest is the pattern it was filled with"""
    filled = np.frombuffer(bytes([PATTERN]) * 8, dtype=np.uint64)[0]
    n = max(length - 1, 0)
    for j, want in enumerate(want_rows):
        assert np.array_equal(rows[j, :n], R.vec_to_limbs(curve, want)), j
    assert (rows[:, n:] == filled).all()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("name", list(LENS))
def test_values_and_quotient_rows_match_the_reference(gpu_workers, curve, cid, name):
    w = gpu_workers(curve)
    length = LENS[name](kzg.tile())
    coeffs, limbs = poly(curve, length)
    zs = point_list(curve, length, 100 + length)
    ref = [R.synth_div(curve, coeffs, z) for z in zs]
    assert all(y == R.horner(curve, coeffs, z) for (q, y), z in zip(ref, zs))
    with w.scope() as s:
        d_poly = s.upload(limbs).ptr if length else 0
        for M in (1, 2, 5):
            for q_stride in (max(length - 1, 0), length + 5):
                for idx in windows(len(zs), M):
                    vals, rows, st = run_open(w, d_poly, length, R.vec_to_limbs(curve, [zs[i] for i in idx]), q_stride)
                    assert not st.any(), (M, q_stride, idx)
                    assert np.array_equal(vals, R.vec_to_limbs(curve, [ref[i][1] for i in idx])), (M, q_stride, idx)
                    check_rows(curve, length, rows, [ref[i][0] for i in idx])


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("M", [63, 64, 65])
def test_point_counts_across_the_table_kernels_workgroup_seam(gpu_workers, curve, cid, M):
    w = gpu_workers(curve)
    length = kzg.tile() + 1
    coeffs, limbs = poly(curve, length)
    rng = random.Random(M)
    zs = [0, 1, R.FR[curve] - 1] + [rng.randrange(R.FR[curve]) for _ in range(M - 3)]
    rng.shuffle(zs)
    with w.scope() as s:
        vals, rows, st = run_open(w, s.upload(limbs).ptr, length, R.vec_to_limbs(curve, zs), length - 1)
    ref = [R.synth_div(curve, coeffs, z) for z in zs]
    assert not st.any()
    assert np.array_equal(vals, R.vec_to_limbs(curve, [y for _, y in ref]))
    check_rows(curve, length, rows, [q for q, _ in ref])


def test_top_stage_scan_with_two_tiles_per_lane(gpu_workers, oracle):
    """Every stage with more than one unit of work: the top kernel gives lane l the tiles [l per, (l + 1) per) with per = ceil(nt / TOP), so
    per = 2 needs nt = ceil((len - 1) / T) > TOP, i.e. len > TOP T + 1.  len = TOP T + 3 is nt = TOP + 1: lanes that scan two tiles, lanes
    with none, and a last tile of two coefficients.  Against the oracle's C poly_eval and poly_div_linear."""
    curve, cid = "bn254", 0
    w = gpu_workers(curve)
    T, TOP = kzg.tile(), kzg.top_lanes()
    length = TOP * T + 3
    assert (length - 1 + T - 1) // T == TOP + 1
    limbs = oracle.rand_fr(cid, 77, length)
    zs = np.concatenate([R.to_limbs(curve, 0)[None, :], oracle.rand_fr(cid, 78, 2)])
    with w.scope() as s:
        vals, rows, st = run_open(w, s.upload(limbs).ptr, length, zs, length - 1)
    assert not st.any()
    for j in range(3):
        assert np.array_equal(vals[j], oracle.poly_eval(cid, limbs, zs[j])), j
        assert np.array_equal(rows[j], oracle.poly_div_linear(cid, limbs, zs[j])), j


@pytest.mark.parametrize("curve,cid", CURVES)
def test_values_only_mode_equals_the_full_mode(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    length = kzg.tile() + 2
    coeffs, limbs = poly(curve, length)
    zs = R.vec_to_limbs(curve, point_list(curve, length, 5)[:5])
    with w.scope() as s:
        d = s.upload(limbs).ptr
        full, _, _ = run_open(w, d, length, zs, length - 1)
        only, _, st = run_open(w, d, length, zs, 0, quotients=False)
    assert not st.any() and np.array_equal(full, only)
    assert np.array_equal(only, kzg.evaluate(w, limbs, zs))
    assert np.array_equal(only, R.vec_to_limbs(curve, [R.horner(curve, coeffs, R.from_limbs(curve, z)) for z in zs]))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_bad_arguments(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    p = R.FR[curve]
    length = kzg.tile() + 2
    coeffs, limbs = poly(curve, length)
    zs = [3, 0, 5, 7]
    pts = R.vec_to_limbs(curve, zs)
    pts[1] = R.plain_limbs(p)                              # the modulus itself
    pts[3] = np.full(4, 2 ** 64 - 1, dtype=np.uint64)
    with w.scope() as s:
        d = s.upload(limbs)
        vals, rows, st = run_open(w, d.ptr, length, pts, length + 5)
        assert [int(x) for x in st] == [0, 8, 0, 8]
        ref = [R.synth_div(curve, coeffs, z) for z in zs]
        zero = [0] * (length - 1)
        assert np.array_equal(vals, R.vec_to_limbs(curve, [ref[0][1], 0, ref[2][1], 0]))
        check_rows(curve, length, rows, [ref[0][0], zero, ref[2][0], zero])
        only, _, st = run_open(w, d.ptr, length, pts, 0, quotients=False)
        assert [int(x) for x in st] == [0, 8, 0, 8] and np.array_equal(only, vals)
        # an output that overlaps the polynomial
        d_pts, d_val, d_st, d_q = s.upload(pts), s.alloc(4 * 32), s.alloc(4 * 4), s.alloc(4 * length * 32)
        for args in ((d.ptr, d_q.ptr, d_st.ptr), (d_val.ptr, d.ptr + 32 * (length - 1), d_st.ptr), (d_val.ptr, d_q.ptr, d.ptr + 64)):
            with pytest.raises(PlonkError) as e:
                w.poly_open_many_dev(d.ptr, length, d_pts.ptr, 4, args[0], args[1], length - 1, args[2])
            assert e.value.code == -1
        with pytest.raises(PlonkError) as e:
            w.poly_open_many_dev(d.ptr, length, d_pts.ptr, 4, d_val.ptr, d_q.ptr, length - 2, d_st.ptr)       # rows would overlap
        assert e.value.code == -1
        w.poly_open_many_dev(d.ptr, length, d_pts.ptr, 0, 0, 0, 0, 0)                                         # no points: nothing happens
    with pytest.raises(ValueError):
        kzg.open_many(w, limbs, pts)
    with pytest.raises(ValueError):
        kzg.evaluate(w, limbs, pts)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_reference_points_are_the_oracles_commitments(gpu_workers, oracle, curve, cid):
    """The trapdoor expressions of tests/kzg_ref.py pinned against oracle.commit_polynomial on the SRS itself."""
    w = srs_worker(gpu_workers, curve)
    n = 40
    srs = _SRS[curve].download((n, 2 * w.q64))
    assert np.array_equal(srs[1], R.g_times(curve, cid, R.TAU)[0])
    coeffs, limbs = poly(curve, n)
    z = 12345
    q, y = R.synth_div(curve, coeffs, z)
    for c, want in ((coeffs, R.commitment(curve, cid, coeffs)), (q, R.proof(curve, cid, coeffs, z))):
        got = oracle.jac_to_affine(cid, oracle.commit_polynomial(cid, srs, R.vec_to_limbs(curve, c)))
        assert got[1] == want[1] and np.array_equal(got[0], want[0])
    assert R.holds(curve, cid, R.commitment(curve, cid, coeffs), R.proof(curve, cid, coeffs, z), z, y)
    assert not R.holds(curve, cid, R.commitment(curve, cid, coeffs), R.proof(curve, cid, coeffs, z), z, y + 1)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_open_many_proofs_are_the_trapdoor_expression(gpu_workers, curve, cid):
    w = srs_worker(gpu_workers, curve)
    T = kzg.tile()
    for length in (T + 2, 1, 0):                          # a constant and the zero polynomial: pi = infinity
        coeffs, limbs = poly(curve, length)
        zs = point_list(curve, length, 9)[:5]
        pts = R.vec_to_limbs(curve, zs)
        ops = kzg.open_many(w, limbs, pts)
        assert len(ops) == 5
        for z, op in zip(zs, ops):
            assert np.array_equal(op.point, R.to_limbs(curve, z))
            assert np.array_equal(op.value, R.to_limbs(curve, R.horner(curve, coeffs, z)))
            assert np.array_equal(op.proof_xy, R.xy_of(R.proof(curve, cid, coeffs, z))), (length, z)
            assert length > 1 or not op.proof_xy.any()
        if length > 1:                                     # chunks of 2, 2 and 1; and from a polynomial already on the device
            row_bytes = (length - 1) * 32
            with w.scope() as s:
                for src in (limbs, (s.upload(limbs), length), (s.upload(limbs).ptr, length)):
                    again = kzg.open_many(w, src, pts, max_scratch_bytes=2 * row_bytes + row_bytes // 2)
                    assert all(np.array_equal(a.point, b.point) and np.array_equal(a.value, b.value) and np.array_equal(a.proof_xy, b.proof_xy)
                               for a, b in zip(ops, again)) and len(again) == 5
            one = kzg.open_many(w, limbs, pts, max_scratch_bytes=1)          # at least one point per chunk
            assert all(np.array_equal(a.proof_xy, b.proof_xy) for a, b in zip(ops, one))
            comm = kzg.commit(w, limbs)
            want = R.commitment(curve, cid, coeffs)
            assert comm[1] == want[1] and np.array_equal(comm[0], want[0])
    assert kzg.open_many(w, limbs, np.zeros((0, 4), np.uint64)) == []


@pytest.mark.parametrize("curve,cid", CURVES)
def test_open_many_needs_a_key_as_long_as_the_quotient(gpu_workers, curve, cid):
    w = srs_worker(gpu_workers, curve)
    calls = []
    real = w.poly_open_many_dev
    w.poly_open_many_dev = lambda *a: calls.append(a) or real(*a)
    try:
        n = w.n_bases
        limbs = np.tile(R.to_limbs(curve, 1), (n + 2, 1))
        with pytest.raises(ValueError):
            kzg.open_many(w, limbs, R.vec_to_limbs(curve, [3]))
        assert not calls
        assert len(kzg.open_many(w, limbs[:n + 1], R.vec_to_limbs(curve, [3]))) == 1 and len(calls) == 1
    finally:
        del w.poly_open_many_dev


@pytest.mark.parametrize("curve,cid", CURVES)
def test_open_many_agrees_with_the_single_point_entry_points(gpu_workers, curve, cid):
    """A second witness, not the reference: poly_eval_dev, poly_div_linear_dev and commit_dev at one point."""
    w = srs_worker(gpu_workers, curve)
    length = 2 * kzg.tile() + 1
    _, limbs = poly(curve, length)
    z = R.to_limbs(curve, 0xC0FFEE)
    op = kzg.open_many(w, limbs, z[None, :])[0]
    with w.scope() as s:
        d, d_q = s.upload(limbs), s.alloc((length - 1) * 32)
        assert np.array_equal(op.value, w.poly_eval_dev(d.ptr, length, z))
        w.poly_div_linear_dev(d.ptr, length, z, d_q.ptr)
        xy, inf = w.g1_to_affine(w.commit_dev(d_q.ptr, length - 1))
    assert not inf and np.array_equal(op.proof_xy, np.asarray(xy).reshape(-1))
