"""The folded first pass of coset transforms (csrc/ntt_kernels.hpp: the CTW instantiation of ntt_pass_kernel), bit for bit against the oracle.

The first pass of a class transform (plonk_coset_eval_dev) and of the whole-vector forward coset transform used to multiply every element by
a row-table entry s^a at load; with option ntt_coset_twiddles = 1 (the default) the scale sits in the butterfly twiddles of that pass — a
per-class table of prepared constants s^(R / 2^(sigma+1)) * w_(2^(sigma+1))^j — wherever the pass has the production shape: width >= 5, two or
more passes, prepared-constant butterflies, swizzled 8-column tiles.  Single-pass class transforms, widths below 5, ntt_shoup = 0 and
ntt_coset_twiddles = 0 keep the row table.

Every case asserts the ROUTE before it compares values: a folded launch is bracketed by the profiling scope "ntt_pass_coset_tw", so its launch
count says how many passes of a call were folded (1 per transform that has a folded first pass, 0 otherwise).

Mutations tried on a scratch copy under the host emulation (tests/hostemu), each failing these cases BY VALUE with the count still right:
the stage offset 2^sigma - 1 off by one (2^sigma), and s^(R / 2^sigma) in place of s^(R / 2^(sigma+1)) in the table."""
import contextlib

import numpy as np
import pytest

from ntt_plans import plan_widths
from test_gpu_coset_classes import _consts, _folded

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
SCOPE = "ntt_pass_coset_tw"
OPTIONS = {"ntt_max_log_r": 9, "ntt_shoup": 1, "ntt_coset_twiddles": 1, "ntt_plane_budget": -1}


@contextlib.contextmanager
def forced(w, **options):
    """The worker trimmed (nothing cached), the options set, profiling on; the defaults back afterwards."""
    try:
        w.trim()
        for key, value in options.items():
            w.set_option(key, value)
        w.profile_enable(True)
        w.profile_reset()
        yield
    finally:
        w.profile_enable(False)
        w.profile_reset()
        for key, value in OPTIONS.items():
            w.set_option(key, value)
        w.trim()


def folded_launches(w, call):
    """call() -> (its result, the folded pass launches it caused)"""
    w.profile_reset()
    out = call()
    return out, int(w.profile_get(SCOPE)[1])


def classes_of(log_size, length):
    """coset_eval_run's class count (csrc/poly_ops.hip), as a power of two"""
    k = 0
    while k < 4 and log_size - k > 1 and 2 * length < 3 * ((1 << log_size) >> (k + 1)):
        k += 1
    return k


_WANT = {}


def want_eval(oracle, cid, log_size, length, mult=1):
    """(coefficients, evaluations on mult * g * <w_size>): the oracle's coset FFT of the zero-padded / folded vector, once per case.  A shift
    other than g is the coset FFT of the coefficients scaled by mult^i."""
    key = (cid, log_size, length, mult)
    if key not in _WANT:
        size = 1 << log_size
        P, f, g, _ = _consts(oracle, cid, log_size)
        poly = oracle.rand_fr(cid, 8800 + 31 * log_size + length % 1009, length)
        ref = poly
        if mult != 1:
            ref = np.stack([P.fr_to_limbs(f, P.fr_from_limbs(f, x) * pow(mult, i, f.p) % f.p) for i, x in enumerate(poly)])
        want = oracle.ntt(cid, _folded(P, f, g, ref, size), False, True, threads=8)
        poly.setflags(write=False)
        want.setflags(write=False)
        _WANT[key] = (poly, want, P.fr_to_limbs(f, g * mult % f.p))
    return _WANT[key]


def check_eval(w, oracle, curve, cid, log_size, length, count, mult=1, where=""):
    poly, want, shift = want_eval(oracle, cid, log_size, length, mult)
    size = 1 << log_size
    dp, out = w.alloc(length * 32).upload(poly), w.alloc(size * 32)
    try:
        _, got_count = folded_launches(w, lambda: w.coset_eval_dev(dp.ptr, length, size, shift, out.ptr))
        where = f"{curve} coset_eval 2^{log_size} <- {length} ({1 << classes_of(log_size, length)} classes) {where}"
        assert got_count == count, f"{where}: {got_count} folded launches, expected {count}"
        assert np.array_equal(out.download((size, 4)), want), where
        assert np.array_equal(dp.download((length, 4)), poly), where + " (input modified)"
    finally:
        dp.free(); out.free()


# ---------------------------------------------------------------------------------------------- first-pass widths
# (ntt_max_log_r, log class size, log classes): w + w for every folded width at its smallest size, 5 + 5 + 5, and the flagship's first-pass
# shape (8 classes of 8 + 8) at 2^19 points
WIDTHS = [(5, 10, 1), (6, 12, 1), (7, 14, 1), (8, 16, 1), (9, 18, 0), (5, 15, 0), (8, 16, 3)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_m,log_b", WIDTHS, ids=["+".join(map(str, plan_widths(m, r))) + f"x{1 << b}" for r, m, b in WIDTHS])
def test_every_folded_first_pass_width(gpu_workers, oracle, curve, cid, max_log_r, log_m, log_b):
    w = gpu_workers(curve)
    widths = plan_widths(log_m, max_log_r)
    assert len(widths) >= 2 and widths[0] >= 5
    length = (1 << log_m) + 3
    assert classes_of(log_m + log_b, length) == log_b
    with forced(w, ntt_max_log_r=max_log_r):
        check_eval(w, oracle, curve, cid, log_m + log_b, length, 1, where="plan " + "+".join(map(str, widths)))


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_b", [0, 1, 2, 3])
def test_class_counts(gpu_workers, oracle, curve, cid, log_b):
    """1, 2, 4, 8 classes of 2^10 points (5 + 5): the table base is the workgroup's class"""
    w = gpu_workers(curve)
    with forced(w):
        assert classes_of(10 + log_b, 1 << 10) == log_b
        check_eval(w, oracle, curve, cid, 10 + log_b, 1 << 10, 1)


# (log size, length) on classes of M = 2^10 points: 1 and a length far below M (16 classes, nearly every row zero), M - 1, M, the fold path with
# M + 2 and M + 3 (nfold = 2), and 8M (NTT_MAX_FOLD) on one class
LENGTHS = [(14, 1), (14, 37), (11, 1023), (11, 1024), (11, 1026), (11, 1027), (10, 8192)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_size,length", LENGTHS)
def test_lengths_zero_rows_and_folds(gpu_workers, oracle, curve, cid, log_size, length):
    w = gpu_workers(curve)
    assert log_size - classes_of(log_size, length) == 10
    with forced(w):
        check_eval(w, oracle, curve, cid, log_size, length, 1)


# ---------------------------------------------------------------------------------------------- the routes that keep the row table
@pytest.mark.parametrize("curve,cid", CURVES)
def test_narrow_and_single_pass_classes_keep_the_row_table(gpu_workers, oracle, curve, cid):
    """Single-pass class transforms (widths 1 ... 4 and 9: the first pass is the last, its tile columns are the classes) and first passes
    narrower than 5 in multi-pass plans (3 + 3, 4 + 4, 4 + 4 + 4) are not folded: count 0, values exact."""
    w = gpu_workers(curve)
    with forced(w):
        for log_m in (1, 2, 3, 4, 9):
            check_eval(w, oracle, curve, cid, log_m, 1 << log_m, 0, where="single pass")
        check_eval(w, oracle, curve, cid, 12, (1 << 9) + 3, 0, where="8 single-pass classes")
    for max_log_r, log_size, length in [(3, 6, 64), (4, 8, 256), (4, 13, (1 << 12) + 3)]:
        with forced(w, ntt_max_log_r=max_log_r):
            check_eval(w, oracle, curve, cid, log_size, length, 0, where="plan " + "+".join(map(str, plan_widths(log_size - classes_of(log_size, length), max_log_r))))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_options_select_the_route_not_the_result(gpu_workers, oracle, curve, cid):
    """ntt_coset_twiddles = 0 and ntt_shoup = 0 each run the row-table first pass (count 0); the bytes are those of the folded route"""
    w = gpu_workers(curve)
    for log_size, length in [(11, 1027), (19, (1 << 16) + 3)]:
        with forced(w):
            check_eval(w, oracle, curve, cid, log_size, length, 1, where="default")
        with forced(w, ntt_coset_twiddles=0):
            check_eval(w, oracle, curve, cid, log_size, length, 0, where="ntt_coset_twiddles=0")
        with forced(w, ntt_shoup=0):
            check_eval(w, oracle, curve, cid, log_size, length, 0, where="ntt_shoup=0")
    with forced(w):                                   # toggled on a cached shift set: the set holds both tables
        check_eval(w, oracle, curve, cid, 11, 1027, 1)
        w.set_option("ntt_coset_twiddles", 0)
        check_eval(w, oracle, curve, cid, 11, 1027, 0)
        w.set_option("ntt_coset_twiddles", 1)
        check_eval(w, oracle, curve, cid, 11, 1027, 1)


# ---------------------------------------------------------------------------------------------- whole-vector transforms
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_n", [10, 16], ids=["5+5", "8+8"])
def test_whole_vector_forward_coset_transform_is_folded(gpu_workers, oracle, curve, cid, log_n):
    """plonk_ntt forward on the coset g * <w>: the g^(a * r_1) half of the shift is the folded pass's table (one per (r_1, width), cached with the
    row tables), the g^b half stays in the plane.  The inverse coset transform and the plain transforms have no row scale: count 0."""
    w = gpu_workers(curve)
    assert plan_widths(log_n, 9) == [log_n // 2] * 2
    v = oracle.rand_fr(cid, 8900 + log_n, 1 << log_n)
    with forced(w):
        for rep in range(2):                          # the second call finds the table cached
            got, count = folded_launches(w, lambda: w.ntt(v, False, True))
            assert count == 1, (curve, log_n, rep, count)
            assert np.array_equal(got, oracle.ntt(cid, v, False, True, threads=8)), (curve, log_n, rep)
        for inv, coset in [(True, True), (False, False), (True, False)]:
            got, count = folded_launches(w, lambda: w.ntt(v, inv, coset))
            assert count == 0, (curve, log_n, inv, coset, count)
            assert np.array_equal(got, oracle.ntt(cid, v, inv, coset, threads=8)), (curve, log_n, inv, coset)
        w.set_option("ntt_coset_twiddles", 0)
        got, count = folded_launches(w, lambda: w.ntt(v, False, True))
        assert count == 0 and np.array_equal(got, oracle.ntt(cid, v, False, True, threads=8)), (curve, log_n, "ntt_coset_twiddles=0")


# ---------------------------------------------------------------------------------------------- table lifetime
@pytest.mark.parametrize("curve,cid", CURVES)
def test_shift_sets_cached_evicted_and_trimmed(gpu_workers, oracle, curve, cid):
    """Two shifts of one size, alternating: both sets cached under the default budget, each evicting the other when the budget holds one set's
    planes; then plonk_trim, then again.  The coset twiddle tables live and die with their shift set: every evaluation folded and exact."""
    w = gpu_workers(curve)
    log_size, length = 12, 1027                       # 4 classes of 2^10 points, nfold = 2
    one_set = (1 << log_size) * 32
    for budget in (-1, one_set):
        with forced(w, ntt_plane_budget=budget):
            for rnd in range(2):
                for mult in (1, 3, 1, 3):
                    check_eval(w, oracle, curve, cid, log_size, length, 1, mult=mult, where=f"budget {budget} round {rnd} shift g*{mult}")
                w.trim()
