"""Whole-vector NTT (plonk_ntt / plonk_ntt_dev) vs the oracle: bit-exact Montgomery limbs.

Mirrors the shape of the reference's tests: 4 modes x several domain sizes incl. odd log N
(dispatcher.rs:246-350 uses 2^11 and 2^13; playground.rs:82-103 uses 512 plus the zero-padding and
round-trip identities)."""
import numpy as np
import pytest

from ntt_plans import FORCED_PLANS, plan_str, plan_widths

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]
CURVES = [("bn254", 0), ("bls12_381", 1)]


_WANT = {}


def oracle_ntt(oracle, cid, v, seed, log_n, inv, coset):
    """oracle.ntt of the seeded input `v`, computed once per (curve, seed, size, mode) and shared by the forced-plan cases of up to 2^16
    points (the same vector runs under several plans); never modified."""
    if log_n > 16:
        return oracle.ntt(cid, v, inv, coset, threads=8)
    key = (cid, seed, log_n, inv, coset)
    if key not in _WANT:
        _WANT[key] = oracle.ntt(cid, v, inv, coset, threads=8)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def extreme_inputs(oracle, cid, log_n):
    """all p - 1, alternating 0 / p - 1, a single p - 1 among zeros, half p - 1 and half random"""
    n = 1 << log_n
    pm1 = oracle.field_const(cid, 0, 0) - np.array([1, 0, 0, 0], dtype=np.uint64)       # p - 1: self-inverse under the Montgomery map up to sign, any fixed residue will do
    rnd = oracle.rand_fr(cid, 4242 + log_n, n)
    cases = []
    a = np.tile(pm1, (n, 1)); cases.append(a)
    b = np.zeros((n, 4), dtype=np.uint64); b[::2] = pm1; cases.append(b)
    c = np.zeros((n, 4), dtype=np.uint64); c[n - 1] = pm1; cases.append(c)
    d = rnd.copy(); d[: n // 2] = pm1; cases.append(d)
    return cases


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5, 9, 10, 11, 13, 16])
def test_ntt_matches_oracle(gpu_workers, oracle, curve, cid, log_n):
    w = gpu_workers(curve)
    v = oracle.rand_fr(cid, 1000 + log_n, 1 << log_n)
    for inv, coset in MODES:
        got = w.ntt(v, inv, coset)
        want = oracle.ntt(cid, v, inv, coset, threads=4)
        assert np.array_equal(got, want), f"{curve} 2^{log_n} inv={inv} coset={coset}"


@pytest.mark.parametrize("curve,cid", [("bn254", 0), ("bls12_381", 1)])
@pytest.mark.parametrize("log_n", [9, 10, 18])
def test_ntt_extreme_inputs_and_both_butterfly_forms(gpu_workers, oracle, curve, cid, log_n):
    """The lazy bounds of the pass kernel at their top (ntt_kernels.hpp: values grow 4p per stage to < 36p with the precomputed-
    quotient butterflies, which BLS12-381's Fr uses since round 4): inputs of all p - 1, alternating 0 / p - 1 and a single p - 1 among zeros,
    through a full 2^9-row pass (log_n = 9), a two-pass plan (10) and two full passes (18), every mode, with the Shoup butterflies (the
    default) and with the Montgomery ones (option ntt_shoup = 0) — bit-exact against the oracle both ways."""
    w = gpu_workers(curve)
    cases = extreme_inputs(oracle, cid, log_n)
    try:
        for shoup in (1, 0):
            w.set_option("ntt_shoup", shoup)
            for v in cases:
                for inv, coset in MODES:
                    assert np.array_equal(w.ntt(v, inv, coset), oracle.ntt(cid, v, inv, coset, threads=8)), (curve, log_n, shoup, inv, coset)
    finally:
        w.set_option("ntt_shoup", 1)


@pytest.mark.parametrize("log_n", [20, 21])
def test_ntt_large_three_pass(gpu_workers, oracle, log_n):
    w = gpu_workers("bn254")
    v = oracle.rand_fr(0, 77, 1 << log_n)
    for inv, coset in [(False, True), (True, True)]:
        got = w.ntt(v, inv, coset)
        want = oracle.ntt(0, v, inv, coset, threads=8)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- forced plans (option ntt_max_log_r)
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", FORCED_PLANS)
def test_ntt_forced_plan_matches_oracle(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """w.ntt in all four modes with both butterfly forms under a plan forced by ntt_max_log_r, bit-exact against the oracle: three-pass
    plans on BLS12-381 and in the plain modes, four-pass plans, widths 3 and 4 as middle and last passes and width 5 as a middle pass
    (inter-pass planes keyed by the widths on both sides) — none of which the default plans reach below 2^23 points.  The list
    (ntt_plans.FORCED_PLANS) holds each width 2 ... 7 as a first, a middle and a last pass of a three-pass plan (2 leads only 2+2) and
    the four-pass plans; test_abi_and_host_logic.py checks that without a GPU.  Width 8 or 9 as a MIDDLE pass needs 2^23 points or
    more: that stays with test_gpu_fullsize.py."""
    w = gpu_workers(curve)
    seed = 3000 + log_n
    v = oracle.rand_fr(cid, seed, 1 << log_n)
    plan = plan_str(log_n, max_log_r)
    try:
        w.set_option("ntt_max_log_r", max_log_r)
        for inv, coset in MODES:
            want = oracle_ntt(oracle, cid, v, seed, log_n, inv, coset)
            for shoup in (1, 0):
                w.set_option("ntt_shoup", shoup)
                assert np.array_equal(w.ntt(v, inv, coset), want), f"{curve} 2^{log_n} plan {plan} shoup={shoup} inv={inv} coset={coset}"
    finally:
        w.set_option("ntt_max_log_r", 9)
        w.set_option("ntt_shoup", 1)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", [(3, 12), (4, 16)])
def test_ntt_forced_four_pass_plan_on_extreme_inputs(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """The extreme inputs of test_ntt_extreme_inputs_and_both_butterfly_forms through a FOUR-pass plan: the per-stage growth the pass kernel
    budgets for (4p per stage, under 36p) then spans the largest number of inter-pass canonicalisations a plan can have."""
    w = gpu_workers(curve)
    plan = plan_str(log_n, max_log_r)
    assert plan.count("+") == 3
    cases = extreme_inputs(oracle, cid, log_n)
    try:
        w.set_option("ntt_max_log_r", max_log_r)
        for i, v in enumerate(cases):
            for inv, coset in MODES:
                want = oracle.ntt(cid, v, inv, coset, threads=8)
                for shoup in (1, 0):
                    w.set_option("ntt_shoup", shoup)
                    assert np.array_equal(w.ntt(v, inv, coset), want), f"{curve} 2^{log_n} plan {plan} input {i} shoup={shoup} inv={inv} coset={coset}"
    finally:
        w.set_option("ntt_max_log_r", 9)
        w.set_option("ntt_shoup", 1)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", [(3, 9), (3, 12), (4, 12), (4, 16)])
def test_ntt_dev_forced_three_and_four_pass_plans(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """plonk_ntt_dev (device buffers, input and output apart) under forced three- and four-pass plans, forward and inverse, coset and plain"""
    w = gpu_workers(curve)
    n = 1 << log_n
    seed = 3000 + log_n
    v = oracle.rand_fr(cid, seed, n)
    plan = plan_str(log_n, max_log_r)
    assert plan.count("+") in (2, 3)
    d_in, d_out = w.alloc(n * 32), w.alloc(n * 32)
    try:
        w.set_option("ntt_max_log_r", max_log_r)
        for inv, coset in MODES:
            d_in.upload(v)                                    # a multi-pass transform leaves its intermediate values in the input buffer
            w.ntt_dev(d_in.ptr, d_out.ptr, n, inv, coset)
            assert np.array_equal(d_out.download((n, 4)), oracle_ntt(oracle, cid, v, seed, log_n, inv, coset)), f"{curve} 2^{log_n} plan {plan} inv={inv} coset={coset}"
    finally:
        w.set_option("ntt_max_log_r", 9)
        w.set_option("ntt_shoup", 1)
        d_in.free(); d_out.free()


def test_ntt_forced_plan_of_too_many_passes_is_refused(gpu_workers, oracle):
    """2^13 points in passes of at most 2^3 rows would be five passes (NTT_MAX_PASSES is 4): an error, after which the worker still works"""
    from distributed_plonk_amd._ffi import PlonkError
    w = gpu_workers("bn254")
    assert len(plan_widths(13, 3)) == 5 and len(plan_widths(12, 3)) == 4
    try:
        w.set_option("ntt_max_log_r", 3)
        with pytest.raises(PlonkError) as e:
            w.ntt(oracle.rand_fr(0, 3013, 1 << 13))
        assert "too many passes" in str(e.value), f"plan {plan_str(13, 3)}: {e.value}"
        v = oracle.rand_fr(0, 3012, 1 << 12)
        assert np.array_equal(w.ntt(v, False, True), oracle_ntt(oracle, 0, v, 3012, 12, False, True)), f"plan {plan_str(12, 3)} after the refusal"
    finally:
        w.set_option("ntt_max_log_r", 9)
        w.set_option("ntt_shoup", 1)


def test_playground_identities(gpu_workers, oracle):
    """playground.rs:100-102."""
    w = gpu_workers("bls12_381")
    l = 512
    exps = oracle.rand_fr(1, 5, l)
    t = np.zeros((2 * l, 4), dtype=np.uint64)
    t[:l] = exps
    assert np.array_equal(w.ntt(t, False, True), oracle.ntt(1, t, False, True))      # zero padding
    assert np.array_equal(w.ntt(w.ntt(exps, False, True), True, True), exps)         # coset round trip
    assert np.array_equal(w.ntt(w.ntt(exps, False, False), True, False), exps)


def test_domain_errors(gpu_workers):
    from distributed_plonk_amd._ffi import PlonkError
    w = gpu_workers("bn254")
    with pytest.raises(PlonkError) as e:
        w.ntt(np.zeros((3, 4), dtype=np.uint64))
    assert e.value.code == -2
    with pytest.raises(PlonkError):
        w.init(None, 1 << 29, 0)          # BN254 two-adicity is 28


def test_transpose(gpu_workers, oracle):
    w = gpu_workers("bn254")
    for rows, cols in [(32, 64), (64, 32), (48, 80), (1, 7)]:
        v = oracle.rand_fr(0, rows * cols, rows * cols)
        got = w.transpose(v, rows, cols)
        want = v.reshape(rows, cols, 4).transpose(1, 0, 2).reshape(-1, 4)
        assert np.array_equal(got, want)
