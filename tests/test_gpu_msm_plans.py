"""Every plan branch of the MSM engine at the smallest size that reaches it, on both curves.  The engine reports the plan it would run
(plonk_msm_plan: the host function msm_slice itself consumes), tests/msm_plans.py restates the planner and the data-dependent choices of the
kernels, and each row of its PLAN_CASES names the branches it exists for: a case asserts them from the engine's plan BEFORE it runs and then
compares the point with the oracle in affine form, exactly.  The plan query launches nothing, so the restatement is compared with the engine at
every size up to 2^26 in no time."""
import itertools

import numpy as np
import pytest

import msm_plans as M
from distributed_plonk_amd._ffi import MsmWorkload, PlonkError

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
RESTORE = {"msm_window": 0, "msm_fused_order": 1, "msm_sort_stage_cap": 0, "msm_sort_slice_index": 0, "msm_reduce_grid": 0, "msm_fused_y3": 1,
           "msm_acc_persist": 4}
_cache = {}


def _set(w, opts):
    for k, v in opts.items():
        w.set_option(k, v)


def _plan_of(w, row):
    """the engine's plan for a row; the caller restores the options"""
    _set(w, RESTORE)
    _set(w, row["opts"])
    w.set_option("msm_window", row["window"])
    return w.msm_plan(row["n"], row["K"])


def _inputs(oracle, cid, n):
    """duplicated bases (P + P in a bucket: the redo path) with one infinity base among them, shared by every case of that size"""
    key = ("bases", cid, n)
    if key not in _cache:
        bases = oracle.gen_bases(cid, 61, 300, n)
        b, inf = bases.copy(), np.zeros(n, dtype=np.uint8)
        b[11], inf[11] = 0, 1
        _cache[key] = (bases, b, inf)
    return _cache[key]


def _scalars(oracle, cid, row, p):
    key = ("sc", cid, row["n"], row["scalars"], p["c"], p["low_bits"])
    if key not in _cache:
        _cache[key] = M.make_scalars(row["scalars"], oracle, cid, row["n"], p)
    return _cache[key]


def _want(oracle, cid, n, sc_key, sc, ln=None):
    """the oracle's point, computed once per (curve, bases, scalar vector)"""
    key = ("want", cid, n, sc_key, ln)
    if key not in _cache:
        bases, _, inf = _inputs(oracle, cid, n)
        ln = n if ln is None else ln
        _cache[key] = oracle.jac_to_affine(cid, oracle.msm(cid, bases[:ln], sc[:ln], inf[:ln], threads=8))
    return _cache[key]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_planner_restatement_matches_the_engine(gpu_workers, curve, cid):
    """msm_plans.plan against plonk_msm_plan on every field: forced windows 2 ... 20 and the automatic choice, sizes from 1 to 2^26 (the natural
    idx_bits == 0 cases at 2^24, 2^22 against 2^22 + 1 at c = 20), one and three vectors, and the product of the options the planner reads.
    Where the engine refuses (n * W beyond 32 bits) the restatement says None."""
    w = gpu_workers(curve)
    bits = M.FR_BITS[cid]
    sizes = [1, 5, 1 << 10, 1 << 12, 1 << 13, 1 << 14, (1 << 14) + 1, 39768, 1 << 16, 1 << 18, 1 << 22, (1 << 22) + 1, 1 << 24, 1 << 26]
    checked = refused = 0
    try:
        _set(w, RESTORE)
        n_cu = w.msm_plan(1 << 12, 1)["n_cu"]
        for fo, cap, si, gr in itertools.product((0, 1, 2), (0, 1024, 2048, 3000), (0, 1), (0, 1)):
            opts = {"msm_fused_order": fo, "msm_sort_stage_cap": cap, "msm_sort_slice_index": si, "msm_reduce_grid": gr}
            _set(w, opts)
            for window in [0] + list(range(2, 21)):
                w.set_option("msm_window", window)
                for n, K in itertools.product(sizes, (1, 3)):
                    want = M.plan(bits, n, K, window, dict(opts, n_cu=n_cu))
                    try:
                        got = w.msm_plan(n, K)
                    except PlonkError:
                        got = None
                        refused += 1
                    assert got == want, (opts, window, n, K, {k: (got[k], want[k]) for k in got if got[k] != want[k]} if got and want else (got, want))
                    checked += 1
        # the forms the list exists for
        _set(w, RESTORE)
        w.set_option("msm_window", 20)
        assert w.msm_plan(1 << 22, 1)["idx_bits"] == 22 and w.msm_plan((1 << 22) + 1, 1)["idx_bits"] == 0 and w.msm_plan(1 << 24, 1)["idx_bits"] == 0
        w.set_option("msm_window", 0)
        p = w.msm_plan(1 << 24, 1)
        assert (p["c"], p["idx_bits"], p["staged"], p["fused_order"], p["gsplit"]) == (20, 0, 1, 1, 32), p
        assert checked == 48 * 20 * 28 and 0 < refused < checked // 10
    finally:
        _set(w, RESTORE)


@pytest.mark.parametrize("curve,cid", CURVES)
def test_case_table_reaches_every_branch_it_names(gpu_workers, oracle, curve, cid):
    """Every row of PLAN_CASES reaches each branch it names, and the table holds every branch of msm_plans.REQUIRED — judged from the ENGINE's plan
    and, for the data-dependent branches (chunks of the staged kernel, heavy buckets), from the restated digits of the row's own scalars.  A row
    that stops reaching its branch fails here by the branch's name."""
    w = gpu_workers(curve)
    try:
        held = {}
        for row in M.PLAN_CASES:
            p = _plan_of(w, row)
            data = M.CaseData(lambda row=row, p=p: _scalars(oracle, cid, row, p), p)
            for f in row["branches"]:
                held[(row["id"], f)] = bool(M.FEATURES[f](row, p, data))
                assert held[(row["id"], f)], f"case {row['id']} no longer reaches the branch '{f}' on {curve}: plan {p}"
        missing = M.missing_branches(M.PLAN_CASES, lambda r, f: held[(r["id"], f)])
        assert not missing, f"no case of PLAN_CASES reaches: {missing}"
    finally:
        _set(w, RESTORE)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("row", M.PLAN_CASES, ids=lambda r: r["id"])
def test_plan_case_matches_oracle(gpu_workers, oracle, curve, cid, row):
    w = gpu_workers(curve)
    n, K = row["n"], row["K"]
    _, b, _ = _inputs(oracle, cid, n)
    try:
        p = _plan_of(w, row)
        data = M.CaseData(lambda: _scalars(oracle, cid, row, p), p)
        for f in row["branches"]:
            assert M.FEATURES[f](row, p, data), f"case {row['id']} does not reach the branch '{f}': plan {p}"
        w.init(b, 0, 0)
        if K == 1:
            sc = _scalars(oracle, cid, row, p)
            got = w.g1_to_affine(w.var_msm(MsmWorkload(0, n), sc))
            want = _want(oracle, cid, n, (row["scalars"], p["c"], p["low_bits"]), sc)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), row["id"]
        else:
            lens = (n, n - 37, 1)[:K]
            vecs = [oracle.rand_fr(cid, 80 + k, n) for k in range(K)]          # Montgomery form: the commitment entry points take coefficients
            bufs = [w.alloc(n * 32) for _ in vecs]
            try:
                for d, v in zip(bufs, vecs):
                    d.upload(v)
                pts = w.commit_many_dev([(d.ptr, ln) for d, ln in zip(bufs, lens)])
            finally:
                for d in bufs:
                    d.free()
            for k, (v, ln, pt) in enumerate(zip(vecs, lens, pts)):
                got = w.g1_to_affine(pt)
                want = _want(oracle, cid, n, ("mont", 80 + k), oracle.from_mont(cid, v), ln)
                assert got[1] == want[1] and np.array_equal(got[0], want[0]), (row["id"], k)
    finally:
        _set(w, RESTORE)
