"""The passes of the MSM sort in front of the bucket accumulation, at the smallest sizes where each can go wrong: the level-1 kernel that cuts the
digits and counts the partition histograms in one pass over the scalars (window groups, zero-digit padding of short vectors, the carry chain), the
level-1 scatter that keeps a lane's 16 digits in registers (partial last slice, lanes without a valid entry) and the staged level-2 kernel that
keeps a lane's entries in registers when the partition is one chunk of at most 18 * 1024 entries (and streams it twice otherwise).  Every case
asserts the route it means to take from the engine's plan (and, where the route depends on the data, from the restated digits of its scalars)
BEFORE it runs, then compares the points with the oracle in affine form, exactly — on both curves, with plain scalars (var_msm) and with
Montgomery coefficients (commit_many_dev, one to five vectors of unequal lengths in one launch set)."""
import numpy as np
import pytest

import msm_plans as M
from distributed_plonk_amd._ffi import MsmWorkload

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
RESTORE = {"msm_window": 0, "msm_fused_order": 1, "msm_sort_stage_cap": 0, "msm_sort_slice_index": 0, "msm_reduce_grid": 0, "msm_fused_y3": 1,
           "msm_acc_persist": 4}
SLICE = 1 << M.SORT_SLICE_LOG
STAGE_KEEP = 18                      # entries per lane the staged level-2 kernel keeps in registers (csrc/msm_kernels.hpp)
DIGHIST_LDS_WORDS = 78 * 256         # histogram counters of the level-1 kernel per window group (csrc/msm_kernels.hpp)
_cache = {}


def _set(w, opts):
    for k, v in opts.items():
        w.set_option(k, v)


def _plan(w, n, K, window=0, **opts):
    _set(w, RESTORE)
    _set(w, opts)
    w.set_option("msm_window", window)
    return w.msm_plan(n, K)


def _bases(oracle, cid, n):
    """duplicated bases (P + P in a bucket) with one infinity among them, shared by every case of that size"""
    key = ("bases", cid, n)
    if key not in _cache:
        bases = oracle.gen_bases(cid, 61, 300, n)
        b, inf = bases.copy(), np.zeros(n, dtype=np.uint8)
        if n > 11:
            b[11], inf[11] = 0, 1
        _cache[key] = (bases, b, inf)
    return _cache[key]


def _want(oracle, cid, n, key, sc, ln):
    k = ("want", cid, n, key, ln)
    if k not in _cache:
        bases, _, inf = _bases(oracle, cid, n)
        _cache[k] = oracle.jac_to_affine(cid, oracle.msm(cid, bases[:ln], sc[:ln], inf[:ln], threads=8))
    return _cache[k]


def _limbs(v):
    return [(v >> (64 * i)) & 0xffffffffffffffff for i in range(4)]


def _modulus(oracle, cid):
    return sum(int(x) << (64 * i) for i, x in enumerate(oracle.field_const(cid, 0, 0)[:4]))


def _random(oracle, cid, seed, n):
    key = ("rnd", cid, seed, n)
    if key not in _cache:
        _cache[key] = oracle.from_mont(cid, oracle.rand_fr(cid, seed, n))
    return _cache[key]


def _check_plain(w, oracle, cid, n, key, sc):
    """one vector of canonical scalars through var_msm"""
    got = w.g1_to_affine(w.var_msm(MsmWorkload(0, n), sc))
    want = _want(oracle, cid, n, key, sc, n)
    assert got[1] == want[1] and np.array_equal(got[0], want[0]), ("plain", key)


def _check_mont(w, oracle, cid, n, keys, vecs, lens):
    """len(vecs) vectors as Montgomery coefficients through commit_many_dev, lens[k] of them valid"""
    bufs = [w.alloc(n * 32) for _ in vecs]
    try:
        for d, v in zip(bufs, vecs):
            d.upload(oracle.field_op(cid, 0, "to_mont", v))
        pts = w.commit_many_dev([(d.ptr, ln) for d, ln in zip(bufs, lens)])
    finally:
        for d in bufs:
            d.free()
    for k, (v, ln, pt) in enumerate(zip(vecs, lens, pts)):
        got = w.g1_to_affine(pt)
        if ln == 0:
            assert got[1], ("mont", keys[k], "empty vector is not the point at infinity")
            continue
        want = _want(oracle, cid, n, keys[k], v, ln)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), ("mont", keys[k], k, ln)


def _batch(oracle, cid, n, key0, sc0, lens):
    """vector 0 is the case's own, the others random: (keys, vectors) for _check_mont"""
    keys = [key0] + [("rnd", 90 + k) for k in range(1, len(lens))]
    return keys, [sc0] + [_random(oracle, cid, 90 + k, n) for k in range(1, len(lens))]


def _lens(n, K):
    return (n, 1, 0, n - 3, n)[:K]


def _wgroups(p):
    """window groups of the level-1 kernel: the W1 * (2^lp + 1) counters of a vector in groups of what DIGHIST_LDS_WORDS holds"""
    per = max(1, DIGHIST_LDS_WORDS // ((1 << p["lp"]) + 1))
    return (p["W1"] + per - 1) // per


# ---------------------------------------------------------------------------------------------- slice edges and unequal batches
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("n", [SLICE - 1, SLICE, SLICE + 1, 3 * SLICE - 5])
def test_slice_edges(gpu_workers, oracle, curve, cid, n):
    """A full slice, one entry short of it, one entry into the next (1023 of the scatter's 1024 lanes hold no valid digit of the last slice) and a
    ragged third slice: the register-cached sweeps mask what lies beyond the end."""
    w = gpu_workers(curve)
    try:
        p = _plan(w, n, 1)
        assert p["nblk"] == (n + SLICE - 1) // SLICE and p["n"] == n
        w.init(_bases(oracle, cid, n)[1], 0, 0)
        sc = M.make_scalars("uniform", oracle, cid, n, p)
        _check_plain(w, oracle, cid, n, "uniform", sc)
        _check_mont(w, oracle, cid, n, ["uniform"], [sc], [n])
    finally:
        _set(w, RESTORE)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("K", [1, 2, 5])
def test_batches_with_unequal_lengths(gpu_workers, oracle, curve, cid, K):
    """lens n, 1, 0, n - 3, n over two slices: the level-1 kernel writes the zero digits of the padding (and counts them in the zero bins), a
    vector of one scalar and an empty one ride along."""
    w = gpu_workers(curve)
    n = SLICE + 1
    try:
        p = _plan(w, n, K)
        assert p["K"] == K and p["nblk"] == 2
        w.init(_bases(oracle, cid, n)[1], 0, 0)
        sc = M.make_scalars("uniform", oracle, cid, n, p)
        keys, vecs = _batch(oracle, cid, n, "uniform", sc, _lens(n, K))
        _check_mont(w, oracle, cid, n, keys, vecs, _lens(n, K))
    finally:
        _set(w, RESTORE)


# ---------------------------------------------------------------------------------------------- digit edges and window groups
def _edge_scalars(oracle, cid, n, p):
    """0, 1, r - 1, 2^(c-1), the scalar whose every raw digit is 2^(c-1) (the largest positive digit in every window: no carry) and that scalar
    plus one (raw digit 2^(c-1) + 1 in window 0: the carry runs through every window into the top one), then random ones"""
    r, c, half = _modulus(oracle, cid), p["c"], 1 << (p["c"] - 1)
    allhalf, inc = 0, []
    for wd in range(p["W1"]):
        if allhalf + (half << (wd * c)) + 1 < r:
            allhalf += half << (wd * c)
            inc.append(wd)
    sc = _random(oracle, cid, 33, n).copy()
    vals = [0, 1, r - 1, half, allhalf, allhalf + 1, half + 1, r - half]
    for i, v in enumerate(vals):
        sc[i] = _limbs(v)
    dig = M.signed_digits(sc[:8], c, p["W1"])
    assert M.digits_value(dig, c) == vals
    assert [int(dig[wd, 4]) for wd in range(p["W1"])] == [half if wd in inc else 0 for wd in range(p["W1"])]      # the largest positive digit: no carry
    if inc == list(range(p["W1"] - 1)):            # one more in window 0: every window below the top one turns negative, the top one takes the carry
        assert all(int(dig[wd, 5]) >> 31 == 1 for wd in inc) and int(dig[p["W1"] - 1, 5]) == 1
    return sc


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("window,groups", [(4, 1), (9, 1), (11, 2), (13, 2), (14, 1), (16, 1), (0, None)])
def test_digit_edges_and_window_groups(gpu_workers, oracle, curve, cid, window, groups):
    """The fused digits of the edge scalars under windows whose histograms fit one LDS group (c = 4: 64 windows of 9 counters; c = 9, 14, 16) and
    under windows that need two (c = 11, 13: 24 and 20 windows of 1025 counters), and under the automatic window, one vector plain and three ragged ones in one set."""
    w = gpu_workers(curve)
    n = (1 << 12) + 3
    try:
        p = _plan(w, n, 3, window)
        assert groups is None or _wgroups(p) == groups, (p, _wgroups(p))       # (the automatic window: whatever the cost model picks)
        assert p["K"] == 3 and (window == 0 or p["c"] == window)
        if window == 4:
            assert p["W1"] == 64
        w.init(_bases(oracle, cid, n)[1], 0, 0)
        sc = _edge_scalars(oracle, cid, n, p)
        key = ("edges", p["c"])
        _check_plain(w, oracle, cid, n, key, sc)
        keys, vecs = _batch(oracle, cid, n, key, sc, (n, n - 3, 1))
        _check_mont(w, oracle, cid, n, keys, vecs, (n, n - 3, 1))
    finally:
        _set(w, RESTORE)


# ---------------------------------------------------------------------------------------------- every level-2 route
def _route(p, data):
    """the staged kernel's route for the largest partition of a case: 'direct-kernel' (not staged), 'kept' (one chunk from registers), 'one-chunk'
    (one chunk, two sweeps), 'chunks' (2 - 8), 'direct' (the staged kernel's one-pass fallback)"""
    if not p["staged"]:
        return "direct-kernel"
    length, _ = data.largest()
    nch, direct, _ = M.chunks(length, p)
    if direct:
        return "direct"
    if nch > 1:
        return "chunks"
    return "kept" if length <= STAGE_KEEP * p["STAGE_THREADS"] else "one-chunk"


KEEP_MAX = STAGE_KEEP * M.STAGE_THREADS
ROUTES = [
    # id, route, n, window, scalars, options
    ("c9", "direct-kernel", 1 << 12, 9, "uniform", {}),
    ("c19-kept-full", "kept", KEEP_MAX, 19, "one-partition", {}),
    ("c19-one-above", "one-chunk", KEEP_MAX + 1, 19, "one-partition", {}),
    ("c20-kept", "kept", 1 << 13, 20, "one-partition", {}),
    ("c20-kept-uniform-3-slices", "kept", 39768, 20, "uniform", {}),
    ("c20-chunks", "chunks", 1 << 13, 20, "one-partition", {"msm_sort_stage_cap": 2048}),
    ("c20-direct", "direct", 1 << 13, 20, "one-partition", {"msm_sort_stage_cap": 1024}),
]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("slice_index", [0, 1])
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c[0])
def test_level2_routes(gpu_workers, oracle, curve, cid, case, fused, slice_index):
    """Every route of the level-2 sort, entries with the full point index and with the index inside the slice, the bucket-size histogram inside
    and outside the sort; the partition of exactly 18 * 1024 entries is kept in registers, the one of 18 * 1024 + 1 (still one chunk of the
    buffer) is read twice.  Three vectors of unequal lengths, the case's own scalars first, and the same scalars alone in plain form."""
    name, route, n, window, kind, opts = case
    w = gpu_workers(curve)
    try:
        opts = dict(opts, msm_fused_order=fused, msm_sort_slice_index=slice_index)
        p = _plan(w, n, 3, window, **opts)
        assert p["c"] == window and p["K"] == 3 and p["fused_order"] == (fused == 2) and (p["idx_bits"] == 0) == (slice_index == 1)
        sc = M.make_scalars(kind, oracle, cid, n, p)
        data = M.CaseData(lambda: sc, p)
        assert _route(p, data) == route, (name, p, data.largest()[0])
        if route in ("kept", "one-chunk"):
            assert data.largest()[0] <= p["stage_cap"]
        if name == "c19-kept-full":
            assert data.largest()[0] == KEEP_MAX
        if name == "c19-one-above":
            assert data.largest()[0] == KEEP_MAX + 1
        w.init(_bases(oracle, cid, n)[1], 0, 0)
        key = (kind, p["c"], p["low_bits"])
        _check_plain(w, oracle, cid, n, key, sc)
        keys, vecs = _batch(oracle, cid, n, key, sc, (n, n - 3, 1))
        _check_mont(w, oracle, cid, n, keys, vecs, (n, n - 3, 1))
    finally:
        _set(w, RESTORE)
