"""The MSM engine's host planner and its digit decomposition restated for the tests that force plan shapes (tests/test_gpu_msm_plans.py):
`plan` is msm_plan / plan_window / sort_geometry / msm_group / msm_launch_sets of csrc/msm_engine.hip (the host side; the kernels are
csrc/msm_kernels.hpp) written again in Python and compared field by field with
what the engine reports through plonk_msm_plan; `signed_digits`, `partition_lengths`, `chunks`, `chunk_entries` and `heavy_buckets` restate the
data-dependent choices of msm_digits_kernel, sort_partition_staged_kernel and msm_accumulate_kernel, so that a case can say before it runs which
of their branches its scalars reach; PLAN_CASES is the case table, every row naming the branches it exists for (FEATURES)."""
import numpy as np

from distributed_plonk_amd._ffi import MSM_PLAN_FIELDS

FR_BITS = {0: 254, 1: 255}                       # fr_params(curve).bits: BN254, BLS12-381

# kernel constants as the engine reports them (the restatement test compares; `chunks` and `heavy_buckets` read them from the plan they are given)
SORT_SLICE_LOG, STAGE_THREADS, STAGE_MAX_CHUNKS, HEAVY_BUCKET, HEAVY_SEGS, REDUCE_K = 14, 1024, 8, 2048, 8, 4
REDUCE_COST = 2.7 * 3300.0
DEFAULTS = {"msm_fused_order": 1, "msm_sort_stage_cap": 0, "msm_sort_slice_index": 0, "msm_reduce_grid": 0, "msm_acc_persist": 4, "msm_slice_log": 26,
            "msm_batch_max": 32, "msm_fused_y3": 1, "n_cu": 256}


def sort_geometry(cb, n):
    lp = max(min(cb, 10), cb - 11)
    return None if lp > 13 or n > (1 << 27) else lp


def window_usable(n, bits, c):
    if sort_geometry(c - 1, n) is None:
        return False
    W = (bits + c) // c
    return not (W > 1 and bits - (W - 1) * c < min(c - 3, 8))


def window_cost(n, bits, c, G):
    W = (bits + c) // c
    sets = float(min(max(G, 1), W))
    par = min(1.0, sets * float(1 << (c - 1)) / 262144.0)
    return float(W) * float(n) * 2480.0 / par + sets * float(1 << (c - 1)) * REDUCE_COST


def choose_window(n, bits):
    best, bc = 1e300, 4
    for c in range(4, 21):
        if window_usable(n, bits, c):
            cost = window_cost(n, bits, c, (bits + c) // c)
            if cost < best:
                best, bc = cost, c
    return bc


def plan_window(n, bits, window):
    """no fixed-base table (msm_precompute = 0, the default; the table keeps its own tests)"""
    return min(max(window, 2), 20) if window > 0 else choose_window(n, bits)


def plan(bits, n, K, window=0, options=None):
    """The fields of plonk_msm_plan for K vectors over n points, forced window `window` (0 = automatic) and `options` (plonk_set_option keys, plus
    "n_cu": the device's CU count); None where the engine refuses."""
    o = dict(DEFAULTS)
    o.update(options or {})
    if n <= 0 or K <= 0:
        return None
    m = min(1 << min(max(o["msm_slice_log"], 8), 26), n)
    c = plan_window(m, bits, window)
    W1 = (bits + c) // c
    group = max(1, min(K, 0xfffffff0 // (m * W1)))
    if group * W1 > 65535:
        group = 65535 // W1
    group = min(group, min(max(o["msm_batch_max"], 1), 64))
    n, K = m, min(group, K)
    G, W, cb = W1, K * W1, c - 1
    nbuckets = (K * G) << cb
    if nbuckets >= 0xffffffff:
        return None
    avg = (n * W) // nbuckets + 1
    heavy_thresh = max(HEAVY_BUCKET, 4 * avg)
    bin_shift = 0
    while (avg >> bin_shift) > 96:
        bin_shift += 1
    if n * W >= 0xffffffff:
        return None
    lp = sort_geometry(cb, n)
    if lp is None:
        return None
    low_bits = cb - lp
    nblk = (n + (1 << SORT_SLICE_LOG) - 1) >> SORT_SLICE_LOG
    ln = 1
    while (1 << ln) < n:
        ln += 1
    idx_bits = ln if low_bits + 1 + ln <= 32 else 0
    if o["msm_sort_slice_index"]:
        idx_bits = 0
    lev_k, lev_nch, cur = [], [], 1 << cb
    while cur > 1 and len(lev_k) < 15:
        lev_k.append(min(REDUCE_K, cur))
        lev_nch.append(cur // lev_k[-1])
        cur = lev_nch[-1]
    gsplit = min(32, max(1, (lev_nch[0] if lev_k else 1) // 2048))
    fo = o["msm_fused_order"]
    fused = fo == 2 or (fo == 1 and n * K >= (1 << 23))
    lds_fixed = ((1 << low_bits) + (0 if idx_bits else nblk)) * 4
    lds_staged = 78 * 1024
    stage_cap = (lds_staged - lds_fixed) // 4 if lds_fixed + 4096 * 4 <= lds_staged else 0
    if o["msm_sort_stage_cap"] > 0 and stage_cap:
        stage_cap = min(stage_cap, max(o["msm_sort_stage_cap"], STAGE_THREADS))
    staged = low_bits >= 8 and stage_cap >= STAGE_THREADS
    acc_grid, persistent = (nbuckets + 255) // 256, False
    if o["msm_acc_persist"] != 0:
        pgrid = o["n_cu"] * o["msm_acc_persist"] if o["msm_acc_persist"] > 0 else -o["msm_acc_persist"]
        if pgrid < acc_grid:
            acc_grid, persistent = pgrid, True
    out = {"c": c, "W1": W1, "G": G, "cb": cb, "lp": lp, "low_bits": low_bits, "nblk": nblk, "idx_bits": idx_bits,
           "packed": int(low_bits + SORT_SLICE_LOG + 1 + lp <= 32), "staged": int(staged), "stage_cap": stage_cap, "fused_order": int(fused),
           "nlev": len(lev_k), "last_k": lev_k[-1] if lev_k else 0, "gsplit": gsplit, "heavy_thresh": heavy_thresh, "persistent": int(persistent),
           "grid_mode": int(o["msm_reduce_grid"] != 0 and cb >= 2), "STAGE_MAX_CHUNKS": STAGE_MAX_CHUNKS, "STAGE_THREADS": STAGE_THREADS,
           "HEAVY_BUCKET": HEAVY_BUCKET, "HEAVY_SEGS": HEAVY_SEGS, "SORT_SLICE_LOG": SORT_SLICE_LOG, "n": n, "K": K, "n_cu": o["n_cu"],
           "acc_grid": acc_grid, "bin_shift": bin_shift}
    assert tuple(out) == MSM_PLAN_FIELDS
    return out


# ---- the data-dependent side
def signed_digits(scalars, c, W1):
    """msm_digits_kernel: scalars (n, 4) uint64 canonical -> (W1, n) uint32 of magnitude | sign << 31, magnitudes 0 .. 2^(c-1)"""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = s.shape[0]
    s = np.concatenate([s, np.zeros((n, 2), dtype=np.uint64)], axis=1)
    half, mask = np.uint64(1 << (c - 1)), np.uint64((1 << c) - 1)
    carry = np.zeros(n, dtype=np.uint64)
    out = np.zeros((W1, n), dtype=np.uint32)
    for w in range(W1):
        limb, off = (w * c) >> 6, (w * c) & 63
        v = s[:, limb] >> np.uint64(off) if limb < 4 else np.zeros(n, dtype=np.uint64)
        if off + c > 64 and limb < 4:
            v = v | (s[:, limb + 1] << np.uint64(64 - off))
        raw = (v & mask) + carry
        carry = (raw > half).astype(np.uint64)
        mag = np.where(carry == 1, np.uint64(1 << c) - raw, raw)
        out[w] = (mag | (carry << np.uint64(31))).astype(np.uint32)
    return out


def digits_value(dig, c):
    """the integers a digit array stands for (the check of signed_digits itself)"""
    vals = [0] * dig.shape[1]
    for w in range(dig.shape[0] - 1, -1, -1):
        for i, d in enumerate(dig[w].tolist()):
            vals[i] = (vals[i] << c) + (-(d & 0x7fffffff) if d >> 31 else d)
    return vals


def partition_lengths(digits, plan):
    """entries per (window, level-1 partition): (W, 2^lp); zero digits are dropped by the sort"""
    mag = digits & np.uint32(0x7fffffff)
    out = np.zeros((digits.shape[0], 1 << plan["lp"]), dtype=np.int64)
    for w in range(digits.shape[0]):
        nz = mag[w][mag[w] != 0]
        out[w] = np.bincount((nz - 1) >> np.uint32(plan["low_bits"]), minlength=1 << plan["lp"])
    return out


def bucket_counts(digits, plan, w, part):
    """entries of the 2^low_bits buckets of one partition"""
    mag = digits[w] & np.uint32(0x7fffffff)
    key = mag[mag != 0].astype(np.int64) - 1
    key = key[(key >> plan["low_bits"]) == part]
    return np.bincount(key & ((1 << plan["low_bits"]) - 1), minlength=1 << plan["low_bits"])


def chunks(length, plan):
    """sort_partition_staged_kernel's choice for a partition of `length` entries: (chunks, direct, buckets per chunk)"""
    cap, nlow = plan["stage_cap"], 1 << plan["low_bits"]
    nch = 1 if length <= cap else min(nlow, (length + (cap - cap // 4) - 1) // (cap - cap // 4))
    direct = nch > plan["STAGE_MAX_CHUNKS"]
    if direct:
        nch = 1
    return nch, direct, (nlow + nch - 1) // nch


def chunk_entries(counts, plan):
    """per chunk of a partition with the given bucket counts: (entries, staged in LDS) — a chunk above the buffer takes the direct path alone"""
    nch, direct, bper = chunks(int(counts.sum()), plan)
    out = []
    for k0 in range(0, len(counts), bper):
        e = int(counts[k0:k0 + bper].sum())
        out.append((e, (not direct) and e <= plan["stage_cap"]))
    return out


def heavy_buckets(digits, plan):
    """(window, bucket, entries) of the buckets above heavy_thresh (plain bucket sets: a bucket is one sorted segment)"""
    out = []
    mag = digits & np.uint32(0x7fffffff)
    for w in range(digits.shape[0]):
        nz = mag[w][mag[w] != 0].astype(np.int64) - 1
        cnt = np.bincount(nz, minlength=1)
        out += [(w, int(b), int(cnt[b])) for b in np.nonzero(cnt > plan["heavy_thresh"])[0]]
    return out


# ---- scalar vectors of the cases (canonical, (n, 4) uint64)
def make_scalars(kind, O, cid, n, p, seed=71):
    rnd = O.from_mont(cid, O.rand_fr(cid, seed, n)).copy()
    if kind == "uniform":                          # with 0, 1 and r - 1 among them
        rnd[0] = 0
        if n > 2:
            rnd[1] = [1, 0, 0, 0]
            rnd[2] = O.field_const(cid, 0, 0) - np.array([1, 0, 0, 0], dtype=np.uint64)
        return rnd
    if kind == "all-equal":
        return np.repeat(rnd[5:6], n, axis=0)
    # the low c bits uniform in [1, 2^low_bits]: window 0's partition 0 holds all n entries (no carry: 2^low_bits < 2^(c-1)); the other bits random
    assert kind in ("one-partition", "one-partition-half") and p["c"] < 64 and p["low_bits"] >= 1
    low = np.random.default_rng(seed + cid).integers(1, (1 << p["low_bits"]) + 1, size=n, dtype=np.uint64)
    if kind == "one-partition-half":               # every second point shares one low digit: a chunk above any buffer, and a heavy bucket
        low[::2] = np.uint64((1 << p["low_bits"]) // 2 + 3)
    rnd[:, 0] = (rnd[:, 0] & ~np.uint64((1 << p["c"]) - 1)) | low
    return rnd


# ---- the branches a case can name: predicate(row, plan, data), data(w, part) -> (partition length, its bucket counts)
class CaseData:
    """digits of a case's scalars under its plan, computed on first use"""

    def __init__(self, scalars, p):
        self.scalars, self.p, self._dig = scalars, p, None

    @property
    def digits(self):
        if self._dig is None:
            self._dig = signed_digits(self.scalars(), self.p["c"], self.p["W1"])
        return self._dig

    def largest(self):
        """(length, chunk list) of the largest partition"""
        pl = partition_lengths(self.digits, self.p)
        w, part = np.unravel_index(int(pl.argmax()), pl.shape)
        return int(pl[w, part]), chunk_entries(bucket_counts(self.digits, self.p, int(w), int(part)), self.p)


def _largest_chunks(p, d):
    length, ch = d.largest()
    return chunks(length, p)[:2], ch


def _slice_rel(p):
    return p["idx_bits"] == 0 and p["nblk"] >= 3 and p["n"] % (1 << p["SORT_SLICE_LOG"]) != 0


FEATURES = {
    "direct-low0": lambda r, p, d: not p["staged"] and p["low_bits"] == 0,
    "direct-low7-packed-boundary": lambda r, p, d: not p["staged"] and p["c"] == 18 and p["low_bits"] == 7 and p["packed"] == 1
                                                   and p["low_bits"] + p["SORT_SLICE_LOG"] + 1 + p["lp"] == 32,
    "staged-c19": lambda r, p, d: p["staged"] == 1 and p["c"] == 19 and p["low_bits"] == 8 and p["packed"] == 0,
    "staged-c20": lambda r, p, d: p["staged"] == 1 and p["c"] == 20 and p["packed"] == 0,
    "staged-one-chunk": lambda r, p, d: p["staged"] == 1 and d.largest()[0] >= p["n"] and _largest_chunks(p, d)[0] == (1, False)
                                        and all(s for _, s in _largest_chunks(p, d)[1]),
    "staged-2-8-chunks": lambda r, p, d: p["staged"] == 1 and 2 <= _largest_chunks(p, d)[0][0] <= p["STAGE_MAX_CHUNKS"] and not _largest_chunks(p, d)[0][1]
                                         and all(s for _, s in _largest_chunks(p, d)[1]),
    "staged-direct-fallback": lambda r, p, d: p["staged"] == 1 and _largest_chunks(p, d)[0][1],
    "staged-mixed-chunks": lambda r, p, d: p["staged"] == 1 and not _largest_chunks(p, d)[0][1]
                                           and {s for _, s in _largest_chunks(p, d)[1]} == {True, False},
    "fused-order-off": lambda r, p, d: p["fused_order"] == 0,
    "fused-order-on": lambda r, p, d: p["fused_order"] == 1,
    "slice-index-direct": lambda r, p, d: not p["staged"] and _slice_rel(p),
    "slice-index-staged": lambda r, p, d: p["staged"] == 1 and _slice_rel(p),
    "gsplit-1": lambda r, p, d: p["gsplit"] == 1,
    "gsplit-2-c15": lambda r, p, d: p["gsplit"] == 2 and p["c"] == 15,
    "gsplit-mid": lambda r, p, d: 2 < p["gsplit"] < 32,
    "gsplit-32": lambda r, p, d: p["gsplit"] == 32,
    "last-level-k2": lambda r, p, d: p["last_k"] == 2 and p["cb"] % 2 == 1,
    "last-level-k4": lambda r, p, d: p["last_k"] == 4,
    "heavy-bucket": lambda r, p, d: len(heavy_buckets(d.digits, p)) >= 1,
    "batched-staged-gsplit": lambda r, p, d: p["K"] == 3 and r["K"] == 3 and p["staged"] == 1 and p["gsplit"] > 1,
    "fused-y3-0": lambda r, p, d: r["opts"].get("msm_fused_y3", 1) == 0,
    "fused-y3-1": lambda r, p, d: r["opts"].get("msm_fused_y3", 1) == 1,
    "persistent": lambda r, p, d: p["persistent"] == 1,
}
STAGED_SHAPES = ("staged-c19", "staged-c20", "staged-one-chunk", "staged-2-8-chunks", "staged-direct-fallback", "staged-mixed-chunks")
# what the table must contain for each curve: single branches, and every staged shape with the bucket ordering outside and inside the sort
REQUIRED = [(f,) for f in FEATURES if f not in ("fused-order-off", "fused-order-on", "persistent")] + \
           [(s, f) for s in STAGED_SHAPES for f in ("fused-order-off", "fused-order-on")]


def _row(id, branches, n, window, scalars, K=1, emu=False, **opts):
    return {"id": id + ("-emu" if emu else ""), "branches": tuple(branches), "n": n, "window": window, "K": K, "scalars": scalars, "opts": opts}


FO, ON = "fused-order-off", "fused-order-on"
PLAN_CASES = [
    # window shapes, 2^12 uniform scalars: the smallest n that fills more than one block of every kernel
    _row("c11", ("direct-low0", "gsplit-1", "last-level-k4", FO), 1 << 12, 11, "uniform", emu=True),
    _row("c15", ("gsplit-2-c15", "last-level-k4"), 1 << 12, 15, "uniform", emu=True),
    _row("c17", ("gsplit-mid", "last-level-k4"), 1 << 12, 17, "uniform"),
    _row("c18", ("direct-low7-packed-boundary", "gsplit-mid", "last-level-k2"), 1 << 12, 18, "uniform"),
    _row("c19", ("staged-c19", "gsplit-32", "last-level-k4", FO), 1 << 12, 19, "uniform", msm_fused_order=0),
    _row("c19-fused", ("staged-c19", ON), 1 << 12, 19, "uniform", msm_fused_order=2),
    _row("c20", ("staged-c20", "gsplit-32", "last-level-k2", FO), 1 << 12, 20, "uniform", msm_fused_order=0),
    _row("c20-fused", ("staged-c20", ON), 1 << 12, 20, "uniform", msm_fused_order=2),
    # chunking of the staged kernel, 2^13 points all in window 0's partition 0
    _row("c20-one-chunk", ("staged-one-chunk", FO), 1 << 13, 20, "one-partition", msm_fused_order=0),
    _row("c20-one-chunk-fused", ("staged-one-chunk", ON), 1 << 13, 20, "one-partition", msm_fused_order=2),
    _row("c20-chunks", ("staged-2-8-chunks", FO), 1 << 13, 20, "one-partition", msm_fused_order=0, msm_sort_stage_cap=2048),
    _row("c20-chunks-fused", ("staged-2-8-chunks", ON), 1 << 13, 20, "one-partition", msm_fused_order=2, msm_sort_stage_cap=2048),
    _row("c19-chunks-fused", ("staged-c19", "staged-2-8-chunks", ON), 1 << 13, 19, "one-partition", msm_fused_order=2, msm_sort_stage_cap=2048),
    _row("c20-direct-fallback", ("staged-direct-fallback", FO), 1 << 13, 20, "one-partition", msm_fused_order=0, msm_sort_stage_cap=1024),
    _row("c20-direct-fallback-fused", ("staged-direct-fallback", ON), 1 << 13, 20, "one-partition", msm_fused_order=2, msm_sort_stage_cap=1024),
    _row("c20-mixed-chunks", ("staged-mixed-chunks", "heavy-bucket", FO), 1 << 13, 20, "one-partition-half", msm_fused_order=0, msm_sort_stage_cap=2048),
    _row("c20-mixed-chunks-fused", ("staged-mixed-chunks", "heavy-bucket", ON), 1 << 13, 20, "one-partition-half", msm_fused_order=2, msm_sort_stage_cap=2048),
    # slice-relative indices: three slices, the last ragged
    _row("c12-slice-index", ("slice-index-direct",), 39768, 12, "uniform", msm_sort_slice_index=1),
    _row("c18-slice-index", ("slice-index-direct", "direct-low7-packed-boundary"), 39768, 18, "uniform", msm_sort_slice_index=1),
    _row("c18-slice-index-one-partition", ("slice-index-direct",), 39768, 18, "one-partition", msm_sort_slice_index=1),
    _row("c20-slice-index", ("slice-index-staged", "staged-c20"), 39768, 20, "uniform", msm_sort_slice_index=1),
    _row("c20-slice-index-one-partition", ("slice-index-staged", "staged-2-8-chunks"), 39768, 20, "one-partition", msm_sort_slice_index=1),
    _row("c20-slice-index-chunks", ("slice-index-staged",), 39768, 20, "uniform", msm_sort_slice_index=1, msm_sort_stage_cap=2048),
    _row("c20-slice-index-chunks-one-partition", ("slice-index-staged", "staged-direct-fallback"), 39768, 20, "one-partition", msm_sort_slice_index=1,
         msm_sort_stage_cap=2048),
    _row("c20-slice-index-chunks-8192-one-partition", ("slice-index-staged", "staged-2-8-chunks"), 39768, 20, "one-partition", msm_sort_slice_index=1,
         msm_sort_stage_cap=8192),
    # the accumulation with Y3 as two products
    _row("y3-split", ("fused-y3-0",), 1 << 12, 0, "uniform", emu=True, msm_fused_y3=0),
    _row("y3-split-all-equal", ("fused-y3-0", "heavy-bucket"), 1 << 12, 0, "all-equal", emu=True, msm_fused_y3=0),
    _row("y3-split-persistent", ("fused-y3-0", "persistent"), 1 << 12, 0, "uniform", emu=True, msm_fused_y3=0, msm_acc_persist=-3),
    _row("y3-fused", ("fused-y3-1",), 1 << 12, 0, "uniform", emu=True, msm_fused_y3=1),
    _row("y3-fused-all-equal", ("fused-y3-1", "heavy-bucket"), 1 << 12, 0, "all-equal", emu=True, msm_fused_y3=1),
    # batched: three ragged vectors (n, n - 37, 1) in one launch set
    _row("c20-batched", ("batched-staged-gsplit", "staged-c20", ON), 1 << 12, 20, "uniform", K=3, msm_fused_order=2),
    _row("c15-batched", ("gsplit-2-c15",), 1 << 12, 15, "uniform", K=3, emu=True, msm_fused_order=2),
]


def missing_branches(rows, holds):
    """the entries of REQUIRED that no row both names and reaches; holds(row, feature) -> bool"""
    return [" + ".join(req) for req in REQUIRED if not any(all(f in r["branches"] and holds(r, f) for f in req) for r in rows)]
