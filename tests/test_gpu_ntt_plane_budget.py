"""The NTT's memory-pressure routes, forced at small sizes with option ntt_plane_budget (bytes of factor planes a context may hold) and
pinned bit for bit against the oracle.

ntt_pass_kernel takes its inter-pass and output factors from precomputed planes in HBM (get_plane / get_epi_plane / the planes of
get_shift_set, csrc/ntt_engine.hip) or, when the plane budget is exhausted, forms them on the fly: two table gathers and a product per
element (the `else` of `if (P.tw_plane != nullptr)`), two_level(P.epi, ...) for the output factor, two_level(P.pro, ...) for a coset shift
that could not be folded into a plane.  The default budget (48 GiB) keeps every other test on the planes; here the budget is a few KiB, so
that 2^9 ... 2^15-point transforms run plane-less, with the plain plane beside a coset shift in the prologue, with a plane for pass 0 only,
and so that the shared-input transforms (plonk_coset_eval_dev, plonk_fft1_dev_compact: no plane-less form) evict, refuse and recover.

Every case asserts the ROUTE before it compares values: the three plane generators are bracketed by profiling scopes, and after plonk_trim
nothing is cached, so the launch counts of "ntt_gen_plane" / "ntt_gen_epi_plane" / "ntt_gen_shift_plane" say which planes a transform got
(0 = plane-less, passes - 1 = fully planed, in between = a mixed plan)."""
import contextlib

import numpy as np
import pytest

from distributed_plonk_amd import _ffi
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.dispatcher import Dispatcher, make_fft_workloads, split_rc
from ntt_plans import plan_str, plan_widths
from test_gpu_coset_classes import _class_plan, _consts, _folded
from test_gpu_ntt import CURVES, MODES, extreme_inputs

pytestmark = pytest.mark.gpu

GENS = ("ntt_gen_plane", "ntt_gen_epi_plane", "ntt_gen_shift_plane")
ERR_HIP = {name: code for code, name in _ffi.ERR_NAMES.items()}["PLONK_ERR_HIP"]
NONE = (0, 0, 0)


def case_id(max_log_r, log_n):
    return f"n{log_n}r{max_log_r}"


def launches(w):
    """(inter-pass, output-factor, shared-input first-pass) planes generated since the last reset — process-wide counters"""
    return tuple(int(w.profile_get(name)[1]) for name in GENS)


def routed(w, call, want, where):
    """call() with the generator launch counts it caused checked against `want` BEFORE its result goes anywhere"""
    w.profile_reset()
    out = call()
    got = launches(w)
    assert got == tuple(want), f"{where}: plane generator launches {dict(zip(GENS, got))}, expected {tuple(want)}"
    return out


@contextlib.contextmanager
def plane_budget(workers, budget, max_log_r=9):
    """Every worker trimmed (nothing cached), then given the budget and the plan cap; profiling on.  Everything back to the defaults after."""
    try:
        for w in workers:
            w.trim()
            w.set_option("ntt_plane_budget", budget)
            w.set_option("ntt_max_log_r", max_log_r)
        workers[0].profile_enable(True)
        workers[0].profile_reset()
        yield
    finally:
        workers[0].profile_enable(False)
        workers[0].profile_reset()
        for w in workers:
            w.set_option("ntt_plane_budget", -1)
            w.set_option("ntt_max_log_r", 9)
            w.set_option("ntt_shoup", 1)
            w.trim()


def plain_plane_bytes(log_n, max_log_r):
    """bytes of the inter-pass planes of one plain forward transform: r_prev * 32 per non-last pass, r_prev = 2^log_n shrinking by each width"""
    r_prev, total = 1 << log_n, 0
    for width in plan_widths(log_n, max_log_r)[:-1]:
        total += r_prev * 32
        r_prev >>= width
    return total


_INPUTS, _WANT = {}, {}


def inputs(oracle, cid, log_n):
    """a random vector and the four extreme ones of test_gpu_ntt.py, built once per (curve, size), never modified"""
    if (cid, log_n) not in _INPUTS:
        vs = [oracle.rand_fr(cid, 5100 + log_n, 1 << log_n)] + extreme_inputs(oracle, cid, log_n)
        for v in vs:
            v.setflags(write=False)
        _INPUTS[cid, log_n] = vs
    return _INPUTS[cid, log_n]


def want_ntt(oracle, cid, log_n, i, inv, coset):
    """oracle.ntt of inputs(...)[i], computed once and shared by the plans and budgets the same vector runs under"""
    key = (cid, log_n, i, inv, coset)
    if key not in _WANT:
        _WANT[key] = oracle.ntt(cid, inputs(oracle, cid, log_n)[i], inv, coset, threads=8)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def ntt_dev(w, d_in, d_out, v, inv, coset):
    d_in.upload(v)                      # a multi-pass transform leaves its intermediate values in the input buffer
    w.ntt_dev(d_in.ptr, d_out.ptr, len(v), inv, coset)
    return d_out.download((len(v), 4))


# ---------------------------------------------------------------------------------------------- a. no plane at all
WHOLE = [(9, 10), (9, 11), (9, 13), (3, 9), (3, 12), (4, 12), (5, 15)]        # 5+5, 6+5, 7+6, 3+3+3, 3+3+3+3, 4+4+4, 5+5+5


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", WHOLE, ids=[case_id(*c) for c in WHOLE])
def test_budget_zero_whole_vector_transforms_run_without_planes(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """plonk_ntt and plonk_ntt_dev in all four modes with both butterfly forms under budget 0, on a random vector and the extreme ones (all
    p - 1, alternating, a single p - 1, half and half): every inter-pass factor is a tl * th product formed in the pass (not canonical, where the
    plane holds a canonical value), pass 0 of the inverse modes reads the 1/M-scaled tw_lo table, the forward coset shift stays in the prologue
    (two_level(P.pro, ...)).  Route: none of the three generators runs."""
    w = gpu_workers(curve)
    n, plan = 1 << log_n, plan_str(log_n, max_log_r)
    assert len(plan_widths(log_n, max_log_r)) >= 2, plan
    d_in, d_out = w.alloc(n * 32), w.alloc(n * 32)
    try:
        with plane_budget([w], 0, max_log_r):
            for shoup in (1, 0):
                w.set_option("ntt_shoup", shoup)
                for i, v in enumerate(inputs(oracle, cid, log_n)):
                    for inv, coset in MODES:
                        where = f"{curve} 2^{log_n} plan {plan} input {i} shoup={shoup} inv={inv} coset={coset}"
                        want = want_ntt(oracle, cid, log_n, i, inv, coset)
                        got = routed(w, lambda: w.ntt(v, inv, coset), NONE, where)
                        assert np.array_equal(got, want), where
                        got = routed(w, lambda: ntt_dev(w, d_in, d_out, v, inv, coset), NONE, where + " (ntt_dev)")
                        assert np.array_equal(got, want), where + " (ntt_dev)"
    finally:
        d_in.free(); d_out.free()


# ---------------------------------------------------------------------------------------------- b. the plain plane beside a prologue shift
PLAIN_CACHED = [(9, 10), (9, 13), (3, 9)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", PLAIN_CACHED, ids=[case_id(*c) for c in PLAIN_CACHED])
def test_plain_planes_cached_and_the_coset_shift_left_in_the_prologue(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """The budget holds exactly the planes of the plain forward transform.  That transform builds them (passes - 1 launches); the coset
    forward transform of the same size then finds no room for its folded plane, takes the plain ones from the cache and keeps its shift in the
    prologue (tw_plane != nullptr together with P.pro.enabled, a pairing no default plan produces); the inverse modes get no scale-folded
    pass-0 plane and run from the scaled tw_lo table (with the plain inverse planes of the later passes not fitting either).  No further
    generator launch in any of them, all exact."""
    w = gpu_workers(curve)
    widths = plan_widths(log_n, max_log_r)
    plan, NP = plan_str(log_n, max_log_r), len(widths)
    assert NP >= 2
    vs = inputs(oracle, cid, log_n)
    with plane_budget([w], plain_plane_bytes(log_n, max_log_r), max_log_r):
        got = routed(w, lambda: w.ntt(vs[0], False, False), (NP - 1, 0, 0), f"{curve} plan {plan}: the plain forward transform")
        assert np.array_equal(got, want_ntt(oracle, cid, log_n, 0, False, False))
        for shoup in (1, 0):
            w.set_option("ntt_shoup", shoup)
            for i, v in enumerate(vs):
                for inv, coset in [(False, True), (True, False), (True, True), (False, False)]:
                    where = f"{curve} 2^{log_n} plan {plan} input {i} shoup={shoup} inv={inv} coset={coset} beside the cached plain planes"
                    got = routed(w, lambda: w.ntt(v, inv, coset), NONE, where)
                    assert np.array_equal(got, want_ntt(oracle, cid, log_n, i, inv, coset)), where


# ---------------------------------------------------------------------------------------------- c. a plane for pass 0 only
MIXED = [(3, 9), (3, 12)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", MIXED, ids=[case_id(*c) for c in MIXED])
def test_mixed_plan_pass_0_planed_later_passes_on_the_fly(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """Budget = 2^log_n * 32, the pass-0 plane alone (folded with the coset shift / the 1/M scale where the mode has one: same size): pass 0
    streams its plane, passes 1 ... form their factors on the fly.  Exactly one generator launch per mode (each mode starts from a trimmed
    context), none for the further inputs of that mode."""
    w = gpu_workers(curve)
    plan = plan_str(log_n, max_log_r)
    assert len(plan_widths(log_n, max_log_r)) >= 3
    with plane_budget([w], (1 << log_n) * 32, max_log_r):
        for inv, coset in MODES:
            w.trim()
            for i, v in enumerate(inputs(oracle, cid, log_n)):
                where = f"{curve} 2^{log_n} plan {plan} input {i} inv={inv} coset={coset}"
                got = routed(w, lambda: w.ntt(v, inv, coset), (1 if i == 0 else 0, 0, 0), where)
                assert np.array_equal(got, want_ntt(oracle, cid, log_n, i, inv, coset)), where


# ---------------------------------------------------------------------------------------------- d. the distributed passes
@contextlib.contextmanager
def in_process_workers(gpu_workers, curve, S):
    from distributed_plonk_amd.worker import PlonkWorker
    extra = [PlonkWorker(me=i, device=0, curve=curve) for i in range(1, S)]
    try:
        yield [gpu_workers(curve)] + extra
    finally:
        for w in extra:
            w.close()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r", [9, 3])
@pytest.mark.parametrize("S", [1, 2])
def test_budget_zero_distributed_transform(gpu_workers, oracle, curve, cid, S, max_log_r):
    """Dispatcher.fft like the reference's test_fft (domains 2^11 and 2^13, all four modes) with every in-process worker on budget 0: the row
    pass's output factor w_N^(+-(q + q0) k) comes from two_level(P.epi, ...) instead of the output-factor plane, which also keeps the per-row
    coset constant (and with it the whole coset shift) in the prologue.  ntt_max_log_r = 3 makes the 2^5 ... 2^7-point rows and columns
    multi-pass (3+2, 3+3, 3+2+2), so the contiguous row pass and the interleaved column pass form their inter-pass factors on the fly too."""
    with in_process_workers(gpu_workers, curve, S) as workers:
        with plane_budget(workers, 0, max_log_r):
            d = Dispatcher(workers)
            d.init(None, 1 << 11, 1 << 13)
            for is_quot in (False, True):
                N = d.quot_domain_size if is_quot else d.domain_size
                coeffs = oracle.rand_fr(cid, 31 + is_quot, N)
                for is_inv, is_coset in MODES:
                    where = f"{curve} S={S} ntt_max_log_r={max_log_r} quot={is_quot} inv={is_inv} coset={is_coset}"
                    got = routed(workers[0], lambda: d.fft(coeffs, is_quot, is_inv, is_coset), NONE, where)
                    assert np.array_equal(got, oracle.ntt(cid, coeffs, is_inv, is_coset, threads=4)), where


@pytest.mark.parametrize("max_log_r", [9, 3])
def test_budget_zero_per_step_parity_fft1_exchange_fft2(gpu_workers, oracle, max_log_r):
    """The steps of test_gpu_distributed.py's per-step parity — fft1 rows, the exchange, fft2 columns, against fft1_helper / the pack and scatter
    maps / fft2_helper — on two workers under budget 0, with single-pass (2^5 / 2^4) and forced two-pass (3+2 / 2+2) rows and columns."""
    S, log_n, cid = 2, 9, 0
    N = 1 << log_n
    r, c = split_rc(N)
    wl = make_fft_workloads(N, S)
    coeffs = oracle.rand_fr(cid, 99, N)
    rows = coeffs.reshape(c, r, 4).transpose(1, 0, 2).copy()
    with in_process_workers(gpu_workers, "bn254", S) as ws:
        with plane_budget(ws, 0, max_log_r):
            d = Dispatcher(ws)
            d.init(None, N, 0)
            for is_inv, is_coset in MODES:
                o_rows = np.stack([oracle.fft1_helper(cid, rows[b], b, log_n, is_inv, is_coset) for b in range(r)])
                o_cols = [np.zeros((wl[s].num_cols(), r, 4), dtype=np.uint64) for s in range(S)]
                for src in range(S):
                    for dst in range(S):
                        blk = oracle.exchange_pack(np.ascontiguousarray(o_rows[wl[src].row_start:wl[src].row_end]), wl[dst].col_start, wl[dst].col_end)
                        oracle.exchange_scatter(o_cols[dst], wl[src].row_start, blk)
                want = [np.stack([oracle.fft2_helper(cid, o_cols[s][i], i + wl[s].col_start, log_n, is_inv, is_coset)
                                  for i in range(wl[s].num_cols())]) for s in range(S)]

                def device_steps():
                    id = 4321 + 2 * is_inv + is_coset
                    for w in ws:
                        w.fft_init(id, wl, False, is_inv, is_coset)
                    for s, w in enumerate(ws):
                        for j in range(wl[s].num_rows()):
                            w.fft1(id, j, rows[wl[s].row_start + j])
                    d._fft2_prepare_all(id)
                    return [w.fft2(id, r) for w in ws]

                where = f"ntt_max_log_r={max_log_r} inv={is_inv} coset={is_coset}"
                got = routed(ws[0], device_steps, NONE, where)
                for s in range(S):
                    assert np.array_equal(got[s], want[s]), f"rank {s} {where}"


# ---------------------------------------------------------------------------------------------- e. the shared-input transforms
def class_shape(log_size, length, max_log_r):
    """(classes, passes per class transform) by the rule test_gpu_coset_classes.py restates from coset_eval_run"""
    classes, plan = _class_plan(log_size, length, max_log_r).split(" x ")
    return int(classes), plan.count("+") + 1


def eval_case(oracle, cid, log_size, length, seed):
    """A coefficient vector, the shifts A = g and B = g * w_(2 size), and its evaluations on A * <w_size> and B * <w_size>: the stride-2
    slices of the oracle's coset FFT over 2 * size points (as in test_class_evaluations_are_slices_of_the_coset_fft)"""
    size = 1 << log_size
    assert length <= 2 * size
    P, f, g, w2 = _consts(oracle, cid, log_size + 1)
    poly = oracle.rand_fr(cid, seed, length)
    padded = np.zeros((2 * size, 4), dtype=np.uint64)
    padded[:length] = poly
    big = oracle.ntt(cid, padded, False, True, threads=8)
    return poly, [P.fr_to_limbs(f, g), P.fr_to_limbs(f, g * w2 % f.p)], [big[0::2], big[1::2]]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("log_size,length", [(9, 70), (12, (1 << 9) + 3), (6, 100)])
def test_budget_zero_coset_eval_with_single_pass_classes(gpu_workers, oracle, curve, cid, log_size, length):
    """plonk_coset_eval_dev whose class transforms are single-pass (8 classes of 2^6 and of 2^9 points, one class of 2^6 with a fold): the shift
    set has row tables and fold constants but no plane, counts 0 bytes and fits budget 0.  Plain (shift 1) and coset (shift g), no generator
    launch, exact."""
    w = gpu_workers(curve)
    size = 1 << log_size
    classes, passes = class_shape(log_size, length, 9)
    assert passes == 1
    P, f, g, _ = _consts(oracle, cid, log_size)
    poly = oracle.rand_fr(cid, 5200 + log_size, length)
    dp, out = w.alloc(length * 32).upload(poly), w.alloc(size * 32)
    try:
        with plane_budget([w], 0):
            for shift, coset in ((1, False), (g, True)):
                where = f"{curve} coset_eval 2^{log_size} <- {length} ({classes} classes) shift {'g' if coset else '1'}"
                want = oracle.ntt(cid, _folded(P, f, shift, poly, size), False, coset, threads=8)

                def run():
                    w.coset_eval_dev(dp.ptr, length, size, P.fr_to_limbs(f, shift), out.ptr)
                    return out.download((size, 4))

                assert np.array_equal(routed(w, run, NONE, where), want), where
    finally:
        dp.free(); out.free()


def compact_rows(oracle, cid, log_N, S):
    """the zero-padded vector of test_zero_padded_row_pass_matches_oracle (N / 8 + 3 coefficients), its decimated rows and workloads"""
    N = 1 << log_N
    length = N // 8 + 3
    r, c = split_rc(N)
    row_len = min(c, (length + r - 1) // r)
    v = np.zeros((N, 4), dtype=np.uint64)
    v[:length] = oracle.rand_fr(cid, 8100 + log_N, length)
    t = np.ascontiguousarray(v.reshape(c, r, 4).transpose(1, 0, 2))
    assert not t[:, row_len:].any()
    return v, t, row_len, r, c, make_fft_workloads(N, S)


def compact_fft1(workers, id, wl, t, row_len, is_coset):
    keep = []
    for s, w in enumerate(workers):
        w.fft_init(id, wl, False, False, is_coset)
        rows = np.ascontiguousarray(t[wl[s].row_start:wl[s].row_end, :row_len])
        keep.append(w.alloc(rows.nbytes).upload(rows))
        w.fft1_dev_compact(id, keep[-1].ptr, row_len)
    return keep


def compact_fft2(workers, id, wl, r, c):
    u = np.empty((c, r, 4), dtype=np.uint64)
    for s, w in enumerate(workers):
        u[wl[s].col_start:wl[s].col_end] = w.fft2(id, r)
    return np.ascontiguousarray(u.transpose(1, 0, 2)).reshape(-1, 4)


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("S", [1, 2])
def test_compact_row_pass_without_and_with_room_for_its_output_factor_plane(gpu_workers, oracle, curve, cid, S):
    """plonk_fft1_dev_compact at 2^11 (r = 32, c = 64: 9 leading coefficients per row, 8 single-pass classes of 8 points, so the shift set
    counts 0 bytes).  Its row pass runs inside plonk_fft2_prepare and ALWAYS carries the row twiddle w_N^(b k'), which the shared-input mode
    takes from the output-factor plane only: under budget 0 the prepare step fails with PLONK_ERR_HIP, "no room for the output-factor plane",
    plain and coset — a successful compact row pass without that plane does not exist at any size, so the other outcome is pinned with the
    budget set to exactly that plane's bytes (c * rows-of-the-worker * 32): one ntt_gen_epi_plane launch per worker, no other plane, exact.
    The refused task is not lost: with room for the plane the same prepare call goes through and the transform is exact."""
    log_N = 11
    v, t, row_len, r, c, wl = compact_rows(oracle, cid, log_N, S)
    assert class_shape(log_N - (log_N >> 1), row_len, 9) == (8, 1)
    epi_bytes = c * (r // S) * 32
    with in_process_workers(gpu_workers, curve, S) as workers:
        d = Dispatcher(workers)
        d.init(None, 1 << log_N, 0)
        for is_coset in (False, True):
            want = oracle.ntt(cid, v, False, is_coset, threads=8)
            where = f"{curve} S={S} coset={is_coset}"
            keep = []
            try:
                with plane_budget(workers, 0):
                    keep += compact_fft1(workers, 600 + is_coset, wl, t, row_len, is_coset)
                    workers[0].profile_reset()
                    with pytest.raises(PlonkError) as e:
                        d._fft2_prepare_all(600 + is_coset)
                    assert launches(workers[0]) == NONE, where
                    assert e.value.code == ERR_HIP and "no room for the output-factor plane" in str(e.value), f"{where}: {e.value}"
                    for w in workers:
                        w.set_option("ntt_plane_budget", epi_bytes)
                    routed(workers[0], lambda: d._fft2_prepare_all(600 + is_coset), (0, S, 0), where + " (the refused task, with room)")
                    assert np.array_equal(compact_fft2(workers, 600 + is_coset, wl, r, c), want), where + " (the refused task, with room)"
                with plane_budget(workers, epi_bytes):
                    def run():
                        keep.extend(compact_fft1(workers, 610 + is_coset, wl, t, row_len, is_coset))
                        d._fft2_prepare_all(610 + is_coset)
                        return compact_fft2(workers, 610 + is_coset, wl, r, c)
                    assert np.array_equal(routed(workers[0], run, (0, S, 0), where), want), where
            finally:
                for b in keep:
                    b.free()


# (ntt_max_log_r, log size, coefficients) of coset evaluations with multi-pass classes: 8 x 2+2, 16 x 3+3+3 / 8 x 2+2, 8 x 3+2+2, 8 x 5+5.  A class
# transform of three passes takes the planes of its passes 1 ... from get_plane like a whole-vector transform (and forms those factors on the fly
# when they do not fit); only its pass-0 planes belong to the shift set.
REFUSED = [(3, 7, 19), (3, 13, 5)]
EVICTING = [(3, 7, 19), (3, 10, 131), (9, 13, (1 << 10) + 3)]


def class_later_planes(log_size, length, max_log_r, room):
    """how many planes of passes 1 ... passes - 2 of the class transform fit into `room` bytes (they are asked for in pass order)"""
    classes, _ = class_shape(log_size, length, max_log_r)
    widths = plan_widths(log_size - (classes.bit_length() - 1), max_log_r)
    r_prev, count = (1 << log_size) // classes >> widths[0], 0
    for width in widths[1:-1]:
        if r_prev * 32 <= room:
            room -= r_prev * 32
            count += 1
        r_prev >>= width
    return count


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_size,length", REFUSED, ids=[f"n{c[1]}r{c[0]}" for c in REFUSED])
def test_budget_zero_coset_eval_with_multi_pass_classes_is_refused(gpu_workers, oracle, curve, cid, max_log_r, log_size, length):
    """Multi-pass class transforms need their first-pass planes and there is no plane-less form: PLONK_ERR_HIP, "plane budget".  The context
    survives (a whole-vector transform right after is exact, plane-less), and with the default budget back the same call succeeds."""
    w = gpu_workers(curve)
    size = 1 << log_size
    classes, passes = class_shape(log_size, length, max_log_r)
    assert passes >= 2
    poly, shifts, wants = eval_case(oracle, cid, log_size, length, 5300 + log_size)
    dp, out = w.alloc(length * 32).upload(poly), w.alloc(size * 32)
    where = f"{curve} coset_eval 2^{log_size} <- {length}: {_class_plan(log_size, length, max_log_r)}"

    def run():
        w.coset_eval_dev(dp.ptr, length, size, shifts[0], out.ptr)
        return out.download((size, 4))

    try:
        with plane_budget([w], 0, max_log_r):
            w.profile_reset()
            with pytest.raises(PlonkError) as e:
                run()
            assert launches(w) == NONE, where
            assert e.value.code == ERR_HIP and "plane budget" in str(e.value), f"{where}: {e.value}"
            log_n = 9
            got = routed(w, lambda: w.ntt(inputs(oracle, cid, log_n)[0], False, True), NONE, where + ": whole-vector transform after the refusal")
            assert np.array_equal(got, want_ntt(oracle, cid, log_n, 0, False, True)), where + ": whole-vector transform after the refusal"
            w.set_option("ntt_plane_budget", -1)
            assert np.array_equal(routed(w, run, (passes - 2, 0, classes), where + " with the default budget"), wants[0]), where + " with the default budget"
    finally:
        dp.free(); out.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_size,length", EVICTING, ids=[f"n{c[1]}r{c[0]}" for c in EVICTING])
def test_shift_sets_evict_each_other_and_the_bytes_are_given_back_once(gpu_workers, oracle, curve, cid, max_log_r, log_size, length):
    """Budget = one shift set's planes (classes * 2^log_class * 32 = size * 32).  Coset A builds its set (one ntt_gen_shift_plane launch per
    class); coset B of the same size does not fit beside it, so A's set is dropped after a stream sync and B's built; A again: built AGAIN (a
    set served from the dropped entry would launch nothing), each result exact.  The 3+2+2 classes find no room for their pass-1 plane beside
    the set and form that pass's factors on the fly: a mixed plan in shared-input mode.  Then the budget grows by the planes of a whole-vector plain
    transform: they fit exactly if plane_bytes is one set's bytes now — evicted bytes subtracted once per eviction, not zero times (nothing
    would fit) and not twice (the unsigned count would wrap).  After a trim the same set and the same planes fit again."""
    w = gpu_workers(curve)
    size = 1 << log_size
    classes, passes = class_shape(log_size, length, max_log_r)
    assert passes >= 2
    set_bytes = size * 32
    poly, shifts, wants = eval_case(oracle, cid, log_size, length, 5400 + log_size)
    dp, out = w.alloc(length * 32).upload(poly), w.alloc(size * 32)
    NP = len(plan_widths(log_size, max_log_r))
    assert NP >= 2
    where = f"{curve} coset_eval 2^{log_size} <- {length}: {_class_plan(log_size, length, max_log_r)}"

    def run(which):
        w.coset_eval_dev(dp.ptr, length, size, shifts[which], out.ptr)
        return out.download((size, 4))

    try:
        with plane_budget([w], set_bytes, max_log_r):
            for step, which in enumerate((0, 1, 0)):
                got = routed(w, lambda: run(which), (0, 0, classes), f"{where} step {step} (coset {'AB'[which]})")
                assert np.array_equal(got, wants[which]), f"{where} step {step} (coset {'AB'[which]})"
            got = routed(w, lambda: run(0), NONE, where + ": coset A again, cached")
            assert np.array_equal(got, wants[0]), where + ": coset A again, cached"
            for again in (False, True):
                if again:
                    w.trim()
                    w.set_option("ntt_plane_budget", set_bytes)
                    got = routed(w, lambda: run(1), (0, 0, classes), where + ": after trim")
                    assert np.array_equal(got, wants[1]), where + ": after trim"
                w.set_option("ntt_plane_budget", set_bytes + plain_plane_bytes(log_size, max_log_r))
                v = inputs(oracle, cid, log_size)[0]
                got = routed(w, lambda: w.ntt(v, False, False), (NP - 1, 0, 0), f"{where}: whole-vector planes beside the resident set (after trim: {again})")
                assert np.array_equal(got, want_ntt(oracle, cid, log_size, 0, False, False)), where
    finally:
        dp.free(); out.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_size,length", EVICTING, ids=[f"n{c[1]}r{c[0]}" for c in EVICTING])
def test_coset_eval_is_refused_while_whole_vector_planes_hold_the_budget(gpu_workers, oracle, curve, cid, max_log_r, log_size, length):
    """The budget is filled by the planes of a plain whole-vector transform of the same size (at least size * 32 bytes: a shift set would fit an
    empty budget).  Shared-input transforms may only drop other shift sets, and there is none: "plane budget", nothing generated.  After a trim
    the same call under the same budget succeeds."""
    w = gpu_workers(curve)
    size = 1 << log_size
    classes, passes = class_shape(log_size, length, max_log_r)
    assert passes >= 2
    NP = len(plan_widths(log_size, max_log_r))
    budget = plain_plane_bytes(log_size, max_log_r)
    assert NP >= 2 and budget >= size * 32
    poly, shifts, wants = eval_case(oracle, cid, log_size, length, 5500 + log_size)
    dp, out = w.alloc(length * 32).upload(poly), w.alloc(size * 32)
    where = f"{curve} coset_eval 2^{log_size} <- {length}: {_class_plan(log_size, length, max_log_r)}"

    def run():
        w.coset_eval_dev(dp.ptr, length, size, shifts[0], out.ptr)
        return out.download((size, 4))

    try:
        with plane_budget([w], budget, max_log_r):
            v = inputs(oracle, cid, log_size)[0]
            got = routed(w, lambda: w.ntt(v, False, False), (NP - 1, 0, 0), where + ": filling the budget")
            assert np.array_equal(got, want_ntt(oracle, cid, log_size, 0, False, False)), where
            w.profile_reset()
            with pytest.raises(PlonkError) as e:
                run()
            assert launches(w) == NONE, where
            assert e.value.code == ERR_HIP and "plane budget" in str(e.value), f"{where}: {e.value}"
            w.trim()
            later = class_later_planes(log_size, length, max_log_r, budget - size * 32)
            assert np.array_equal(routed(w, run, (later, 0, classes), where + " after trim"), wants[0]), where + " after trim"
    finally:
        dp.free(); out.free()


# ---------------------------------------------------------------------------------------------- f. trim resets the accounting
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", PLAIN_CACHED, ids=[case_id(*c) for c in PLAIN_CACHED])
def test_trim_resets_the_plane_accounting(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """Budget = the plain forward planes, exactly.  The transform builds them, plonk_trim frees them, and the same transform builds them again:
    with plane_bytes left at its old value nothing would fit (0 launches).  A third run finds them cached."""
    w = gpu_workers(curve)
    NP, plan = len(plan_widths(log_n, max_log_r)), plan_str(log_n, max_log_r)
    assert NP >= 2
    v, want = inputs(oracle, cid, log_n)[0], want_ntt(oracle, cid, log_n, 0, False, False)
    with plane_budget([w], plain_plane_bytes(log_n, max_log_r), max_log_r):
        for step, count in (("first", NP - 1), ("after trim", NP - 1), ("cached", 0)):
            if step == "after trim":
                w.trim()
            got = routed(w, lambda: w.ntt(v, False, False), (count, 0, 0), f"{curve} plan {plan} {step}")
            assert np.array_equal(got, want), f"{curve} plan {plan} {step}"


# ---------------------------------------------------------------------------------------------- g. the option itself
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("max_log_r,log_n", [(3, 9), (9, 13)], ids=[case_id(3, 9), case_id(9, 13)])
def test_negative_budget_restores_the_default_and_the_option_is_per_context(gpu_workers, oracle, curve, cid, max_log_r, log_n):
    """Under budget 0 the coset transform generates nothing; after ntt_plane_budget = -1 the same transform generates its passes - 1 planes (the
    default route: the shift folded into the pass-0 plane).  The budget belongs to the context it was set on: a second worker on the same
    device keeps generating planes while the first runs plane-less.  Budgets take effect at the next transform and free nothing: back on budget
    0, the planes cached under the default still serve (0 launches; a plain transform, whose pass-0 plane is not among them, gets none)."""
    from distributed_plonk_amd.worker import PlonkWorker
    w = gpu_workers(curve)
    NP, plan = len(plan_widths(log_n, max_log_r)), plan_str(log_n, max_log_r)
    assert NP >= 2
    v = inputs(oracle, cid, log_n)[0]
    want, want_plain = want_ntt(oracle, cid, log_n, 0, False, True), want_ntt(oracle, cid, log_n, 0, False, False)
    other = PlonkWorker(me=0, device=0, curve=curve)
    try:
        with plane_budget([w, other], 0, max_log_r):
            other.set_option("ntt_plane_budget", -1)
            for step, (who, count) in enumerate(((w, 0), (other, NP - 1), (w, 0), (other, 0))):
                got = routed(w, lambda: who.ntt(v, False, True), (count, 0, 0), f"{curve} plan {plan} step {step}")
                assert np.array_equal(got, want), f"{curve} plan {plan} step {step}"
            w.set_option("ntt_plane_budget", -1)
            assert np.array_equal(routed(w, lambda: w.ntt(v, False, True), (NP - 1, 0, 0), f"{curve} plan {plan} after -1"), want)
            w.set_option("ntt_plane_budget", 0)
            assert np.array_equal(routed(w, lambda: w.ntt(v, False, True), NONE, f"{curve} plan {plan} budget 0 over cached planes"), want)
            assert np.array_equal(routed(w, lambda: w.ntt(v, False, False), NONE, f"{curve} plan {plan} budget 0, plain"), want_plain)
    finally:
        other.close()
