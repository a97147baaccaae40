"""The NTT planner restated for the tests that force plans with option ntt_max_log_r (tests/test_gpu_ntt.py, tests/test_gpu_coset_classes.py):
one statement of ntt_plan_widths (csrc/ntt_engine.hip) for assertion messages and case lists, and the list of forced plans itself."""


def plan_widths(log_m, max_log_r):
    """The pass widths of a 2^log_m-point transform when no pass may be wider than max_log_r (clamped to 3..9): as few passes as
    possible, as even as possible, the wider ones first."""
    mx = max(3, min(max_log_r, 9))
    if log_m <= mx:
        return [log_m]
    passes = -(-log_m // mx)
    base, rem = divmod(log_m, passes)
    return [base + (1 if i < rem else 0) for i in range(passes)]


def plan_str(log_m, max_log_r):
    return "+".join(str(w) for w in plan_widths(log_m, max_log_r))


# (ntt_max_log_r, log size): each width 2 ... 7 as a first, a middle and a last pass of a three-pass plan (2 as a first pass exists only in
# 2+2: the first pass is the widest and the option is clamped to 3), and four-pass plans (NTT_MAX_PASSES)
FORCED_PLANS = [(3, L) for L in range(4, 13)] + [(4, L) for L in (9, 10, 12, 13, 16)] + [(5, L) for L in (11, 13, 15, 16, 20)] + \
               [(6, L) for L in (13, 16, 18)] + [(7, L) for L in (15, 19, 21)]
