"""Time of the device witness solver (plonk_circuit_solve_dev) on one GPU, beside one pass of the satisfiability check.

    python tools/solve_probe.py [--log-n 22 24] [--curve bn254] [--reps 3] [--depth 64] [--hints {inv,root5,bits}]

The circuit: (2^log_n - 2) / depth parallel hash chains of `depth` gates each (two of three rounds x <- x^5 + c y^5 + k, the third
x <- q0 x y + q1 x x), built with `depth` array operations of builder.CircuitBuilder — the full-size case of tests/test_gpu_solve.py.
Reported, from the HIP events the library records around its own launches (plonk_profile_*): the solver's setup (validation, liveness,
sort keys, first frontier), its sort (radix passes + segment heads), its level launches (one per level, with the host's read of the
next frontier size in between) and their sum; the host clock around the whole call; and `circuit_check` on the solved instance — the
existing kernel that evaluates the same gate equation over every gate in one pass, which is the yardstick.  The first repetition is a
warm-up (it also sizes the context's scratch); the others give the median, in milliseconds.

--hints runs the same shape with hinted rounds (plonk_circuit_solve_hints_dev) after the hint-free run of the same size, which is its
yardstick: `inv` and `bits` replace every third round by x <- 1 / x or x <- bit (round mod 254) of x, `root5` alternates x <- x^5 + c y^5 + k
and x <- x^(1/5), Rescue-like.  A level of the hinted chains holds hints only or gates only, so the time of a hint level is what is left
of `levels` after the gate levels at the hint-free run's time per level.  Without --hints the output is what it was.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd.builder import CircuitBuilder  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

PHASES = ["solve_setup", "solve_sort", "solve_levels"]


def hash_chains(curve: str, log_n: int, depth: int, hints=None):
    f = _fr.FIELDS[curve]
    chains = ((1 << log_n) - 2) // depth
    rnd = random.Random(log_n)
    b = CircuitBuilder(curve)
    x, y = b.input(chains), b.input(chains)
    for t in range(depth):
        if hints == "root5" and t % 2 == 1:
            x = b.root5(x)
        elif hints == "inv" and t % 3 == 2:
            x = b.inv(x)
        elif hints == "bits" and t % 3 == 2:
            x = b.bit(x, t % 254)
        elif hints is None and t % 3 == 2:
            x = b.mul_add(x, y, x, x, q0=rnd.randrange(f.p), q1=rnd.randrange(f.p))
        else:
            x = b.pow5_lc([x, y], [1, rnd.randrange(f.p)], const=rnd.randrange(f.p))
    return b.build(), chains


def hint_levels(depth: int, hints: str) -> int:
    return depth // 2 if hints == "root5" else depth // 3


def one_size(w: PlonkWorker, log_n: int, depth: int, reps: int, hints=None) -> dict:
    t0 = time.perf_counter()
    built, chains = hash_chains(w.curve_name, log_n, depth, hints)
    build_s = time.perf_counter() - t0
    n = built.n
    d_in = w.alloc(2 * chains * 32)
    w.synth_fr(log_n, d_in.ptr, 2 * chains)
    inputs = d_in.download((2 * chains, 4))
    d_in.free()
    times = {k: [] for k in PHASES + ["solve_events", "solve_host", "circuit_check"]}
    res = {}
    try:
        for rep in range(reps + 1):
            w.sync()
            w.profile_reset()
            w.profile_enable(True)
            t0 = time.perf_counter()
            s = built.solve_dev(w, inputs)
            host_ms = (time.perf_counter() - t0) * 1e3          # includes the upload of the inputs; the first repetition that of the circuit
            w.sync()
            prof = {k: w.profile_get(k)[0] for k in PHASES}
            d_wires = w.alloc(5 * n * 32)
            try:
                w.circuit_witness_dev(s.d_wire_vars, n, s.d_witness.ptr, built.num_vars, d_wires.ptr)
                bad = w.circuit_check_dev(d_wires.ptr, s.d_selector_evals, s.d_pub.ptr, None, n)
                w.sync()
                check_ms = w.profile_get("circuit_check")[0]
            finally:
                d_wires.free()
                res = dict(levels=s.levels, evaluations=s.evaluations, check=bad)
                s.close()
            w.profile_enable(False)
            if rep == 0:
                continue
            for k in PHASES:
                times[k].append(prof[k])
            times["solve_events"].append(sum(prof.values()))
            times["solve_host"].append(host_ms)
            times["circuit_check"].append(check_ms)
    finally:
        built.close()
        w.trim()
    out = {k: statistics.median(v) for k, v in times.items()}
    return dict(log_n=log_n, curve=w.curve_name, depth=depth, chains=chains, num_vars=built.num_vars, build_s=round(build_s, 2), **res,
                ms={k: round(v, 3) for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log-n", type=int, nargs="+", default=[22, 24])
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--hints", choices=["inv", "root5", "bits"], default=None)
    a = ap.parse_args()
    w = PlonkWorker(me=0, device=0, curve=a.curve)
    try:
        for log_n in a.log_n:
            r = one_size(w, log_n, a.depth, a.reps)
            ms = r["ms"]
            print(f"2^{log_n} gates, {a.curve}, {r['chains']} chains of depth {a.depth}: {r['levels']} levels, {r['evaluations']} evaluations, check {r['check']}")
            print(f"  solver: setup {ms['solve_setup']:.2f} ms, sort {ms['solve_sort']:.2f} ms, levels {ms['solve_levels']:.2f} ms "
                  f"({ms['solve_levels'] / max(r['levels'], 1):.3f} ms per level), sum {ms['solve_events']:.2f} ms; host clock {ms['solve_host']:.2f} ms")
            print(f"  circuit_check, one pass over every gate: {ms['circuit_check']:.2f} ms  ->  solver = {ms['solve_events'] / ms['circuit_check']:.1f} x check, "
                  f"levels alone {ms['solve_levels'] / ms['circuit_check']:.1f} x", flush=True)
            print(json.dumps(r), flush=True)
            if a.hints:
                h = one_size(w, log_n, a.depth, a.reps, a.hints)
                hm, hl = h["ms"], hint_levels(a.depth, a.hints)
                per_gate_level = ms["solve_levels"] / max(r["levels"], 1)
                per_hint_level = (hm["solve_levels"] - (h["levels"] - hl) * per_gate_level) / max(hl, 1)
                print(f"  --hints {a.hints}: {hl} hint levels of {h['chains']} hints among {h['levels']} levels, {h['evaluations']} evaluations, check {h['check']}")
                print(f"  solver: setup {hm['solve_setup']:.2f} ms, sort {hm['solve_sort']:.2f} ms, levels {hm['solve_levels']:.2f} ms, sum {hm['solve_events']:.2f} ms; "
                      f"host clock {hm['solve_host']:.2f} ms")
                print(f"  per hint level {per_hint_level:.3f} ms ({per_hint_level * 1e6 / h['chains']:.1f} ns per hint) against {per_gate_level:.3f} ms per gate level of the "
                      f"hint-free run ({per_gate_level * 1e6 / r['chains']:.1f} ns per gate): {per_hint_level / per_gate_level:.1f} x", flush=True)
                print(json.dumps(dict(hints=a.hints, hint_levels=hl, per_hint_level_ms=round(per_hint_level, 4), per_gate_level_ms=round(per_gate_level, 4), **h)),
                      flush=True)
    finally:
        w.close()


if __name__ == "__main__":
    main()
