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

    python tools/solve_probe.py --replay 16 [--height 32] [--members 50] [--fuse-widths 0 64 256 1024] [--reps 5]

--replay K runs another measurement instead: K witnesses of membership.membership_circuit(curve, height, members) over one accumulator,
their inputs gathered on the device.  K sequential solve_dev calls against one plonk_circuit_schedule_dev and one solve_many_dev per fuse
width (plonk_circuit_replay_dev), and K preprocess calls against one setup() and K instances: host clock around work that ends in a
synchronise, the variants alternating within a repetition, median (min .. max) of at least 5 repetitions after a warm-up that also
compares the replayed witness with the solved one (profiles/solve_replay.txt).
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


def replay_probe(w: PlonkWorker, height: int, m: int, K: int, reps: int, widths) -> dict:
    """K witnesses of membership_circuit(curve, height, m) over one accumulator, host clock around work that ends in a synchronise, the variants
    alternating within each repetition: K x solve_dev against schedule + solve_many_dev per fuse width, K x preprocess against setup + K instances."""
    import numpy as np
    from distributed_plonk_amd import rescue as RS
    from distributed_plonk_amd.membership import membership_circuit
    built = membership_circuit(w.curve_name, height, m)
    n, rows, count = built.n, 2 + 4 * height, m * K
    d_el = w.alloc(count * 32)
    w.synth_fr(height, d_el.ptr, count)
    acc = RS.Accumulator(w, RS.RescueParams.default(w.curve_name), d_el.download((count, 4)), height)
    d_el.free()
    roots = np.ascontiguousarray(np.broadcast_to(acc.root.reshape(1, 1, 4), (K, 1, 4)))
    d_all = w.alloc(K * rows * m * 32)
    for b in range(K):
        buf = acc.witness_inputs_dev(range(b * m, (b + 1) * m))
        w.memcpy_d2d(d_all.ptr + b * rows * m * 32, buf.ptr, rows * m * 32)
        buf.free()
    at = lambda b: d_all.ptr + b * rows * m * 32
    times = {}

    def timed(name, fn):
        w.sync()
        t0 = time.perf_counter()
        out = fn()
        w.sync()
        times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def solve_each(keep_last):
        last = None
        for b in range(K):
            s = built.solve_dev(w, public_inputs=roots[b], d_inputs=at(b))
            if keep_last and b == K - 1:
                last = s.witness()
            s.close()
        return last

    def record():
        d_vars, d_sel, d_def, *d_hint = built._upload(w)
        d_order = w.alloc(n * 4)
        try:
            return w.circuit_schedule_dev(d_vars.ptr, n, built.num_vars, d_sel.ptr, d_def.ptr, d_hint[0].ptr if d_hint else 0, d_order.ptr)[1:3]
        finally:
            d_order.free()

    def replay(width):
        batch = built.solve_many_dev(w, public_inputs=roots, d_inputs=d_all.ptr, fuse_width=width)
        w.sync()
        return batch

    def preprocess_each():
        for b in range(K):
            built.preprocess(w, public_inputs=roots[b], d_inputs=at(b)).close()

    def setup_and_instances():
        key = built.setup(w)
        batch = built.solve_many_dev(w, public_inputs=roots, d_inputs=d_all.ptr)
        for inst in key.instances(batch):
            inst.close()
        batch.close()
        key.close()

    try:
        built.schedule(w)
        levels = evaluations = 0
        for rep in range(reps + 1):
            want = timed("solve_dev x K", lambda: solve_each(rep == 0))            # the warm-up also compares the results
            levels, evaluations = timed("schedule", record)
            for width in widths:
                batch = timed(f"solve_many_dev fuse_width={width}", lambda: replay(width))
                if want is not None:
                    assert np.array_equal(batch.witness(K - 1), want), f"fuse_width {width}: the replayed witness differs from the solved one"
                batch.close()
            timed("preprocess x K", preprocess_each)
            timed("setup + solve_many_dev + K instances", setup_and_instances)
    finally:
        d_all.free()
        acc.close()
        built.close()
        w.trim()
    stat ={k: dict(median=round(statistics.median(v[1:]), 3), min=round(min(v[1:]), 3), max=round(max(v[1:]), 3)) for k, v in times.items()}
    return dict(curve=w.curve_name, height=height, m=m, K=K, n=n, num_vars=built.num_vars, levels=levels, evaluations=evaluations, reps=reps, ms=stat)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replay", type=int, default=0, metavar="K", help="time K witnesses of the membership circuit: solve_dev x K against schedule + solve_many_dev")
    ap.add_argument("--height", type=int, default=32)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--fuse-widths", type=int, nargs="+", default=[0, 64, 256, 1024])
    ap.add_argument("--log-n", type=int, nargs="+", default=[22, 24])
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--hints", choices=["inv", "root5", "bits"], default=None)
    a = ap.parse_args()
    w = PlonkWorker(me=0, device=0, curve=a.curve)
    try:
        if a.replay:
            r = replay_probe(w, a.height, a.members, a.replay, max(a.reps, 5), a.fuse_widths)
            print(f"membership_circuit({a.curve}, {a.height}, {a.members}): n = {r['n']}, {r['levels']} levels, {r['evaluations']} evaluations; K = {a.replay} witnesses, "
                  f"median (min .. max) of {r['reps']} repetitions after a warm-up, ms")
            for name, s in r["ms"].items():
                print(f"  {name:40s} {s['median']:10.3f}  ({s['min']:.3f} .. {s['max']:.3f})")
            print(json.dumps(r), flush=True)
            return
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
