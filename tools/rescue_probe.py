"""Rate of the Rescue kernels (csrc/rescue_kernels.hpp, csrc/rescue_acc_kernels.hpp) on one GPU.

    python tools/rescue_probe.py [--log 20] [--curve bn254 bls12_381] [--reps 7] [--out profiles/rescue_probe.txt]

Times 2^log permutations (plonk_rescue_permute_dev, one launch) and a tree over 2^log leaves (plonk_rescue_merkle_dev, `log` launches,
2^log - 1 hashes) from the HIP events the library records around its own launches (plonk_profile_*: "rescue_permute", "rescue_merkle").
The accumulator leg times plonk_rescue_acc_build_dev ("rescue_acc_build") at 2^log elems and height 32 — one permutation per node, the
launches counted as (levels with more than one node) + 2 — and the reference's own case, 50 elems at height 32: 104 permutations of which
the last 28 are ONE lane's chain in one launch, so that build is bounded by one lane's permutation latency, reported as us per chain link.
Inputs are generated on the device from a seed.  One warm-up run of each (it loads the code object and uploads the parameters), then
`reps` timed runs: the median, the smallest and the largest, in milliseconds, and from the median the permutations per second and the
implied field products per second at 12 x (4 x 335 + 12 + 32) = 16608 products per permutation (335: solve_hints.hpp's own count of
products per fixed-exponent power, 329 to 340 depending on field and exponent).  There is no threshold: the figures are context.  A run
without a GPU fails; it prints no number."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import rescue as RS  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

PRODUCTS = 12 * (4 * 335 + 12 + 32)
ACC_HEIGHT = 32


def timed(w: PlonkWorker, name: str, call, reps: int) -> list:
    out = []
    for rep in range(reps + 1):
        w.sync()
        w.profile_reset()
        w.profile_enable(True)
        call()
        w.sync()
        ms = w.profile_get(name)[0]
        w.profile_enable(False)
        if rep:
            out.append(ms)
    return out


def line(what: str, perms: int, ms: list) -> str:
    med = statistics.median(ms)
    rate = perms / (med * 1e-3)
    return (f"  {what}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs after 1 warm-up)  ->  {rate / 1e6:.2f} M permutations/s, "
            f"{rate * PRODUCTS / 1e9:.1f} G field products/s implied")


def probe(curve: str, log: int, reps: int) -> list:
    w = PlonkWorker(me=0, device=0, curve=curve)
    prm = RS.RescueParams.default(curve)
    count = 1 << log
    lines = [f"{curve}, {PRODUCTS} products per permutation:"]
    try:
        buf = w.alloc(4 * count * 32)                  # 4 * count Fr: `count` states, or a tree of 2 * count - 1 nodes
        try:
            w.synth_fr(1, buf.ptr, 4 * count)
            lines.append(line(f"2^{log} permutations, one launch", count, timed(w, "rescue_permute", lambda: RS.permute_dev(w, prm, buf.ptr, count), reps)))
            lines.append(line("1 permutation, one launch: one lane's latency", 1, timed(w, "rescue_permute", lambda: RS.permute_dev(w, prm, buf.ptr, 1), reps)))
            lines.append(line(f"tree over 2^{log} leaves, {log} launches, {count - 1} hashes", count - 1,
                              timed(w, "rescue_merkle", lambda: RS.merkle_dev(w, prm, buf.ptr, log), reps)))
            for n_elems in (count, 50):
                counts = RS.acc_level_counts(ACC_HEIGHT, n_elems)
                nodes, wide = sum(counts), sum(c > 1 for c in counts)
                ms = timed(w, "rescue_acc_build", lambda: RS.acc_build_dev(w, prm, buf.ptr, n_elems, ACC_HEIGHT, buf.offset(count * 32)), reps)
                med = statistics.median(ms)
                chain = counts.count(1) - 1
                lines.append(line(f"accumulator of {n_elems} elems, height {ACC_HEIGHT}: {wide + 2} launches, {nodes} permutations, a chain of {chain}", nodes, ms)
                             + f"; {med * 1e6 / nodes:.0f} ns per permutation" + (f", at most {med * 1e3 / chain:.0f} us per chain link" if n_elems == 50 else ""))
        finally:
            buf.free()
    finally:
        w.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--curve", nargs="+", default=["bn254", "bls12_381"], choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = [f"tools/rescue_probe.py --log {a.log} --reps {a.reps}: HIP events around the library's own launches, one MI355X"]
    for curve in a.curve:
        lines += probe(curve, a.log, a.reps)
        print("\n".join(lines[-6:]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
