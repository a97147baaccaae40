"""Per-stage time of user-circuit preprocessing on one GPU (distributed_plonk_amd/circuit.py).

    python tools/preprocess_timing.py [--log-n 20 24] [--curve bn254] [--reps 3]

A random wiring (half the positions on one padding variable, the rest uniform over n variables) and random witness / selectors; the
circuit is not satisfied, which the stages timed here do not care about.  Stages: sort + link and the id_perm / sigma writer (HIP events
recorded by the library around their launches: plonk_profile_*), witness placement and the check (the same events; both end in a
synchronise), the 18 n-point iNTTs and the 18 verifying-key commitments (host clock around work that ends in a synchronise).
The first repetition is a warm-up and is not reported; the table gives the median of the others in milliseconds.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd.circuit import default_k  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

STAGES = ["sort+link", "sigma+id_perm", "witness", "check", "intt x18", "commit x18"]


def one_size(w: PlonkWorker, log_n: int, reps: int) -> dict:
    n = 1 << log_n
    f = _fr.FIELDS[w.curve_name]
    rs = np.random.RandomState(log_n)
    wv = rs.randint(1, n, size=5 * n, dtype=np.uint32)
    wv[rs.permutation(5 * n)[: 5 * n // 2]] = 0
    num_vars = n
    bufs = []
    alloc = lambda nbytes: bufs.append(w.alloc(nbytes)) or bufs[-1]
    d_vars = alloc(wv.nbytes).upload(wv)
    d_wit, d_sel, d_pi = alloc(num_vars * 32), alloc(13 * n * 32), alloc(n * 32)
    w.synth_fr(1, d_wit.ptr, num_vars)
    w.synth_fr(2, d_sel.ptr, 13 * n)
    w.memset_dev(d_pi.ptr, 0, n * 32)
    d_id, d_idx, d_sig, d_wires = alloc(5 * n * 32), alloc(5 * n * 8), alloc(5 * n * 32), alloc(5 * n * 32)
    d_coef, tmp = alloc(18 * n * 32), alloc(n * 32)
    # commit key: n + 3 synthetic points padded to a multiple of 32 (the vk commitments need bases, not a trapdoor)
    key = ((n + 3 + 31) >> 5) << 5
    d_ck = alloc(key * (64 if w.curve_name == "bn254" else 96))
    w.synth_bases(3, 1 << 12, key, d_ck.ptr)
    w.init_dev(d_ck.ptr, key, n, 8 * n)
    k = default_k(w.curve_name)
    times = {s: [] for s in STAGES}
    try:
        for rep in range(reps + 1):
            w.sync()
            w.profile_reset()
            w.profile_enable(True)
            w.circuit_permutation_dev(d_vars.ptr, n, num_vars, k, d_id.ptr, d_idx.ptr, d_sig.ptr)
            w.circuit_witness_dev(d_vars.ptr, n, d_wit.ptr, num_vars, d_wires.ptr)
            w.circuit_check_dev(d_wires.ptr, d_sel.ptr, d_pi.ptr, d_idx.ptr, n)
            w.sync()
            prof = {name: w.profile_get(name)[0] for name in ("circuit_sort", "circuit_sigma", "circuit_witness", "circuit_check")}
            w.profile_enable(False)
            t0 = time.perf_counter()
            for t, src in enumerate([d_sel.ptr + i * n * 32 for i in range(13)] + [d_sig.ptr + i * n * 32 for i in range(5)]):
                w.memcpy_d2d_async(tmp.ptr, src, n * 32)
                w.ntt_dev(tmp.ptr, d_coef.ptr + t * n * 32, n, True, False)
            w.sync()
            t1 = time.perf_counter()
            w.commit_many_dev([(d_coef.ptr + t * n * 32, n) for t in range(18)])
            w.sync()
            t2 = time.perf_counter()
            if rep == 0:
                continue
            for s, v in zip(STAGES, [prof["circuit_sort"], prof["circuit_sigma"], prof["circuit_witness"], prof["circuit_check"],
                                     (t1 - t0) * 1e3, (t2 - t1) * 1e3]):
                times[s].append(v)
    finally:
        for b in bufs:
            b.free()
        w.trim()
    return {s: statistics.median(v) for s, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    w = PlonkWorker(me=0, device=0, curve=a.curve)
    try:
        for log_n in a.log_n:
            res = one_size(w, log_n, a.reps)
            print(f"2^{log_n} gates, {a.curve}: " + ", ".join(f"{s} {v:.2f} ms" for s, v in res.items()), flush=True)
            print(json.dumps({"log_n": log_n, "curve": a.curve, "ms": {s: round(v, 3) for s, v in res.items()}}), flush=True)
    finally:
        w.close()


if __name__ == "__main__":
    main()
