"""KZG openings of one polynomial at M points, the many-point route against M rounds of the single-point entry points, on one GPU.

    python tools/kzg_probe.py [--log 20] [--points 1 16 64 256] [--reps 3] [--verify-logs 10 16] [--out profiles/kzg.txt]

On BN254, a random polynomial of 2^log coefficients under a trapdoor key of as many points, for every M:
  many-point   the device time of one plonk_poly_open_many_dev over the M points (plonk_last_kernel_ms) and the wall time of kzg.open_many
               (upload of the points, that call, one plonk_commit_many_dev over the M quotient rows, the read-back), all M rows in one chunk;
  M calls      the same openings from what the library had before: M rounds of plonk_poly_eval_dev and plonk_poly_div_linear_dev with the
               point on the host (a power table and a division table built and uploaded per new point, at most 64 of them cached), then
               the same one plonk_commit_many_dev — wall time of the rounds alone and of the whole.
Times by the host clock around calls that end in a device synchronise, one warm-up then `reps` runs (median, smallest, largest); every run
uses fresh points, so the M-call route never finds its tables cached.  The openings of both routes are compared.  Then kzg.batch_verify of
2^10 and 2^16 honest openings: wall time and the device time of its two entry points.  There is no threshold: the figures are context.  A
run without a GPU fails; it prints no number."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd import kzg  # noqa: E402
from distributed_plonk_amd import verifier as VF  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3
CURVE = "bn254"


def stat(ms: list) -> str:
    return f"median {statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


def m_calls(w, d_poly, n, pts, d_rows):
    """The openings at pts by the single-point entry points: (values, proofs, ms of the eval + division rounds)."""
    row = n - 1
    w.sync()
    t = time.perf_counter()
    vals = []
    for j, z in enumerate(pts):
        vals.append(w.poly_eval_dev(d_poly, n, z))
        w.poly_div_linear_dev(d_poly, n, z, d_rows + j * row * 32)
    w.sync()
    rounds = (time.perf_counter() - t) * 1e3
    jac = w.commit_many_dev([(d_rows + j * row * 32, row) for j in range(len(pts))])
    return np.stack(vals), [kzg._affine(w, j) for j in jac], rounds


def probe_open(w, log: int, Ms, reps: int) -> list:
    f = _fr.FIELDS[CURVE]
    n = 1 << log
    rng = random.Random(20)
    lines = []
    with w.scope() as s:
        d_srs, d_poly = s.alloc(n * 2 * w.q64 * 8), s.alloc(n * 32)
        w.synth_srs(f.to_limbs(TAU % f.p), n, d_srs.ptr)
        w.init_dev(d_srs.ptr, n, 0, 0)
        w.synth_fr(11, d_poly.ptr, n)
        d_rows = s.alloc(max(Ms) * (n - 1) * 32)
        for M in Ms:
            dev, many, rounds, whole, same = [], [], [], [], True
            for rep in range(reps + 1):
                pts = f.vec_to_limbs([rng.randrange(f.p) for _ in range(M)])
                with w.scope() as t:                          # the device time of the one call, on its own
                    d_pts, d_val, d_st = t.upload(pts), t.alloc(M * 32), t.alloc(M * 4)
                    w.poly_open_many_dev(d_poly.ptr, n, d_pts.ptr, M, d_val.ptr, d_rows.ptr, n - 1, d_st.ptr)
                    ms_dev = w.last_kernel_ms()
                w.sync()
                t0 = time.perf_counter()
                ops = kzg.open_many(w, (d_poly, n), pts, max_scratch_bytes=M * (n - 1) * 32)
                ms_many = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                vals, proofs, ms_rounds = m_calls(w, d_poly.ptr, n, pts, d_rows.ptr)
                ms_whole = (time.perf_counter() - t0) * 1e3
                same = same and all(np.array_equal(o.value, v) and np.array_equal(o.proof_xy, p) for o, v, p in zip(ops, vals, proofs))
                if rep:
                    dev.append(ms_dev); many.append(ms_many); rounds.append(ms_rounds); whole.append(ms_whole)
            ratio = statistics.median(whole) / statistics.median(many)
            lines += [f"  M = {M}, 2^{log} coefficients ({reps} runs after 1 warm-up, fresh points each run; both routes give the same openings: {same}):",
                      f"    many-point: plonk_poly_open_many_dev device time {stat(dev)}; kzg.open_many wall {stat(many)}",
                      f"    M calls:    eval + division rounds wall {stat(rounds)}; with the commitments, wall {stat(whole)}",
                      f"    M calls / many-point, whole openings: {ratio:.2f}x; rounds / device time of the one call: "
                      f"{statistics.median(rounds) / statistics.median(dev):.2f}x"]
            print("\n".join(lines[-4:]), flush=True)
            assert same
    return lines


def probe_verify(w, logs, reps: int) -> list:
    f = _fr.FIELDS[CURVE]
    key = VF.OpenKey.from_trapdoor(CURVE, TAU)
    rng = random.Random(21)
    coeffs = f.vec_to_limbs([rng.randrange(f.p) for _ in range(1 << 10)])
    comm = kzg.commit(w, coeffs)
    base = kzg.open_many(w, coeffs, f.vec_to_limbs([rng.randrange(f.p) for _ in range(64)]))
    lines = []
    for log in logs:
        K = 1 << log
        ops = [base[i % 64] for i in range(K)]
        wall, kms, ok = [], [], True
        for rep in range(reps + 1):
            st = {}
            t0 = time.perf_counter()
            verdict = kzg.batch_verify(w, key, [comm] * K, ops, stats=st)
            ms = (time.perf_counter() - t0) * 1e3
            ok = ok and all(verdict) and st["pairing_checks"] == 1
            if rep:
                wall.append(ms); kms.append(st["kernel_ms"])
        lines.append(f"  kzg.batch_verify, K = 2^{log} honest openings (64 distinct), one pairing check, all accepted: {ok}: wall {stat(wall)}; "
                     f"device: plonk_kzg_pairs_dev {stat([k['verify'] for k in kms])}, plonk_g1_sum_tree_dev {stat([k['tree'] for k in kms])}")
        print(lines[-1], flush=True)
        assert ok
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--points", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--verify-logs", type=int, nargs="*", default=[10, 16])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = [f"tools/kzg_probe.py --log {a.log} --points {' '.join(map(str, a.points))} --reps {a.reps}: one MI355X, {CURVE}, tile {kzg.tile()}"]
    w = PlonkWorker(me=0, device=0, curve=CURVE)
    try:
        lines += probe_open(w, a.log, a.points, a.reps)
        lines += probe_verify(w, a.verify_logs, a.reps)
    finally:
        w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
