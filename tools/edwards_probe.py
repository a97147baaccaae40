"""Rates of the Edwards kernels (csrc/edwards_kernels.hpp) and times of the signature circuit on one GPU.

    python tools/edwards_probe.py [--log 20] [--sigs 65536] [--circuit 16] [--curve bn254 bls12_381] [--reps 5] [--out profiles/edwards_probe.txt]

Times plonk_edwards_mul_dev and plonk_edwards_fixed_mul_dev at 2^log lanes from the HIP events the library records around its own launches
("edwards_mul", "edwards_fixed_mul"; the points are [k] G for random k, made on the device), one warm-up then `reps` runs: the median, the
smallest and the largest, the points per second and the implied field products per second at bit_length(r) x 19 + 338 products per
variable-base and 64 x 11 + 337 per fixed-base multiplication.  Then, by the wall clock: edwards.schnorr_verify over `sigs` signatures
(uploads, the two Rescue hashes, the curve check, both multiplications, the addition, the download and the comparison), and
edwards.schnorr_circuit(curve, `circuit`): build, solve_dev, preprocess and prove_dev, once each after nothing but the library's own warm-up.
For scale it times the pure-Python reference's scalar multiplication on this host.  There is no threshold: the figures are context.  A run
without a GPU fails; it prints no number."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import edwards as ED  # noqa: E402
from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd import verifier as VF  # noqa: E402
from distributed_plonk_amd.prover import Prover  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF


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


def line(what: str, count: int, products: int, ms: list) -> str:
    med = statistics.median(ms)
    rate = count / (med * 1e-3)
    return (f"  {what}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs after 1 warm-up)  ->  {rate / 1e6:.2f} M points/s, "
            f"{rate * products / 1e9:.1f} G field products/s implied at {products} products each")


def wall(w: PlonkWorker, call):
    w.sync()
    t = time.perf_counter()
    out = call()
    w.sync()
    return out, (time.perf_counter() - t) * 1e3


def probe(curve: str, log: int, sigs: int, m: int, reps: int) -> list:
    w = PlonkWorker(me=0, device=0, curve=curve)
    prm = ED.EdwardsParams.default(curve)
    f = _fr.FIELDS[curve]
    bits = f.p.bit_length()
    count = 1 << log
    lines = [f"{curve}:"]
    try:
        d_k, d_p, d_out = w.alloc(count * 32), w.alloc(count * 64), w.alloc(count * 64)
        try:
            w.synth_fr(1, d_k.ptr, count)
            ED.fixed_mul_dev(w, prm, d_k.ptr, count, d_p.ptr)          # the points; also builds the table
            w.synth_fr(2, d_k.ptr, count)
            lines.append(line(f"mul, 2^{log} lanes, one launch", count, bits * 19 + 338, timed(w, "edwards_mul", lambda: ED.mul_dev(w, prm, d_k.ptr, d_p.ptr, count, d_out.ptr), reps)))
            lines.append(line(f"fixed_mul, 2^{log} lanes, one launch", count, 64 * 11 + 337,
                              timed(w, "edwards_fixed_mul", lambda: ED.fixed_mul_dev(w, prm, d_k.ptr, count, d_out.ptr), reps)))
        finally:
            for b in (d_k, d_p, d_out):
                b.free()
        rnd = random.Random(curve)
        rand = lambda n: np.frombuffer(b"".join(rnd.randrange(1, f.p).to_bytes(32, "little") for _ in range(n)), dtype=np.uint64).reshape(n, 4).copy()
        sk, nonce, msg = rand(sigs), rand(sigs), rand(sigs)            # any canonical limbs are some residue's Montgomery form
        pk, t_key = wall(w, lambda: ED.keygen(w, prm, sk))
        (R, s), t_sign = wall(w, lambda: ED.schnorr_sign(w, prm, sk, nonce, msg))
        ok, t_ver = wall(w, lambda: ED.schnorr_verify(w, prm, pk, msg, (R, s)))
        assert ok.all()
        lines.append(f"  {sigs} signatures, wall clock: keygen {t_key:.1f} ms, schnorr_sign {t_sign:.1f} ms (s on the host in Python integers), schnorr_verify {t_ver:.1f} ms "
                     f"-> {sigs / (t_ver * 1e-3) / 1e3:.1f} k verifications/s")
        t = time.perf_counter()
        built = ED.schnorr_circuit(curve, m)
        t_build = (time.perf_counter() - t) * 1e3
        inputs, public = ED.schnorr_witness_inputs(pk[:m], msg[:m], (R[:m], s[:m]))
        solved, t_solve0 = wall(w, lambda: built.solve_dev(w, inputs, public))
        solved.close()
        solved, t_solve = wall(w, lambda: built.solve_dev(w, inputs, public))
        levels = solved.levels
        solved.close()
        inst, t_pre = wall(w, lambda: built.preprocess(w, inputs, public, check=True))
        n = built.n
        key_size = ((n + 3 + 31) >> 5) << 5
        ck = w.alloc(key_size * (64 if curve == "bn254" else 96))
        pv = None
        try:
            w.memset_dev(ck.ptr, 0, ck.nbytes)
            w.synth_srs(f.to_limbs(TAU), n + 3, ck.ptr)
            w.init_dev(ck.ptr, key_size, n, 8 * n)
            pv = Prover(w, built.log_n)
            pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
            pub = inst.public_inputs()
            blinders = dict(wires=rand(10).reshape(5, 2, 4), perm=rand(3))
            prove = lambda: pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(pub))
            _, t_prove0 = wall(w, prove)
            proof, t_prove = wall(w, prove)
            assert VF.verify(w, pv.verifying_key(), VF.OpenKey.from_trapdoor(curve, TAU), pub, proof)
        finally:
            if pv is not None:
                pv.close()
            inst.close()
            ck.free()
            built.close()
        lines.append(f"  schnorr_circuit({curve!r}, {m}): {built.num_gates_unpadded} gates, n = 2^{built.log_n}, {levels} levels; wall clock: build {t_build:.0f} ms (host), "
                     f"solve_dev {t_solve:.1f} ms (first call, with the upload: {t_solve0:.1f}), preprocess with check {t_pre:.1f} ms, prove_dev {t_prove:.1f} ms "
                     f"(first call {t_prove0:.1f}); the proof verifies")
    finally:
        w.close()
    return lines


def reference_time(curve: str) -> str:
    from tests import edwards_ref as E
    rnd = random.Random(1)
    ks = [rnd.randrange(E.MODULI[curve]) for _ in range(8)]
    t = time.perf_counter()
    for k in ks:
        E.mul(curve, k, E.PARAMS[curve]["G"])
    return f"  tests/edwards_ref.py on this host, {curve}: {(time.perf_counter() - t) / len(ks) * 1e3:.1f} ms per scalar multiplication"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--sigs", type=int, default=1 << 16)
    ap.add_argument("--circuit", type=int, default=16)
    ap.add_argument("--curve", nargs="+", default=["bn254", "bls12_381"], choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = [f"tools/edwards_probe.py --log {a.log} --sigs {a.sigs} --circuit {a.circuit} --reps {a.reps}: one MI355X"]
    for curve in a.curve:
        got = probe(curve, a.log, a.sigs, a.circuit, a.reps) + [reference_time(curve)]
        lines += got
        print("\n".join(got), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
