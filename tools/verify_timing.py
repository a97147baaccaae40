#!/usr/bin/env python3
"""Timing of batched verification (distributed_plonk_amd/verifier.py) on one GPU: device time per proof of plonk_verify_batch_dev at
K = 1, 64, 1024, 4096 (a handful of distinct 2^10 proofs tiled; the per-proof cost does not depend on n beyond zeta^n), the host pairing
check, and batch_verify against K calls of verify.      usage: python tools/verify_timing.py [--curves bn254,bls12_381] [--ks 1,64,1024,4096]

--multi K times, on honest proofs of one 2^10 circuit, batch_verify (the one-key entry point, the key a kernel argument) against
batch_verify_multi (a key per proof, read from the key table): with one key, with the batch alternating between two table rows that hold
the same key, and with every second proof replaced by one of a 2^5 circuit with one public input, so that neighbouring lanes diverge.  Both
fold the batch as a sum tree on the device.  Wall time is the host clock around the whole call (uploads, kernels, the status words and the
root read back, one pairing check); kernel time is plonk_last_kernel_ms after each of the two entry points, as stats["kernel_ms"] has it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd import verifier as VF  # noqa: E402
from distributed_plonk_amd.prover import Prover  # noqa: E402
from distributed_plonk_amd.synthetic import SyntheticInstance  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

TAU = 0xC0FFEE_1234567_89ABCDEF


def _prove(w, f, log_n, num_inputs, count, seed):
    inst = SyntheticInstance(w, log_n, seed=seed, num_inputs=num_inputs, tau=TAU)
    pv = Prover(w, log_n)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        rs = np.random.RandomState(seed)
        bl = lambda: dict(wires=np.stack([f.to_limbs(int(x)) for x in rs.randint(1, 1 << 62, 10)]).reshape(5, 2, 4),
                          perm=np.stack([f.to_limbs(int(x)) for x in rs.randint(1, 1 << 62, 3)]))
        proofs = [pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, bl(), pv.fiat_shamir(pub)) for _ in range(count)]
        vk = dict(pv.verifying_key(), num_inputs=num_inputs)
    finally:
        pv.close()
        inst.close()
    return vk, pub, proofs


def multi(curve, K, repeats):
    """batch_verify against batch_verify_multi at K honest proofs; every row: the best wall time of `repeats` after a warm-up, and the kernel
    time of that call."""
    w = PlonkWorker(0, 0, curve)
    f = _fr.FIELDS[curve]
    try:
        vk, pub, proofs = _prove(w, f, 10, 3, 4, 3)
        vk5, pub5, proofs5 = _prove(w, f, 5, 1, 4, 5)
        key = VF.OpenKey.from_trapdoor(curve, TAU)
        batch = [proofs[i % 4] for i in range(K)]
        mixed = [(proofs5 if i % 2 else proofs)[(i // 2) % 4] for i in range(K)]
        rows = {}

        def timed(name, call):
            call()                                            # warm-up: code objects, the context's buffers
            best = None
            for _ in range(repeats):
                st = {}
                t = time.perf_counter()
                ok = call(st)
                wall = 1000 * (time.perf_counter() - t)
                assert all(ok) and len(ok) == K and st["pairing_checks"] == 1
                if best is None or wall < best["wall_ms"]:
                    kms = st["kernel_ms"]                     # of plonk_verify_batch(_multi)_dev and of plonk_g1_sum_tree_dev
                    best = dict(wall_ms=round(wall, 2), pairing_checks=st["pairing_checks"], kernel_ms=round(sum(kms.values()), 3),
                                verify_kernel_ms=round(kms["verify"], 3), tree_kernel_ms=round(kms["tree"], 3))
            rows[name] = best

        timed("batch_verify", lambda st=None: VF.batch_verify(w, vk, key, [pub] * K, batch, seed=1, stats=st))
        with VF.VerifyKeySet(w, [vk]) as ks:
            timed("batch_verify_multi_one_key", lambda st=None: VF.batch_verify_multi(w, ks, key, [0] * K, [pub] * K, batch, seed=1, stats=st))
        with VF.VerifyKeySet(w, [vk, vk]) as ks:
            timed("batch_verify_multi_two_keys", lambda st=None: VF.batch_verify_multi(w, ks, key, [i % 2 for i in range(K)], [pub] * K, batch, seed=1,
                                                                                       stats=st))
        with VF.VerifyKeySet(w, [vk, vk5]) as ks:
            timed("batch_verify_multi_two_circuits", lambda st=None: VF.batch_verify_multi(w, ks, key, [i % 2 for i in range(K)],
                                                                                           [pub5 if i % 2 else pub for i in range(K)], mixed, seed=1,
                                                                                           stats=st))
        return rows
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--ks", default="1,64,1024,4096")
    ap.add_argument("--single", type=int, default=16, help="proofs checked one by one with verify() for the comparison")
    ap.add_argument("--multi", type=int, default=0, metavar="K", help="time batch_verify against batch_verify_multi at K proofs and nothing else")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.multi:
        print(json.dumps({curve: {"K": a.multi, **multi(curve, a.multi, a.repeats)} for curve in a.curves.split(",")}))
        return
    out = {}
    for curve in a.curves.split(","):
        w = PlonkWorker(0, 0, curve)
        f = _fr.FIELDS[curve]
        inst = SyntheticInstance(w, 10, seed=3, num_inputs=3, tau=TAU)
        pv = Prover(w, 10)
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        rs = np.random.RandomState(1)
        bl = lambda: dict(wires=np.stack([f.to_limbs(int(x)) for x in rs.randint(1, 1 << 62, 10)]).reshape(5, 2, 4),
                          perm=np.stack([f.to_limbs(int(x)) for x in rs.randint(1, 1 << 62, 3)]))
        proofs = [pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, bl(), pv.fiat_shamir(pub)) for _ in range(4)]
        vk = pv.verifying_key()
        key = VF.OpenKey.from_trapdoor(curve, TAU)
        res = {}
        for K in [int(k) for k in a.ks.split(",")]:
            batch = [proofs[i % 4] for i in range(K)]
            rho = VF._rhos(curve, K, 1)
            VF.device_verify(w, vk, [pub] * K, batch, rho)
            best = 1e9
            for _ in range(3):
                VF.device_verify(w, vk, [pub] * K, batch, rho)
                best = min(best, w.last_kernel_ms())
            res[f"device_ms_K{K}"] = round(best, 3)
            res[f"device_us_per_proof_K{K}"] = round(1000 * best / K, 2)
        g1 = VF.g1_generator(curve)
        t = time.perf_counter()
        VF.pairing_check(curve, [g1, g1], [key.h, key.beta_h])
        res["host_pairing_check_ms"] = round(1000 * (time.perf_counter() - t), 2)
        K = a.single
        batch = [proofs[i % 4] for i in range(K)]
        t = time.perf_counter()
        assert all(VF.batch_verify(w, vk, key, [pub] * K, batch, seed=1))
        res[f"batch_verify_ms_K{K}"] = round(1000 * (time.perf_counter() - t), 2)
        t = time.perf_counter()
        assert all(VF.verify(w, vk, key, pub, p) for p in batch)
        res[f"verify_x{K}_ms"] = round(1000 * (time.perf_counter() - t), 2)
        out[curve] = res
        pv.close()
        inst.close()
        w.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
