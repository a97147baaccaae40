#!/usr/bin/env python3
"""Timing of batched verification (distributed_plonk_amd/verifier.py) on one GPU: device time per proof of plonk_verify_batch_dev at
K = 1, 64, 1024, 4096 (a handful of distinct 2^10 proofs tiled; the per-proof cost does not depend on n beyond zeta^n), the host pairing
check, and batch_verify against K calls of verify.      usage: python tools/verify_timing.py [--curves bn254,bls12_381] [--ks 1,64,1024,4096]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381")
    ap.add_argument("--ks", default="1,64,1024,4096")
    ap.add_argument("--single", type=int, default=16, help="proofs checked one by one with verify() for the comparison")
    a = ap.parse_args()
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
