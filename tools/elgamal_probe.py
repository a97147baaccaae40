"""Rates of the sponge, stream and shared-key kernels (csrc/elgamal_kernels.hpp) and of a whole encryption on one GPU.

    python tools/elgamal_probe.py [--log 20] [--curve bn254 bls12_381] [--reps 5] [--out profiles/elgamal_probe.txt]

Times, at 2^log lanes and from the HIP events the library records around its own launches, one warm-up then `reps` runs (median, smallest,
largest): plonk_rescue_sponge_dev at L = 4 (two permutations per lane), plonk_rescue_stream_dev at L = 4 (2^(log-1) texts of two blocks),
plonk_edwards_dh_key_dev (its two launches together), and the launches of elgamal.encrypt_dev at L = 4 over 2^log ciphertexts; each with the field products per
second implied by 16 608 products per permutation, bit_length(r) x 19 + 338 per variable-base and 64 x 11 + 337 per fixed-base
multiplication.  In the same run it times the route to the shared key through the older entry points — plonk_edwards_mul_dev, the
states (S.x, S.y, 0, 0) assembled on the host (download, numpy, upload: by the wall clock), plonk_rescue_permute_dev — with the assembly
and without it, beside plonk_edwards_dh_key_dev, which needs no assembly.  There is no threshold: the figures are context.  A run without a GPU fails; it prints no number."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import edwards as ED  # noqa: E402
from distributed_plonk_amd import elgamal as EG  # noqa: E402
from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd import rescue as RS  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

PERMUTATION = 12 * (4 * 335 + 12 + 32)                # 16 608 products
FIXED_MUL = 64 * 11 + 337


def timed(w: PlonkWorker, names, call, reps: int) -> list:
    """the summed event time of the launches named `names`, per run"""
    out = []
    for rep in range(reps + 1):
        w.sync()
        w.profile_reset()
        w.profile_enable(True)
        call()
        w.sync()
        ms = sum(w.profile_get(n)[0] for n in names)
        w.profile_enable(False)
        if rep:
            out.append(ms)
    return out


def line(what: str, count: int, products: int, ms: list, unit: str) -> str:
    med = statistics.median(ms)
    rate = count / (med * 1e-3)
    return (f"  {what}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs after 1 warm-up)  ->  {rate / 1e6:.2f} M {unit}/s, "
            f"{rate * products / 1e9:.1f} G field products/s implied at {products} products each")


def probe(curve: str, log: int, reps: int) -> list:
    w = PlonkWorker(me=0, device=0, curve=curve)
    prm, rp = ED.EdwardsParams.default(curve), RS.RescueParams.default(curve)
    bits = _fr.FIELDS[curve].p.bit_length()
    mul = bits * 19 + 338
    count, L = 1 << log, 4
    lines = [f"{curve}:"]
    bufs = []
    try:
        alloc = lambda nbytes: bufs.append(w.alloc(nbytes)) or bufs[-1]
        d_k, d_p, d_E, d_keys = alloc(count * 32), alloc(count * 64), alloc(count * 64), alloc(count * 32)
        d_msg, d_ct, d_hash, d_states = alloc(count * L * 32), alloc(count * L * 32), alloc(count * 32), alloc(count * 128)
        w.synth_fr(1, d_k.ptr, count)
        ED.fixed_mul_dev(w, prm, d_k.ptr, count, d_p.ptr)              # the points (encryption keys); also builds the table
        w.synth_fr(2, d_k.ptr, count)
        w.synth_fr(3, d_msg.ptr, count * L)
        lines.append(line(f"sponge, L = {L}, 2^{log} lanes, one launch", count, 2 * PERMUTATION,
                          timed(w, ["rescue_sponge"], lambda: RS.sponge_dev(w, rp, d_msg.ptr, L, count, 1, d_hash.ptr), reps), "messages"))
        lines.append(line(f"stream, L = {L}, 2^{log - 1} texts = 2^{log} lanes, one launch", count, PERMUTATION,
                          timed(w, ["rescue_stream"], lambda: RS.stream_dev(w, rp, d_keys.ptr, d_msg.ptr, L, count // 2, d_ct.ptr), reps), "blocks"))
        fused = timed(w, ["edwards_dh_key"], lambda: EG.dh_key_dev(w, prm, rp, d_k.ptr, d_p.ptr, count, d_keys.ptr), reps)
        lines.append(line(f"dh_key, 2^{log} lanes, two launches (multiplication, permutation)", count, mul + PERMUTATION, fused, "keys"))
        lines.append(line(f"encrypt_dev, L = {L}, 2^{log} ciphertexts, four launches (fixed_mul, dh_key's two, stream of 2^{log + 1} lanes)", count,
                          FIXED_MUL + mul + 3 * PERMUTATION,
                          timed(w, ["edwards_fixed_mul", "edwards_dh_key", "rescue_stream"],
                                lambda: EG.encrypt_dev(w, prm, d_p.ptr, d_msg.ptr, d_k.ptr, L, count, d_E.ptr, d_ct.ptr, d_keys.ptr, rp), reps), "ciphertexts"))
        # the route through the older entry points: mul, the states assembled on the host, permute
        two = timed(w, ["edwards_mul", "rescue_permute"],
                    lambda: (ED.mul_dev(w, prm, d_k.ptr, d_p.ptr, count, d_E.ptr), RS.permute_dev(w, rp, d_states.ptr, count)), reps)
        walls = []
        same = None
        for rep in range(reps + 1):
            w.sync()
            t = time.perf_counter()
            ED.mul_dev(w, prm, d_k.ptr, d_p.ptr, count, d_E.ptr)
            S = d_E.download((count, 2, 4))
            states = np.zeros((count, 4, 4), dtype=np.uint64)
            states[:, :2] = S
            d_states.upload(states)
            RS.permute_dev(w, rp, d_states.ptr, count)
            w.sync()
            if rep:
                walls.append((time.perf_counter() - t) * 1e3)
            else:
                same = np.array_equal(d_states.download((count, 4, 4))[:, 0], d_keys.download((count, 4)))
        assert same, "the two routes disagree"
        f_med, t_med, w_med = statistics.median(fused), statistics.median(two), statistics.median(walls)
        lines.append(f"  the same keys by mul_dev + permute_dev: the two launches alone median {t_med:.3f} ms (min {min(two):.3f}, max {max(two):.3f}); with the states "
                     f"(S.x, S.y, 0, 0) assembled on the host between them, wall clock, median {w_med:.1f} ms (min {min(walls):.1f}, max {max(walls):.1f}); "
                     f"dh_key {f_med:.3f} ms: {100 * (f_med - t_med) / t_med:+.2f} % against the launches alone "
                     f"(spread of the dh_key runs {100 * (max(fused) - min(fused)) / f_med:.2f} %); both routes give identical bytes")
    finally:
        for b in bufs:
            b.free()
        w.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--curve", nargs="+", default=["bn254", "bls12_381"], choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = [f"tools/elgamal_probe.py --log {a.log} --reps {a.reps}: one MI355X"]
    for curve in a.curve:
        got = probe(curve, a.log, a.reps)
        lines += got
        print("\n".join(got), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
