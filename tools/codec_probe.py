"""Rates of the byte codec (csrc/codec_kernels.hpp) and of an SRS loaded from bytes, on one GPU.

    python tools/codec_probe.py [--log 20] [--curve bn254 bls12_381] [--reps 5] [--srs-logs 22 24] [--out profiles/codec.txt]

Times by the host clock around calls that end in a device synchronise, one warm-up then `reps` runs (median, smallest, largest), at 2^log
points; the kernels that take tens of microseconds (encode, the uncompressed and the Fr forms) are timed as windows of 200 calls enqueued back
to back and reported per call, with the bytes they move, since one such call alone would time the launch and the synchronise:
plonk_g1_from_bytes_dev compressed (without and, on BLS12-381, with the subgroup check) and uncompressed, plonk_g1_to_bytes_dev in both forms, plonk_fr_from_bytes_dev / plonk_fr_to_bytes_dev; each also as Fq (Fr) products per second, counted from the exponent's windows:
the 32-bit-word Fq multiplier of fp.hpp, not the 29-bit-limb Fr multiplier behind the 94 - 97 G/s of profiles/elgamal.txt.  Then, on BN254,
`init_bytes` for 2^22 and 2^24 compressed points: the whole call, and its three parts done from here — upload, decode, init_dev.  Last the
pure-Python decoder of tests/codec_ref.py at 2^10 points, the route a user had before.  There is no threshold: the figures are context.  A
run without a GPU fails; it prints no number."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_plonk_amd import codec as CD  # noqa: E402
from distributed_plonk_amd import fr as _fr  # noqa: E402
from distributed_plonk_amd.transcript import FQ_MODULI  # noqa: E402
from distributed_plonk_amd.worker import PlonkWorker  # noqa: E402

TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


def sqrt_products(q: int) -> int:
    """fp_sqrt_3mod4: a^2, a^3, then per 2-bit window of q >> 2 two squarings (after the first non-zero window) and a product (non-zero
    windows), and the closing product by a"""
    e, n, started = q >> 2, 2, False
    for w in range((e.bit_length() + 1) // 2 - 1, -1, -1):
        d = (e >> (2 * w)) & 3
        n += (2 if started else 0) + (1 if d else 0)
        started = started or d != 0
    return n + 1


SHORT = 200         # calls enqueued per timed window for the kernels that take tens of microseconds: one call alone would time the launch and the synchronise


def wall(w: PlonkWorker, call, reps: int, batch: int = 1) -> list:
    """ms per call: `batch` calls enqueued back to back on the context's stream between two synchronises, the window divided by `batch`"""
    out = []
    for rep in range(reps + 1):
        w.sync()
        t = time.perf_counter()
        for _ in range(batch):
            call()
        w.sync()
        if rep:
            out.append((time.perf_counter() - t) * 1e3 / batch)
    return out


def line(what: str, count: int, products: int, ms: list, batch: int = 1, nbytes: int = 0) -> str:
    med = statistics.median(ms)
    rate = count / (med * 1e-3)
    how = f"{len(ms)} windows of {batch} enqueued calls after 1 warm-up window, per call" if batch > 1 else f"{len(ms)} runs after 1 warm-up"
    traffic = f", {nbytes * rate / 1e12:.2f} TB/s read + written at {nbytes} B each" if nbytes else ""
    return (f"  {what}: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, {how})  ->  {rate / 1e6:.1f} M elements/s, "
            f"{rate * products / 1e9:.1f} G products/s at {products} products each{traffic}")


def probe(curve: str, log: int, reps: int) -> list:
    w = PlonkWorker(me=0, device=0, curve=curve)
    q, f = FQ_MODULI[curve], _fr.FIELDS[curve]
    count, nb, n2 = 1 << log, CD.g1_nbytes(curve), 2 * w.q64
    pw = sqrt_products(q)
    comp, unc, enc = 1 + 2 + pw + 1 + 1, 2 + 2 + 1, 2          # to_mont, x^3, the power, its check, from_mont for the sign | two to_mont, x^3, y^2 | two from_mont
    lines = [f"{curve}: the power takes {pw} Fq products, a compressed decode {comp}"]
    bufs = []
    try:
        alloc = lambda nbytes: bufs.append(w.alloc(nbytes)) or bufs[-1]
        d_xy, d_b, d_b2, d_out, d_st = alloc(count * n2 * 8), alloc(count * nb), alloc(count * 2 * nb), alloc(count * n2 * 8), alloc(count * 4)
        d_fr, d_fb = alloc(count * 32), alloc(count * 32)
        w.synth_srs(f.to_limbs(TAU % f.p), count, d_xy.ptr)
        w.synth_fr(7, d_fr.ptr, count)
        w.memset_dev(d_st.ptr, 0, count * 4)
        lines.append(line(f"g1_to_bytes, compressed, 2^{log}", count, enc, wall(w, lambda: CD.g1_to_bytes_dev(w, d_xy.ptr, count, d_b.ptr), reps, SHORT), SHORT,
                          n2 * 8 + nb))
        lines.append(line(f"g1_to_bytes, uncompressed, 2^{log}", count, enc,
                          wall(w, lambda: CD.g1_to_bytes_dev(w, d_xy.ptr, count, d_b2.ptr, "uncompressed"), reps, SHORT), SHORT, n2 * 8 + 2 * nb))
        lines.append(line(f"g1_from_bytes, compressed, no subgroup check, 2^{log}", count, comp,
                          wall(w, lambda: CD.g1_from_bytes_dev(w, d_b.ptr, count, d_out.ptr, d_st.ptr, check_subgroup=False), reps)))
        same = np.array_equal(d_out.download((count, n2)), d_xy.download((count, n2)))
        if curve == "bls12_381":
            sub = 255 * 9 + 128 * 12                                  # 255 doublings (6M + 3S... counted as 9) and ~128 mixed additions (12)
            lines.append(line(f"g1_from_bytes, compressed, with [r] P == O (a second launch), 2^{log}", count, comp + sub,
                              wall(w, lambda: CD.g1_from_bytes_dev(w, d_b.ptr, count, d_out.ptr, d_st.ptr, check_subgroup=True), reps)))
        lines.append(line(f"g1_from_bytes, uncompressed, no subgroup check, 2^{log}", count, unc,
                          wall(w, lambda: CD.g1_from_bytes_dev(w, d_b2.ptr, count, d_out.ptr, d_st.ptr, "uncompressed", False), reps, SHORT), SHORT,
                          n2 * 8 + 2 * nb))
        same = same and np.array_equal(d_out.download((count, n2)), d_xy.download((count, n2))) and w.codec_first_bad_dev(d_st.ptr, count) == -1
        lines.append(line(f"fr_to_bytes, 2^{log}", count, 1, wall(w, lambda: CD.fr_to_bytes_dev(w, d_fr.ptr, count, d_fb.ptr), reps, SHORT), SHORT, 64))
        lines.append(line(f"fr_from_bytes, 2^{log}", count, 1, wall(w, lambda: CD.fr_from_bytes_dev(w, d_fb.ptr, count, d_out.ptr, d_st.ptr), reps, SHORT), SHORT,
                          64))
        lines.append(f"  decoded points equal the encoded ones, no status raised: {same}")
        assert same
    finally:
        for b in bufs:
            b.free()
        w.close()
    return lines


def probe_srs(log: int, reps: int) -> list:
    curve = "bn254"
    w = PlonkWorker(me=0, device=0, curve=curve)
    f = _fr.FIELDS[curve]
    n, nb, n2 = 1 << log, CD.g1_nbytes(curve), 2 * w.q64
    d_xy, d_b, d_st = w.alloc(n * n2 * 8), w.alloc(n * nb), w.alloc(n * 4)
    try:
        w.synth_srs(f.to_limbs(TAU % f.p), n, d_xy.ptr)
        CD.g1_to_bytes_dev(w, d_xy.ptr, n, d_b.ptr)
        blob = d_b.download((n * nb,), dtype=np.uint8)
        w.memset_dev(d_st.ptr, 0, n * 4)
        whole = wall(w, lambda: w.init_bytes(blob, n, n, 8 * n, check_subgroup=False), reps)
        up = wall(w, lambda: d_b.upload(blob), reps)
        dec = wall(w, lambda: CD.g1_from_bytes_dev(w, d_b.ptr, n, d_xy.ptr, d_st.ptr, check_subgroup=False), reps)
        ini = wall(w, lambda: w.init_dev(d_xy.ptr, n, n, 8 * n), reps)
        m = statistics.median
        return [f"  init_bytes, 2^{log} compressed BN254 points ({n * nb >> 20} MiB): median {m(whole):.1f} ms (min {min(whole):.1f}, max {max(whole):.1f}, "
                f"{len(whole)} runs after 1 warm-up); its parts from the caller's side: upload {m(up):.1f} ms (pageable host memory), decode {m(dec):.1f} ms, "
                f"init_dev {m(ini):.1f} ms"]
    finally:
        for b in (d_xy, d_b, d_st):
            b.free()
        w.close()


def probe_python(curve: str, count: int) -> str:
    from tests import codec_ref as R
    from distributed_plonk_amd import verifier as VF
    pts = [R.g1_mul(curve, 3 + i, VF._G1_GEN[curve]) for i in range(16)]
    blobs = [R.g1_encode(curve, pts[i % 16]) for i in range(count)]
    t = time.perf_counter()
    for b in blobs:
        R.g1_decode(curve, b, "compressed", False)
    dt = time.perf_counter() - t
    return f"  pure-Python decode (tests/codec_ref.py, CPU, one thread), {curve}, {count} points: {dt * 1e3:.1f} ms  ->  {count / dt / 1e3:.1f} k points/s"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--curve", nargs="+", default=["bn254", "bls12_381"], choices=["bn254", "bls12_381"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--srs-logs", type=int, nargs="*", default=[22, 24])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = [f"tools/codec_probe.py --log {a.log} --reps {a.reps}: one MI355X"]
    for curve in a.curve:
        got = probe(curve, a.log, a.reps)
        lines += got
        print("\n".join(got), flush=True)
    if a.srs_logs:
        lines.append("an SRS from bytes (bn254):")
    for log in a.srs_logs:
        got = probe_srs(log, min(a.reps, 3))
        lines += got
        print("\n".join(got), flush=True)
    lines.append("for comparison:")
    for curve in a.curve:
        lines.append(probe_python(curve, 1 << 10))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
