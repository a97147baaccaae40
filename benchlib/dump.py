"""--dump-outputs DIR: what the timed path computed in its last step, written as DIR/<name>.npy for an output-for-output comparison of two
builds.  Inputs are seeded, so the same arguments give the same arrays from run to run.

Every array is float64 and exact: a 64-bit limb (Montgomery field elements, affine coordinates) becomes its two 32-bit halves, low half first,
so a field element of 4 limbs is 8 numbers.  Vectors longer than SAMPLE_BLOCK * SAMPLE_BLOCKS elements are dumped as a fixed, seeded sample of
SAMPLE_BLOCKS contiguous blocks; `<name>_index.npy` then holds the element indices of the sample.  All files together stay under MAX_BYTES."""
import os

import numpy as np

MAX_BYTES = 64 << 20
SAMPLE_BLOCK, SAMPLE_BLOCKS = 4096, 16
SAMPLE_SEED = 0xD0C5


def limbs_as_float(a) -> np.ndarray:
    """uint64 limbs -> float64 of their 32-bit halves (exact: every half is below 2^53); bools -> 0.0 / 1.0"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.astype(np.float64)
    a = a.astype(np.uint64, copy=False)
    return a.view(np.uint32).reshape(a.shape[:-1] + (2 * a.shape[-1],)).astype(np.float64)


def proof_arrays(proof: dict) -> dict:
    """A proof dict of the provers (distributed_plonk_amd/prover.py, class_prover.py) -> {name: array}.  Commitments are affine points
    (xy limbs, is_infinity): `<key>_xy` and `<key>_inf`, one row per point; evaluations are field elements: `<key>`, one row per element."""
    out = {}
    for k, v in sorted(proof.items()):
        if k.startswith("_"):
            continue
        items = v if isinstance(v, list) else [v]
        if isinstance(items[0], tuple):
            out[k + "_xy"] = limbs_as_float(np.stack([np.asarray(p[0]) for p in items]))
            out[k + "_inf"] = limbs_as_float(np.array([bool(p[1]) for p in items]))
        else:
            out[k] = limbs_as_float(np.stack([np.asarray(x) for x in items]))
    return out


def sample_index(count: int) -> np.ndarray:
    """the element indices dumped of a vector of `count` elements: all of them, or SAMPLE_BLOCKS seeded blocks of SAMPLE_BLOCK"""
    if count <= SAMPLE_BLOCK * SAMPLE_BLOCKS:
        return np.arange(count)
    starts = np.sort(np.random.default_rng(SAMPLE_SEED).choice(count // SAMPLE_BLOCK, SAMPLE_BLOCKS, replace=False)) * SAMPLE_BLOCK
    return (starts[:, None] + np.arange(SAMPLE_BLOCK)).reshape(-1)


def device_vector(buf, count: int) -> dict:
    """a device vector of `count` field elements (4 limbs each) -> {"": values[, "_index": indices]} of its dumped elements"""
    idx = sample_index(count)
    if len(idx) == count:
        return {"": limbs_as_float(buf.download((count, 4)))}
    blocks = [buf.download((SAMPLE_BLOCK, 4), byte_offset=int(s) * 32) for s in idx[::SAMPLE_BLOCK]]
    return {"": limbs_as_float(np.concatenate(blocks)), "_index": idx.astype(np.float64)}


def op_mix_arrays(b, last_commitment) -> dict:
    """the op-mix step's outputs on this rank: the last of its 13 commitments (affine), the 7 size-n iNTT results and the 8n-point results
    that survive the step (lane 0: the quotient's coset iFFT; another lane: its last coset FFT), each this rank's share as the step leaves it"""
    w = b.w
    xy, inf = w.g1_to_affine(last_commitment)
    out = {"commitment_xy": limbs_as_float(xy[None]), "commitment_inf": limbs_as_float(np.array([inf]))}
    vecs = []
    if b.scheme == "classes":
        vecs += [(f"intt_n_{i}", pair[0], b.n) for i, pair in enumerate(b.cls["bn"])]
        vecs.append(("coset_ifft_8n", b.cls["quot"], b.m))
    else:
        vecs += [(f"intt_n_{i}", pair[0], b.n_loc) for i, pair in enumerate(b.buf_n)]
        if b.nbig:
            vecs += [("coset_ifft_8n" if lane == 0 else f"coset_fft_8n_lane{lane}", b.buf_m[lane][0], b.m_loc) for lane in range(b.n_lanes)]
    for name, buf, count in vecs:
        for suffix, arr in device_vector(buf, count).items():
            out[name + suffix] = arr
    return out


def write(directory: str, arrays: dict, what: str) -> dict:
    """-> the `dump_outputs` field of the result line; refuses (before writing anything) a dump above MAX_BYTES"""
    total = sum(a.nbytes for a in arrays.values())
    if total > MAX_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes exceed the {MAX_BYTES}-byte budget")
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype == np.float64, name
        np.save(os.path.join(directory, name + ".npy"), a)
    return {"dir": directory, "what": what, "files": sorted(n + ".npy" for n in arrays), "bytes": int(total)}
