"""ark-serialize 0.3 bytes <-> the library's Montgomery limbs, on the device (csrc/codec_kernels.hpp; include/plonk_hip.h: plonk_*_bytes*).

What a ceremony, another party's prover and a key file hand over is bytes — `to_bytes!` of the reference: a G1Affine is its x coordinate
little-endian with two flag bits in the last byte (0x80: y is the larger of {y, -y}; 0x40: infinity), or x then y uncompressed; an Fr is 32
bytes.  `transcript.serialize_*` writes that encoding on the host; this module reads and writes it on the device, one lane per element: a
compressed point costs one Fq power (both base fields have q = 3 mod 4) and one squaring.

A bad element is never an exception of the array forms: it is a bit in that element's status word (STATUS_BITS) and zeros in the output.
`proof_from_bytes`, `commitments_from_bytes` and `PlonkWorker.init_bytes` are the forms that raise.  Two things are stricter or less pinned
than ark-serialize: an infinity whose other bytes are not zero is refused, and the `Proof` layout is the one of
`transcript.serialize_proof`.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _ffi
from .transcript import FQ_MODULI, serialize_g1
from .worker import DeviceScope

ENCODINGS = {"compressed": _ffi.PLONK_BYTES_COMPRESSED, "uncompressed": _ffi.PLONK_BYTES_UNCOMPRESSED}
STATUS_BITS = {1: "no point has this x, or the pair is off the curve", 2: "point outside the r-subgroup", 8: "non-canonical encoding",
               16: "a Vec length of the proof differs from 5, 5, 5, 4"}
NPTS, NEVALS = 13, 10


def status_text(status: int) -> str:
    return f"status {int(status)} (" + "; ".join(t for b, t in STATUS_BITS.items() if int(status) & b) + ")"


def _q64(curve: str) -> int:
    return _ffi.FQ_LIMBS64[_ffi.CURVES[curve]]


def g1_nbytes(curve: str, encoding: str = "compressed") -> int:
    return 8 * _q64(curve) * (2 if ENCODINGS[encoding] else 1)


def proof_nbytes(curve: str) -> int:
    """len(transcript.serialize_proof(...)): 768 on BN254, 976 on BLS12-381"""
    return NPTS * g1_nbytes(curve) + NEVALS * 32 + 4 * 8


def _u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)             # a view: no second host copy
    return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)


def g1_encode_host(curve: str, xy, encoding: str = "compressed") -> bytes:
    """One point on the host (big integers): transcript.serialize_g1, and its uncompressed sibling.  xy: x || y Montgomery, (0, 0) = infinity."""
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1)
    inf = not xy.any()
    if not ENCODINGS[encoding]:
        return serialize_g1(curve, xy, inf)
    nb, n, q = g1_nbytes(curve), _q64(curve), FQ_MODULI[curve]
    if inf:
        return bytes(2 * nb - 1) + b"\x40"
    r_inv = pow(pow(2, 64 * n, q), -1, q)
    val = lambda l: sum(int(w) << (64 * i) for i, w in enumerate(l)) * r_inv % q
    return val(xy[:n]).to_bytes(nb, "little") + val(xy[n:]).to_bytes(nb, "little")


# ------------------------------------------------------------------------------------------------ device-pointer forms
def g1_from_bytes_dev(w, d_bytes: int, count: int, d_out_xy: int, d_status: int, encoding: str = "compressed", check_subgroup: bool = True,
                      in_stride: int = 0, out_stride_u64: int = 0, status_stride: int = 1):
    """count elements at d_bytes (in_stride bytes apart; 0 = back to back) -> x || y at d_out_xy (out_stride_u64 u64 apart; 0 = back to back),
    status bits OR-ed into the u32 words at d_status, which the caller cleared.  Enqueued, not synchronised."""
    w.g1_from_bytes_dev(d_bytes, in_stride or g1_nbytes(w.curve_name, encoding), count, ENCODINGS[encoding], check_subgroup, d_out_xy,
                        out_stride_u64 or 2 * w.q64, d_status, status_stride)


def g1_to_bytes_dev(w, d_xy: int, count: int, d_bytes: int, encoding: str = "compressed", in_stride_u64: int = 0, out_stride: int = 0):
    w.g1_to_bytes_dev(d_xy, in_stride_u64 or 2 * w.q64, count, ENCODINGS[encoding], d_bytes, out_stride or g1_nbytes(w.curve_name, encoding))


def fr_from_bytes_dev(w, d_bytes: int, count: int, d_out: int, d_status: int, in_stride: int = 32, out_stride_u64: int = 4, status_stride: int = 1):
    w.fr_from_bytes_dev(d_bytes, in_stride, count, d_out, out_stride_u64, d_status, status_stride)


def fr_to_bytes_dev(w, d_fr: int, count: int, d_bytes: int, in_stride_u64: int = 4, out_stride: int = 32):
    w.fr_to_bytes_dev(d_fr, in_stride_u64, count, d_bytes, out_stride)


# ------------------------------------------------------------------------------------------------ host-array forms
def _alloc(s: DeviceScope, nbytes: int):
    return s.alloc(max(nbytes, 8))


def g1_from_bytes(w, data, encoding: str = "compressed", check_subgroup: bool = True):
    """Serialized points back to back -> (xy (count, 2Q) u64 Montgomery with (0, 0) for infinity and for a bad element, status (count,) u32)."""
    raw, nb = _u8(data), g1_nbytes(w.curve_name, encoding)
    if raw.size % nb:
        raise ValueError(f"g1_from_bytes: {raw.size} bytes is not a multiple of {nb}")
    count = raw.size // nb
    if count == 0:
        return np.zeros((0, 2 * w.q64), np.uint64), np.zeros((0,), np.uint32)
    with DeviceScope(w) as s:
        d_in, d_out, d_st = _alloc(s, raw.nbytes).upload(raw), _alloc(s, count * 16 * w.q64), _alloc(s, count * 4)
        w.memset_dev(d_st.ptr, 0, count * 4)
        g1_from_bytes_dev(w, d_in.ptr, count, d_out.ptr, d_st.ptr, encoding, check_subgroup)
        return d_out.download((count, 2 * w.q64)), d_st.download((count,), dtype=np.uint32)


def g1_to_bytes(w, xy, encoding: str = "compressed") -> bytes:
    """(count, 2Q) u64 points -> their serialization back to back (transcript.serialize_g1 for each, byte for byte)."""
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 2 * w.q64)
    count, nb = xy.shape[0], g1_nbytes(w.curve_name, encoding)
    if count == 0:
        return b""
    with DeviceScope(w) as s:
        d_in, d_out = _alloc(s, xy.nbytes).upload(xy), _alloc(s, count * nb)
        g1_to_bytes_dev(w, d_in.ptr, count, d_out.ptr, encoding)
        return d_out.download((count * nb,), dtype=np.uint8).tobytes()


def fr_from_bytes(w, data):
    """32-byte little-endian scalars back to back -> (limbs (count, 4) u64 Montgomery, status (count,) u32: 8 and 0 for a value >= r)."""
    raw = _u8(data)
    if raw.size % 32:
        raise ValueError(f"fr_from_bytes: {raw.size} bytes is not a multiple of 32")
    count = raw.size // 32
    if count == 0:
        return np.zeros((0, 4), np.uint64), np.zeros((0,), np.uint32)
    with DeviceScope(w) as s:
        d_in, d_out, d_st = _alloc(s, raw.nbytes).upload(raw), _alloc(s, count * 32), _alloc(s, count * 4)
        w.memset_dev(d_st.ptr, 0, count * 4)
        fr_from_bytes_dev(w, d_in.ptr, count, d_out.ptr, d_st.ptr)
        return d_out.download((count, 4)), d_st.download((count,), dtype=np.uint32)


def fr_to_bytes(w, limbs) -> bytes:
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
    count = limbs.shape[0]
    if count == 0:
        return b""
    with DeviceScope(w) as s:
        d_in, d_out = _alloc(s, limbs.nbytes).upload(limbs), _alloc(s, count * 32)
        fr_to_bytes_dev(w, d_in.ptr, count, d_out.ptr)
        return d_out.download((count * 32,), dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------------ proofs and Vec<Commitment>
def _proofs_into(s: DeviceScope, blobs: Sequence[bytes]):
    """proofs_from_bytes_dev with the records in a buffer of the scope `s`: what a caller that frees them with the rest of its call takes."""
    w = s.worker
    nb = proof_nbytes(w.curve_name)
    blobs = [bytes(b) for b in blobs]
    for i, b in enumerate(blobs):
        if len(b) != nb:
            raise ValueError(f"proof {i}: {len(b)} bytes, a serialized proof on {w.curve_name} has {nb}")
    K = len(blobs)
    rec_u64 = 2 * w.q64 * NPTS + 4 * NEVALS
    d_recs = _alloc(s, K * rec_u64 * 8)
    if K == 0:
        return d_recs, np.zeros((0,), np.uint32)
    d_in = s.alloc(K * nb).upload(np.frombuffer(b"".join(blobs), dtype=np.uint8))
    d_st = s.alloc(K * 4)
    w.proofs_from_bytes_dev(d_in.ptr, K, d_recs.ptr, d_st.ptr)
    status = d_st.download((K,), dtype=np.uint32)
    s.free(d_in)
    s.free(d_st)
    return d_recs, status


def proofs_from_bytes_dev(w, blobs: Sequence[bytes]):
    """Serialized proofs -> (DeviceBuffer of len(blobs) records of plonk_verify_batch_dev — the caller frees it —, status (K,) u32).  The
    records stay on the device; only the status words come back.  ValueError for a blob of another length than proof_nbytes(curve)."""
    with DeviceScope(w) as s:
        d_recs, status = _proofs_into(s, blobs)
        return s.release(d_recs), status


def proof_from_bytes(w, blob: bytes) -> dict:
    """One serialized proof -> the dict `Prover.prove` returns (points as (xy, is_infinity), scalars as Montgomery limbs).  ValueError naming
    the status for a blob that does not decode."""
    with DeviceScope(w) as s:
        d_recs, status = _proofs_into(s, [blob])
        if status[0]:
            raise ValueError(f"proof_from_bytes: {status_text(status[0])}")
        rec = d_recs.download((2 * w.q64 * NPTS + 4 * NEVALS,))
    n2 = 2 * w.q64
    pt = lambda i: (rec[n2 * i:n2 * (i + 1)].copy(), not rec[n2 * i:n2 * (i + 1)].any())
    ev = lambda i: rec[n2 * NPTS + 4 * i:n2 * NPTS + 4 * (i + 1)].copy()
    return {"wires_poly_comms": [pt(i) for i in range(5)], "prod_perm_poly_comm": pt(5), "split_quot_poly_comms": [pt(i) for i in range(6, 11)],
            "opening_proof": pt(11), "shifted_opening_proof": pt(12), "wires_evals": [ev(i) for i in range(5)],
            "wire_sigma_evals": [ev(i) for i in range(5, 9)], "perm_next_eval": ev(9)}


def commitments_from_bytes(w, blob: bytes, check_subgroup: bool = True) -> list:
    """A serialized `Vec<Commitment>` — u64 little-endian length, then compressed points — -> [(xy, is_infinity), ...], the form of a
    verifying key's selector_comms / sigma_comms.  ValueError for a length that does not match the blob or an element that does not decode."""
    blob = bytes(blob)
    nb = g1_nbytes(w.curve_name)
    if len(blob) < 8 or (len(blob) - 8) % nb or int.from_bytes(blob[:8], "little") != (len(blob) - 8) // nb:
        raise ValueError("commitments_from_bytes: the length prefix does not match the blob")
    xy, status = g1_from_bytes(w, blob[8:], "compressed", check_subgroup)
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError(f"commitments_from_bytes: element {int(bad[0])}: {status_text(status[bad[0]])}")
    return [(p.copy(), not p.any()) for p in xy]


# ------------------------------------------------------------------------------------------------ G2 (host only)
def g2_from_bytes(curve: str, blob: bytes):
    """A serialized G2Affine (compressed: 2 x Q x 8 bytes, uncompressed: 4 x) -> (x.c0 || x.c1 || y.c0 || y.c1 Montgomery, status).  No GPU."""
    blob = bytes(blob)
    n = 8 * _q64(curve)
    if len(blob) not in (2 * n, 4 * n):
        raise ValueError(f"g2_from_bytes: {len(blob)} bytes, a G2 element on {curve} has {2 * n} or {4 * n}")
    out = np.zeros(4 * _q64(curve), np.uint64)
    st = C.c_int(0)
    _ffi.check(_ffi.lib().plonk_g2_from_bytes(_ffi.CURVES[curve], blob, 0 if len(blob) == 2 * n else 1, out.ctypes.data, C.byref(st)))
    return out, st.value


def g2_to_bytes(curve: str, pt, encoding: str = "compressed") -> bytes:
    pt = np.ascontiguousarray(pt, dtype=np.uint64).reshape(-1)
    if pt.shape != (4 * _q64(curve),):
        raise ValueError("g2_to_bytes: 4Q u64 expected")
    out = C.create_string_buffer(8 * _q64(curve) * (4 if ENCODINGS[encoding] else 2))
    _ffi.check(_ffi.lib().plonk_g2_to_bytes(_ffi.CURVES[curve], pt.ctypes.data, ENCODINGS[encoding], out))
    return out.raw
