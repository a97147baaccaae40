"""Verifying proofs without the SRS trapdoor: jf-plonk's `verify` / `batch_verify` (the pairing check e(A, [tau]_2) = e(B, [1]_2)).

The per-proof work runs on the device, all proofs of a batch in parallel (`plonk_verify_batch_dev`): input checks, the Fiat-Shamir replay,
the ~30 scalars of the linearised check and the two multi-scalar sums rho_k * A_k, rho_k * B_k with

    A = W_zeta + u W_zeta_omega,   B = zeta W_zeta + u zeta w W_zeta_omega + F + u [z] - (E + u z(zeta w)) G.

The host adds the K pairs and runs ONE two-pairing check e(sum rho A, beta H) * e(-sum rho B, H) == 1 (`plonk_pairing_check`); a failed
batch is bisected, so f bad proofs cost O(f log K) pairing checks.  rho_k are drawn from `secrets` unless a seed is given (tests).

`batch_verify_multi` / `batch_verify_multi_bytes` take a verifying key PER PROOF (`VerifyKeySet`, `plonk_verify_batch_multi_dev`) and fold
the batch on the device into a sum tree (`plonk_g1_sum_tree_dev`): the host pairs the root and bisects over tree nodes it reads back
(`bisect_tree`), with no point addition of its own.  The one-key functions keep the host fold.

The transcript labels of the two opening proofs and of u (b"open_proof", b"shifted_open_proof", b"u") are those of jf-plonk's verifier as
far as the public sources show; like the serialised `Proof` layout they are not pinned by a reference-generated proof.
"""
from __future__ import annotations

import ctypes as C
import random
import secrets
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from . import fr as _fr
from .transcript import FQ_MODULI, PlonkTranscript

NPTS, NEVALS = 13, 10
STATUS_BITS = {1: "point off the curve", 2: "point outside the r-subgroup", 4: "zeta in the evaluation domain", 8: "non-canonical encoding"}

_G1_GEN = {"bn254": (1, 2),
           "bls12_381": (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
                         0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)}


def _q64(curve: str) -> int:
    return _ffi.FQ_LIMBS64[_ffi.CURVES[curve]]


def _fq_mont(curve: str, x: int) -> list:
    q, n = FQ_MODULI[curve], _q64(curve)
    v = x * pow(2, 64 * n, q) % q
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)]


def g1_generator(curve: str) -> np.ndarray:
    x, y = _G1_GEN[curve]
    return np.array(_fq_mont(curve, x) + _fq_mont(curve, y), dtype=np.uint64)


def _g1_neg(curve: str, xy: np.ndarray) -> np.ndarray:
    n = _q64(curve)
    if not xy.any():
        return xy.copy()
    q = FQ_MODULI[curve]
    y = sum(int(v) << (64 * i) for i, v in enumerate(xy[n:]))
    ny = (q - y) % q
    return np.concatenate([xy[:n], np.array([(ny >> (64 * i)) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)])


def _point_xy(curve: str, pt) -> np.ndarray:
    """(xy limbs, is_infinity) as Prover / g1_to_affine return it -> x || y with (0, 0) for infinity."""
    xy, inf = pt
    return np.zeros(2 * _q64(curve), np.uint64) if inf else np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1)


def _lib():
    return _ffi.lib()


def g2_generator(curve: str) -> np.ndarray:
    out = np.zeros(4 * _q64(curve), np.uint64)
    _ffi.check(_lib().plonk_g2_generator(_ffi.CURVES[curve], out.ctypes.data))
    return out


def g2_mul(curve: str, scalar_mont, pt: np.ndarray) -> np.ndarray:
    s = np.ascontiguousarray(scalar_mont, dtype=np.uint64)
    pt = np.ascontiguousarray(pt, dtype=np.uint64)
    out = np.zeros(4 * _q64(curve), np.uint64)
    _ffi.check(_lib().plonk_g2_mul(_ffi.CURVES[curve], s.ctypes.data, pt.ctypes.data, out.ctypes.data))
    return out


def g2_check(curve: str, pt: np.ndarray) -> bool:
    pt = np.ascontiguousarray(pt, dtype=np.uint64)
    ok = C.c_int(0)
    _ffi.check(_lib().plonk_g2_check(_ffi.CURVES[curve], pt.ctypes.data, C.byref(ok)))
    return bool(ok.value)


def pairing_check(curve: str, g1_points: Sequence[np.ndarray], g2_points: Sequence[np.ndarray]) -> bool:
    """prod e(P_i, Q_i) == 1.  G1 as x || y, G2 as x.c0 || x.c1 || y.c0 || y.c1 (Montgomery limbs; all zero = infinity)."""
    a = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint64).reshape(-1) for p in g1_points]))
    b = np.ascontiguousarray(np.concatenate([np.asarray(q, np.uint64).reshape(-1) for q in g2_points]))
    r = C.c_int(0)
    _ffi.check(_lib().plonk_pairing_check(_ffi.CURVES[curve], len(g1_points), a.ctypes.data, b.ctypes.data, C.byref(r)))
    return bool(r.value)


class OpenKey:
    """jf-plonk's verifier parameters (UnivariateVerifierParam): g = [1]_1, h = [1]_2, beta_h = [tau]_2.  The G2 points are checked to lie
    on the twist in the order-r subgroup when the key is built."""

    def __init__(self, curve: str, g: np.ndarray, h: np.ndarray, beta_h: np.ndarray):
        self.curve = curve
        self.g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1)
        self.h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1)
        self.beta_h = np.ascontiguousarray(beta_h, dtype=np.uint64).reshape(-1)
        if not np.array_equal(self.g, g1_generator(curve)):
            raise ValueError("OpenKey: g must be the G1 generator the prover's commitments and the device verifier use")
        for name, pt in (("h", self.h), ("beta_h", self.beta_h)):
            if pt.shape != (4 * _q64(curve),) or not g2_check(curve, pt) or not pt.any():
                raise ValueError(f"OpenKey: {name} is not a point of order r on the twist")

    @classmethod
    def from_trapdoor(cls, curve: str, tau: int) -> "OpenKey":
        """The key matching `plonk_synth_srs` / `SyntheticInstance(tau=...)`: beta_h = tau * H."""
        h = g2_generator(curve)
        return cls(curve, g1_generator(curve), h, g2_mul(curve, _fr.FIELDS[curve].to_limbs(tau % _fr.FIELDS[curve].p), h))

    @classmethod
    def from_bytes(cls, curve: str, g: bytes, h: bytes, beta_h: bytes) -> "OpenKey":
        """The key from its three serialized elements (ark-serialize 0.3, compressed or uncompressed by their length): g a G1Affine, h and
        beta_h G2Affine (`plonk_g2_from_bytes`).  g has to be the generator, so it is compared as bytes; a G2 element that does not decode
        raises ValueError naming its status."""
        from . import codec
        xy = g1_generator(curve)
        if bytes(g) not in (codec.g1_encode_host(curve, xy, "compressed"), codec.g1_encode_host(curve, xy, "uncompressed")):
            raise ValueError("OpenKey: g must be the G1 generator the prover's commitments and the device verifier use")
        pts = []
        for name, blob in (("h", h), ("beta_h", beta_h)):
            pt, st = codec.g2_from_bytes(curve, blob)
            if st:
                raise ValueError(f"OpenKey: {name} does not decode: {codec.status_text(st)}")
            pts.append(pt)
        return cls(curve, xy, pts[0], pts[1])


def _jac(curve: str, xy: np.ndarray) -> np.ndarray:
    n = _q64(curve)
    one = np.array(_fq_mont(curve, 1), dtype=np.uint64)
    if not xy.any():
        return np.concatenate([one, one, np.zeros(n, np.uint64)])
    return np.concatenate([xy, one])


def _sum_points(worker, curve: str, pts: Sequence[np.ndarray]) -> np.ndarray:
    acc = _jac(curve, np.zeros(2 * _q64(curve), np.uint64))
    for p in pts:
        if p.any():
            acc = worker.g1_add(acc, _jac(curve, p))
    xy, inf = worker.g1_to_affine(acc)
    return np.zeros_like(xy) if inf else xy


def _vk_state(curve: str, vk: dict, num_inputs: int) -> _ffi.VerifyKey:
    t = PlonkTranscript(curve)
    t.append_vk_and_pub_input(vk["domain_size"], num_inputs, list(vk["k"]), vk["selector_comms"], vk["sigma_comms"], [])
    s = t.t.strobe
    key = _ffi.VerifyKey()
    key.domain_size = int(vk["domain_size"])
    key.num_inputs = num_inputs
    k = np.ascontiguousarray(vk["k"], dtype=np.uint64).reshape(5, 4)
    for i in range(5):
        for j in range(4):
            key.k[i][j] = int(k[i, j])
    key.transcript_state[:] = list(s.state)
    key.transcript_pos[:] = [s.pos, s.pos_begin, s.cur_flags]
    return key


def proof_record(curve: str, proof: dict) -> np.ndarray:
    """One `plonk_verify_batch_dev` record: 13 affine points in `Proof` field order, then the 10 evaluations."""
    pts = list(proof["wires_poly_comms"]) + [proof["prod_perm_poly_comm"]] + list(proof["split_quot_poly_comms"]) \
        + [proof["opening_proof"], proof["shifted_opening_proof"]]
    evs = list(proof["wires_evals"]) + list(proof["wire_sigma_evals"]) + [proof["perm_next_eval"]]
    if len(pts) != NPTS or len(evs) != NEVALS:
        raise ValueError("proof shape: 13 commitments and 10 evaluations expected")
    return np.concatenate([_point_xy(curve, p) for p in pts] + [np.ascontiguousarray(e, dtype=np.uint64).reshape(4) for e in evs])


def device_verify(worker, vk: dict, public_inputs_list, proofs, rho: np.ndarray, debug: bool = False):
    """The device part for K proofs: (points [K, 2 (rho B, rho A), 2Q] u64, status [K] u32, debug [K, 9, 4] or None)."""
    curve = worker.curve_name
    n64 = _q64(curve)
    K = len(proofs)
    if len(public_inputs_list) != K or rho.shape[0] != K:
        raise ValueError("one public-input list and one rho per proof")
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in public_inputs_list]
    num_inputs = pis[0].shape[0] if K else 0
    if any(p.shape[0] != num_inputs for p in pis):
        raise ValueError("every proof of a batch needs the same number of public inputs")
    recs = np.stack([proof_record(curve, p) for p in proofs]) if K else np.zeros((0, 2 * n64 * NPTS + 4 * NEVALS), np.uint64)
    pub = np.concatenate(pis) if num_inputs else np.zeros((1, 4), np.uint64)
    bufs = []
    try:
        for arr in (recs, pub):
            bufs.append(worker.alloc(max(arr.nbytes, 8)))
            bufs[-1].upload(arr)
        return device_verify_records(worker, vk, num_inputs, K, bufs[0].ptr, bufs[1].ptr, rho, debug)
    finally:
        for b in bufs:
            b.free()


def device_verify_records(worker, vk: dict, num_inputs: int, K: int, d_recs: int, d_pub: int, rho: np.ndarray, debug: bool = False):
    """What device_verify does after the upload: K proof records and K x num_inputs public inputs already on the device (pointers) ->
    (points, status, debug) as device_verify returns them."""
    curve = worker.curve_name
    n64 = _q64(curve)
    if len(vk["selector_comms"]) != 13 or len(vk["sigma_comms"]) != 5:
        raise ValueError("verifying key shape")
    key = _vk_state(curve, vk, num_inputs)
    comms = np.concatenate([_point_xy(curve, c) for c in list(vk["selector_comms"]) + list(vk["sigma_comms"])])
    bufs = []
    alloc = lambda nbytes: bufs.append(worker.alloc(max(nbytes, 8))) or bufs[-1]
    try:
        d_comms = alloc(comms.nbytes).upload(comms)
        d_rho = alloc(rho.nbytes).upload(np.ascontiguousarray(rho, dtype=np.uint64))
        d_out = alloc(K * 2 * 2 * n64 * 8)
        d_status = alloc(K * 4)
        d_dbg = alloc(K * 9 * 32) if debug else None
        if debug:
            worker.memset_dev(d_dbg.ptr, 0, K * 9 * 32)
        key.d_comms = d_comms.ptr
        _ffi.check(_lib().plonk_verify_batch_dev(worker.ctx, C.byref(key), K, d_recs, d_pub if num_inputs else None, d_rho.ptr, d_out.ptr,
                                                 d_status.ptr, d_dbg.ptr if debug else None))
        pts = d_out.download((K, 2, 2 * n64))
        status = d_status.download((K,), dtype=np.uint32)
        dbg = d_dbg.download((K, 9, 4)) if debug else None
    finally:
        for b in bufs:
            b.free()
    return pts, status, dbg


def _rhos(curve: str, K: int, seed: Optional[int]) -> np.ndarray:
    f = _fr.FIELDS[curve]
    draw = (lambda: secrets.randbelow(f.p - 1) + 1) if seed is None else (lambda r=random.Random(seed): r.randrange(1, f.p))
    return np.stack([f.to_limbs(draw()) for _ in range(K)]) if K else np.zeros((0, 4), np.uint64)


def batch_verify(worker, vk: dict, open_key: OpenKey, public_inputs_list, proofs, seed: Optional[int] = None, stats: Optional[dict] = None,
                 _rho: Optional[np.ndarray] = None) -> list:
    """One verdict per proof.  `stats` (a dict, optional) receives "pairing_checks" and the status word of every proof ("status")."""
    curve = worker.curve_name
    if open_key.curve != curve:
        raise ValueError("open key and worker are on different curves")
    K = len(proofs)
    rho = _rhos(curve, K, seed) if _rho is None else _rho
    pts, status, _ = device_verify(worker, vk, public_inputs_list, proofs, rho)
    verdict, checks = _bisect(worker, open_key, pts, [i for i in range(K) if status[i] == 0])
    if stats is not None:
        stats["pairing_checks"] = checks
        stats["status"] = [int(s) for s in status]
    return verdict


def _bisect(worker, open_key: OpenKey, pts: np.ndarray, eligible: list):
    """(verdicts, pairing checks): one folded pairing check over the eligible proofs, halved while it fails."""
    curve = worker.curve_name
    verdict = [False] * pts.shape[0]
    checks = [0]

    def holds(idx):
        checks[0] += 1
        b = _sum_points(worker, curve, [pts[i, 0] for i in idx])
        a = _sum_points(worker, curve, [pts[i, 1] for i in idx])
        return pairing_check(curve, [a, _g1_neg(curve, b)], [open_key.beta_h, open_key.h])

    def bisect(idx):
        if not idx:
            return
        if holds(idx):
            for i in idx:
                verdict[i] = True
        elif len(idx) > 1:
            bisect(idx[:len(idx) // 2])
            bisect(idx[len(idx) // 2:])

    bisect(list(eligible))
    return verdict, checks[0]


def batch_verify_bytes(worker, vk: dict, open_key: OpenKey, public_inputs_bytes, proof_blobs, seed: Optional[int] = None,
                       stats: Optional[dict] = None) -> list:
    """batch_verify on what a prover sends: proof_blobs[i] a serialized `Proof` (transcript.serialize_proof), public_inputs_bytes[i] its
    public inputs, 32 bytes each.  Proofs and inputs are decoded on the device (codec.proofs_from_bytes_dev, plonk_fr_from_bytes_dev) and the
    records go to plonk_verify_batch_dev where they are.  A proof that does not decode is rejected without touching the others; `stats`
    receives "decode_status" beside batch_verify's "pairing_checks" and "status"."""
    from . import codec
    curve = worker.curve_name
    if open_key.curve != curve:
        raise ValueError("open key and worker are on different curves")
    K = len(proof_blobs)
    if len(public_inputs_bytes) != K:
        raise ValueError("one public-input blob per proof")
    pubs = [bytes(p) for p in public_inputs_bytes]
    if any(len(p) % 32 or len(p) != len(pubs[0]) for p in pubs):
        raise ValueError("every proof of a batch needs the same number of public inputs, 32 bytes each")
    num_inputs = len(pubs[0]) // 32 if K else 0
    if K == 0:
        if stats is not None:
            stats.update(pairing_checks=0, status=[], decode_status=[])
        return []
    rho = _rhos(curve, K, seed)
    d_recs, decode = codec.proofs_from_bytes_dev(worker, proof_blobs)
    bufs = [d_recs]                              # everything allocated below is freed on every exit
    alloc = lambda nbytes: bufs.append(worker.alloc(nbytes)) or bufs[-1]
    try:
        d_pub = None
        if num_inputs:
            raw = np.frombuffer(b"".join(pubs), dtype=np.uint8)
            d_raw = alloc(raw.nbytes).upload(raw)
            d_pub = alloc(K * num_inputs * 32)
            d_st = alloc(K * num_inputs * 4)
            worker.memset_dev(d_st.ptr, 0, K * num_inputs * 4)
            worker.fr_from_bytes_dev(d_raw.ptr, 32, K * num_inputs, d_pub.ptr, 4, d_st.ptr, 1)
            decode = decode | np.bitwise_or.reduce(d_st.download((K, num_inputs), dtype=np.uint32), axis=1)
        pts, status, _ = device_verify_records(worker, vk, num_inputs, K, d_recs.ptr, d_pub.ptr if d_pub else 0, rho)
    finally:
        for b in bufs:
            b.free()
    verdict, checks = _bisect(worker, open_key, pts, [i for i in range(K) if decode[i] == 0 and status[i] == 0])
    if stats is not None:
        stats["pairing_checks"] = checks
        stats["status"] = [int(s) for s in status]
        stats["decode_status"] = [int(s) for s in decode]
    return verdict


def verify(worker, vk: dict, open_key: OpenKey, public_inputs, proof: dict, stats: Optional[dict] = None) -> bool:
    """One proof, the single check of jf-plonk's verify (rho = 1)."""
    one = _fr.FIELDS[worker.curve_name].to_limbs(1)[None, :]
    return batch_verify(worker, vk, open_key, [public_inputs], [proof], stats=stats, _rho=one)[0]


def check_srs(worker, open_key: OpenKey, count: int, seed: Optional[int] = None) -> bool:
    """The resident commit key P_0..P_count is powers of the tau in open_key.beta_h:
    e(sum rho_i P_(i+1), H) == e(sum rho_i P_i, beta H) over i < count, both sums by the resident-base MSM (plonk_msm_dev)."""
    curve = worker.curve_name
    f = _fr.FIELDS[curve]
    draw = (lambda: secrets.randbelow(f.p - 1) + 1) if seed is None else (lambda r=random.Random(seed): r.randrange(1, f.p))
    rho = np.array([[(x >> (64 * j)) & (2 ** 64 - 1) for j in range(4)] for x in (draw() for _ in range(count))], dtype=np.uint64)   # canonical
    d = worker.alloc(max(rho.nbytes, 8)).upload(rho)
    try:
        s0, inf0 = worker.g1_to_affine(worker.msm_dev(0, count, d.ptr))
        s1, inf1 = worker.g1_to_affine(worker.msm_dev(1, count + 1, d.ptr))
    finally:
        d.free()
    if inf0 or inf1:
        return False
    s0 = s0.reshape(-1)
    s1 = s1.reshape(-1)
    return pairing_check(curve, [s1, _g1_neg(curve, s0)], [open_key.h, open_key.beta_h])


# ------------------------------------------------------------------------------------------------ a key per proof, folded on the device
MULTI_STATUS_BITS = {**STATUS_BITS, 32: "key index out of range", 64: "public-input span out of range or of the wrong length"}
MAX_KEYS = 4096


class VerifyKeySet:
    """Verifying keys of several circuits, ready for `plonk_verify_batch_multi_dev`: every key's 18 commitments uploaded once (one buffer),
    its transcript state computed once, and the filled `plonk_verify_key` array.  A key is the dict `Prover.verifying_key()` returns; its
    public-input count is `vk["num_inputs"]` or `num_inputs[i]`.  `close()` frees the device buffer."""

    def __init__(self, worker, vks: Sequence[dict], num_inputs: Optional[Sequence[int]] = None):
        curve = worker.curve_name
        n64 = _q64(curve)
        vks = list(vks)
        if not 1 <= len(vks) <= MAX_KEYS:
            raise ValueError(f"{len(vks)} verifying keys: 1 .. {MAX_KEYS} per set")
        if num_inputs is not None and len(num_inputs) != len(vks):
            raise ValueError("one public-input count per verifying key")
        comms, counts = [], []
        for i, vk in enumerate(vks):
            if len(vk["selector_comms"]) != 13 or len(vk["sigma_comms"]) != 5 or len(vk["k"]) != 5:
                raise ValueError(f"verifying key shape (key {i})")
            pts = list(vk["selector_comms"]) + list(vk["sigma_comms"])
            for xy, _inf in pts:
                if np.asarray(xy).size != 2 * n64:
                    raise ValueError(f"verifying key {i} is not on {curve}: a commitment of {np.asarray(xy).size} limbs, {2 * n64} expected")
            m = num_inputs[i] if num_inputs is not None else vk.get("num_inputs")
            if m is None:
                raise ValueError(f"verifying key {i}: no public-input count (vk['num_inputs'] or num_inputs=)")
            counts.append(int(m))
            comms.append(np.concatenate([_point_xy(curve, c) for c in pts]))
        self.worker, self.curve, self.n_vks = worker, curve, len(vks)
        self.num_inputs = counts
        self.domain_sizes = [int(vk["domain_size"]) for vk in vks]
        self.keys = (_ffi.VerifyKey * len(vks))()
        self._comms = worker.alloc(len(vks) * 18 * 2 * n64 * 8).upload(np.concatenate(comms))
        for i, vk in enumerate(vks):
            key = _vk_state(curve, vk, counts[i])
            key.d_comms = self._comms.ptr + i * 18 * 2 * n64 * 8
            self.keys[i] = key

    def close(self):
        if self._comms is not None:
            self._comms.free()
            self._comms = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _key_set(worker, keys, vk_index, pis):
    """(VerifyKeySet, owned): a list of dicts is wrapped; a key without "num_inputs" takes the count of the first proof that names it."""
    if isinstance(keys, VerifyKeySet):
        if keys.curve != worker.curve_name:
            raise ValueError("key set and worker are on different curves")
        return keys, False
    keys = list(keys)
    counts = []
    for i, vk in enumerate(keys):
        m = vk.get("num_inputs")
        if m is None:
            m = next((pis[j].shape[0] for j, x in enumerate(vk_index) if int(x) == i), 0)
        counts.append(m)
    return VerifyKeySet(worker, keys, counts), True


def device_verify_multi(worker, keys: VerifyKeySet, vk_index, public_inputs_list, proofs, rho: np.ndarray, debug: bool = False, _offsets=None):
    """device_verify with a key per proof (`plonk_verify_batch_multi_dev`): proof j under keys[vk_index[j]] with its own list of public inputs.
    (points [K, 2 (rho B, rho A), 2Q] u64, status [K] u32, debug [K, 9, 4] or None).  An index >= n_vks and a list of the wrong length are
    verdicts (status 32 / 64), not errors.  _offsets (tests): the K + 1 offsets to pass in place of the running sum of the lists' lengths."""
    K = len(proofs)
    if len(public_inputs_list) != K or len(vk_index) != K or rho.shape[0] != K:
        raise ValueError("one key index, one public-input list and one rho per proof")
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in public_inputs_list]
    bufs = []
    try:
        ptrs = _upload_batch(worker, bufs, vk_index, pis, proofs, _offsets)
        return _multi_records(worker, keys, K, *ptrs, rho, debug)[:3]
    finally:
        for b in bufs:
            b.free()


def _upload_batch(worker, bufs: list, vk_index, pis, proofs, offsets=None):
    """Records, key indices, offsets and the concatenated public inputs of a batch on the device: (d_recs, d_idx, d_pub, d_off, pub_total),
    0 for an empty array.  The buffers are appended to bufs as they are allocated, for the caller to free."""
    curve = worker.curve_name
    K = len(proofs)
    recs = np.stack([proof_record(curve, p) for p in proofs]) if K else np.zeros((0, 2 * _q64(curve) * NPTS + 4 * NEVALS), np.uint64)
    pub = np.concatenate(pis + [np.zeros((0, 4), np.uint64)])
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pis])]).astype(np.uint64) if offsets is None else np.asarray(offsets, dtype=np.uint64)
    if off.shape != (K + 1,):
        raise ValueError("K + 1 offsets")
    ptrs = []
    for arr in (recs, np.asarray(vk_index, dtype=np.uint32), pub, off):
        if arr.nbytes:
            bufs.append(worker.alloc(arr.nbytes))
            bufs[-1].upload(arr)
        ptrs.append(bufs[-1].ptr if arr.nbytes else 0)
    return (*ptrs, pub.shape[0])


def _multi_records(worker, keys: VerifyKeySet, K: int, d_recs: int, d_idx: int, d_pub: int, d_off: int, pub_total: int, rho: np.ndarray,
                   debug: bool = False, extra_mask: Optional[np.ndarray] = None, tree: bool = False, kernel_ms: Optional[dict] = None):
    """The device part on buffers already there: (points, status, debug, d_tree).  With tree=True the sum tree over the output pairs, masked
    by the status words (OR extra_mask), stays on the device in d_tree (a DeviceBuffer the caller frees); None otherwise.  kernel_ms (a
    dict) receives the device time of the two entry points, "verify" and "tree" (plonk_last_kernel_ms: each read waits for its kernels)."""
    n64 = _q64(worker.curve_name)
    bufs = []
    alloc = lambda nbytes: bufs.append(worker.alloc(max(nbytes, 8))) or bufs[-1]
    d_tree = None
    try:
        d_rho = alloc(rho.nbytes).upload(np.ascontiguousarray(rho, dtype=np.uint64))
        d_out = alloc(K * 2 * 2 * n64 * 8)
        d_status = alloc(K * 4)
        d_dbg = alloc(K * 9 * 32) if debug else None
        if debug:
            worker.memset_dev(d_dbg.ptr, 0, K * 9 * 32)
        worker.verify_batch_multi_dev(keys.keys, keys.n_vks, K, d_recs, d_idx, d_pub if pub_total else 0, d_off, pub_total, d_rho.ptr, d_out.ptr, d_status.ptr,
                                      d_dbg.ptr if debug else 0)
        if kernel_ms is not None and K:
            kernel_ms["verify"] = worker.last_kernel_ms()
        status = None
        if tree and K:
            d_mask = d_status
            if extra_mask is not None:
                status = d_status.download((K,), dtype=np.uint32)
                d_mask = alloc(K * 4).upload(np.ascontiguousarray(status | extra_mask, dtype=np.uint32))
            d_tree = worker.alloc((2 * tree_leaves(K) - 1) * 2 * 2 * n64 * 8)
            worker.g1_sum_tree_dev(d_out.ptr, K, d_mask.ptr, d_tree.ptr)
            if kernel_ms is not None:
                kernel_ms["tree"] = worker.last_kernel_ms()
        pts = d_out.download((K, 2, 2 * n64))
        if status is None:
            status = d_status.download((K,), dtype=np.uint32)
        dbg = d_dbg.download((K, 9, 4)) if debug else None
    except BaseException:
        if d_tree is not None:
            d_tree.free()
        raise
    finally:
        for b in bufs:
            b.free()
    return pts, status, dbg, d_tree


def tree_leaves(K: int) -> int:
    """P of `plonk_g1_sum_tree_dev`: the next power of two >= K (1 for K <= 1)."""
    return 1 << max(K - 1, 0).bit_length()


def g1_sum_tree(worker, points: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """`plonk_g1_sum_tree_dev` on host arrays: points [K, 2, 2Q] u64 (mask [K] u32) -> the whole tree [2P - 1, 2, 2Q]."""
    n64 = _q64(worker.curve_name)
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2, 2 * n64)
    K = points.shape[0]
    if K == 0:
        worker.g1_sum_tree_dev(0, 0, 0, 0)
        return np.zeros((0, 2, 2 * n64), np.uint64)
    bufs = [worker.alloc(points.nbytes).upload(points), worker.alloc((2 * tree_leaves(K) - 1) * 4 * n64 * 8)]
    try:
        if mask is not None:
            bufs.append(worker.alloc(K * 4).upload(np.ascontiguousarray(mask, dtype=np.uint32).reshape(K)))
        worker.g1_sum_tree_dev(bufs[0].ptr, K, bufs[2].ptr if mask is not None else 0, bufs[1].ptr)
        return bufs[1].download((2 * tree_leaves(K) - 1, 2, 2 * n64))
    finally:
        for b in bufs:
            b.free()


def bisect_tree(P: int, live: Sequence[bool], holds) -> tuple:
    """The positional bisection over a heap-ordered sum tree of P leaves (a power of two): (verdict per leaf, calls of holds).

    live[j] says that leaf j takes part (a masked leaf does not: it is rejected, and its point is infinity in every sum above it);
    holds(node) says whether the folded check holds for the sum at `node`.  The root is tested; a node that holds accepts every live leaf
    below it, a node that fails descends to both children, a failing leaf is rejected.  A subtree without live leaves is never tested, and
    neither is a node whose verdict is already known: when a node fails and its left child holds (or has no live leaf), the right child
    carries the failure.  So b bad leaves cost at most 1 + 2 b log2 P calls, an all-good batch one, a batch with no live leaf none."""
    assert P >= 1 and P & (P - 1) == 0 and len(live) <= P
    count = [0] * (2 * P - 1)
    for j, l in enumerate(live):
        count[P - 1 + j] = 1 if l else 0
    for i in range(P - 2, -1, -1):
        count[i] = count[2 * i + 1] + count[2 * i + 2]
    verdict = [False] * len(live)
    calls = [0]

    def accept(node):
        if node >= P - 1:
            if count[node]:
                verdict[node - (P - 1)] = True
        elif count[node]:
            accept(2 * node + 1)
            accept(2 * node + 2)

    def visit(node, known_bad):
        if not count[node]:
            return True                                       # nothing below: its sum is infinity, which holds
        if not known_bad:
            calls[0] += 1
            if holds(node):
                accept(node)
                return True
        if node < P - 1:
            left_ok = visit(2 * node + 1, False)
            visit(2 * node + 2, left_ok)                      # this node failed: if the left sum holds, the right one cannot
        return False

    visit(0, False)
    return verdict, calls[0]


def _bisect_on_device_tree(worker, open_key: OpenKey, d_tree, K: int, live: Sequence[bool]):
    curve = worker.curve_name
    pair_bytes = 2 * 2 * _q64(curve) * 8

    def holds(node):                                          # one node read back: [sum rho B, sum rho A]
        b, a = d_tree.download((2, 2 * _q64(curve)), byte_offset=node * pair_bytes)
        return pairing_check(curve, [a, _g1_neg(curve, b)], [open_key.beta_h, open_key.h])

    return bisect_tree(tree_leaves(K), live, holds)


def batch_verify_multi(worker, keys, open_key: OpenKey, vk_index, public_inputs_list, proofs, seed: Optional[int] = None,
                       stats: Optional[dict] = None, _rho: Optional[np.ndarray] = None) -> list:
    """jf-plonk's batch_verify: one verdict per proof, proof j checked under keys[vk_index[j]] (a VerifyKeySet, or a list of key dicts
    wrapped and closed here) with public_inputs_list[j].  The device computes every proof's pair (`plonk_verify_batch_multi_dev`) and folds
    the batch into a sum tree (`plonk_g1_sum_tree_dev`, masked by the status words); the host pairs the root and, if that fails, bisects over
    tree nodes read back one at a time (bisect_tree) — no point addition on the host.  `stats` receives "pairing_checks", "status" and
    "kernel_ms" (the device time of the two entry points)."""
    curve = worker.curve_name
    if open_key.curve != curve:
        raise ValueError("open key and worker are on different curves")
    K = len(proofs)
    if len(vk_index) != K or len(public_inputs_list) != K:
        raise ValueError("one key index and one public-input list per proof")
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in public_inputs_list]
    keyset, owned = _key_set(worker, keys, vk_index, pis)
    bufs, d_tree = [], None
    kms = {} if stats is not None else None
    try:
        if K == 0:
            status, verdict, checks = np.zeros((0,), np.uint32), [], 0
        else:
            rho = _rhos(curve, K, seed) if _rho is None else _rho
            ptrs = _upload_batch(worker, bufs, vk_index, pis, proofs)
            _, status, _, d_tree = _multi_records(worker, keyset, K, *ptrs, rho, tree=True, kernel_ms=kms)
            verdict, checks = _bisect_on_device_tree(worker, open_key, d_tree, K, [s == 0 for s in status])
    finally:
        for b in bufs + [d_tree]:
            if b:
                b.free()
        if owned:
            keyset.close()
    if stats is not None:
        stats["pairing_checks"] = checks
        stats["status"] = [int(s) for s in status]
        stats["kernel_ms"] = kms
    return verdict


def batch_verify_multi_bytes(worker, keys, open_key: OpenKey, vk_index, public_inputs_bytes, proof_blobs, seed: Optional[int] = None,
                             stats: Optional[dict] = None) -> list:
    """batch_verify_multi on what provers send: proof_blobs[j] a serialized `Proof`, public_inputs_bytes[j] its public inputs, 32 bytes each
    and as many as ITS circuit has (blobs of different lengths; one that is no multiple of 32 bytes is a ValueError).  Proofs are decoded by
    codec.proofs_from_bytes_dev and all inputs by ONE plonk_fr_from_bytes_dev launch over their concatenation; a proof or an input that does
    not decode masks its proof out of the fold and rejects it without touching the others.  `stats` receives "decode_status" beside
    "pairing_checks" and "status"."""
    from . import codec
    curve = worker.curve_name
    if open_key.curve != curve:
        raise ValueError("open key and worker are on different curves")
    K = len(proof_blobs)
    if len(public_inputs_bytes) != K or len(vk_index) != K:
        raise ValueError("one key index and one public-input blob per proof")
    pubs = [bytes(p) for p in public_inputs_bytes]
    if any(len(p) % 32 for p in pubs):
        raise ValueError("public inputs are 32 bytes each")
    counts = [len(p) // 32 for p in pubs]
    keyset, owned = _key_set(worker, keys, vk_index, [np.zeros((c, 4), np.uint64) for c in counts])
    bufs, d_tree = [], None
    kms = {} if stats is not None else None
    alloc = lambda nbytes: bufs.append(worker.alloc(nbytes)) or bufs[-1]
    try:
        if K == 0:
            status, decode, verdict, checks = np.zeros((0,), np.uint32), np.zeros((0,), np.uint32), [], 0
        else:
            rho = _rhos(curve, K, seed)
            d_recs, decode = codec.proofs_from_bytes_dev(worker, proof_blobs)
            bufs.append(d_recs)
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
            total = int(off[-1])
            d_idx = alloc(K * 4).upload(np.asarray(vk_index, dtype=np.uint32))
            d_off = alloc((K + 1) * 8).upload(off)
            d_pub = None
            if total:
                raw = np.frombuffer(b"".join(pubs), dtype=np.uint8)
                d_raw = alloc(raw.nbytes).upload(raw)
                d_pub = alloc(total * 32)
                d_st = alloc(total * 4)
                worker.memset_dev(d_st.ptr, 0, total * 4)
                worker.fr_from_bytes_dev(d_raw.ptr, 32, total, d_pub.ptr, 4, d_st.ptr, 1)
                st = d_st.download((total,), dtype=np.uint32)
                decode = decode | np.array([np.bitwise_or.reduce(st[int(off[j]):int(off[j + 1])], initial=0) for j in range(K)], dtype=np.uint32)
            decode = np.ascontiguousarray(decode, dtype=np.uint32)
            _, status, _, d_tree = _multi_records(worker, keyset, K, d_recs.ptr, d_idx.ptr, d_pub.ptr if d_pub else 0, d_off.ptr, total, rho,
                                                  extra_mask=decode, tree=True, kernel_ms=kms)
            verdict, checks = _bisect_on_device_tree(worker, open_key, d_tree, K, [s == 0 and d == 0 for s, d in zip(status, decode)])
    finally:
        for b in bufs + [d_tree]:
            if b:
                b.free()
        if owned:
            keyset.close()
    if stats is not None:
        stats["pairing_checks"] = checks
        stats["status"] = [int(s) for s in status]
        stats["decode_status"] = [int(s) for s in decode]
        stats["kernel_ms"] = kms
    return verdict
