"""Verifying proofs without the SRS trapdoor: jf-plonk's `verify` / `batch_verify` (the pairing check e(A, [tau]_2) = e(B, [1]_2)).

The per-proof work runs on the device, all proofs of a batch in parallel (`plonk_verify_batch_dev`): input checks, the Fiat-Shamir replay,
the ~30 scalars of the linearised check and the two multi-scalar sums rho_k * A_k, rho_k * B_k with

    A = W_zeta + u W_zeta_omega,   B = zeta W_zeta + u zeta w W_zeta_omega + F + u [z] - (E + u z(zeta w)) G.

The device folds the K pairs into a sum tree (`plonk_g1_sum_tree_dev`); the host reads the root back and runs ONE two-pairing check
e(sum rho A, beta H) * e(-sum rho B, H) == 1 (`plonk_pairing_check`).  A failed batch is bisected over tree nodes read back one at a time
(`bisect_tree`), with no point addition on the host, so f bad proofs cost O(f log K) pairing checks.  rho_k are drawn from `secrets`
unless a seed is given (tests).

`batch_verify_multi` / `batch_verify_multi_bytes` take a verifying key PER PROOF (`VerifyKeySet`, `plonk_verify_batch_multi_dev`); the
`_bytes` functions take serialized proofs and public inputs and decode them on the device.  All four batch functions are one sequence of
stages — the batch on the device, the per-proof pairs, the fold (`_fold`) — and differ in where the records come from and in which of the
two per-proof entry points they launch.

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
from .worker import DeviceScope, closing_on_error

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


def _alloc(bufs: DeviceScope, nbytes: int):
    return bufs.alloc(max(nbytes, 8))


def _upload(bufs: DeviceScope, arr: np.ndarray) -> int:
    """The array in a buffer of its own: the device pointer, 0 for an empty array (nothing is allocated for one)."""
    return _alloc(bufs, arr.nbytes).upload(arr).ptr if arr.nbytes else 0


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
    K = len(proofs)
    pis, num_inputs = _one_key_inputs(K, public_inputs_list, rho)
    with DeviceScope(worker) as bufs:
        d_recs, d_pub = _upload_batch(bufs, proofs, pis)
        return device_verify_records(worker, vk, num_inputs, K, d_recs, d_pub, rho, debug)


def device_verify_records(worker, vk: dict, num_inputs: int, K: int, d_recs: int, d_pub: int, rho: np.ndarray, debug: bool = False):
    """What device_verify does after the upload: K proof records and K x num_inputs public inputs already on the device (pointers) ->
    (points, status, debug) as device_verify returns them."""
    with DeviceScope(worker) as bufs:
        return _download_pairs(K, *_launch_pairs(bufs, K, rho, debug, _one_key_launch(bufs, vk, num_inputs, K, d_recs, d_pub)))


# ------------------------------------------------------------------------------------------------ the stages every entry point shares
def _one_key_inputs(K: int, public_inputs_list, rho: np.ndarray):
    """(public inputs as [m, 4] arrays, m): the one-key entry point wants the same count m under every proof."""
    if len(public_inputs_list) != K or rho.shape[0] != K:
        raise ValueError("one public-input list and one rho per proof")
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in public_inputs_list]
    num_inputs = pis[0].shape[0] if K else 0
    if any(p.shape[0] != num_inputs for p in pis):
        raise ValueError("every proof of a batch needs the same number of public inputs")
    return pis, num_inputs


def _upload_batch(bufs: DeviceScope, proofs, pis, *more):
    """A batch of proof dicts on the device: the pointers of the records, of the concatenated public inputs and of every array of `more`
    (key indices, offsets), 0 for an empty array."""
    curve = bufs.worker.curve_name
    recs = np.stack([proof_record(curve, p) for p in proofs]) if len(proofs) else np.zeros((0, 2 * _q64(curve) * NPTS + 4 * NEVALS), np.uint64)
    return [_upload(bufs, arr) for arr in (recs, np.concatenate(pis + [np.zeros((0, 4), np.uint64)]), *more)]


def _decode_batch(bufs: DeviceScope, public_inputs_bytes: Sequence[bytes], proof_blobs):
    """A batch as provers send it, decoded on the device: the proofs as codec.proofs_from_bytes_dev does, their records in a buffer of
    `bufs`, all public inputs (32 bytes each, any number per proof) by ONE plonk_fr_from_bytes_dev launch over their concatenation.  (d_recs, d_pub or 0, the K + 1 offsets of the proofs'
    spans in d_pub, decode [K] u32): decode[j] ORs the codec's status words of proof j and of its inputs."""
    from . import codec
    worker, K = bufs.worker, len(proof_blobs)
    d_recs, decode = codec._proofs_into(bufs, proof_blobs)
    off = np.concatenate([[0], np.cumsum([len(p) // 32 for p in public_inputs_bytes])]).astype(np.uint64)
    total = int(off[-1])
    d_pub = 0
    if total:
        d_raw = _upload(bufs, np.frombuffer(b"".join(public_inputs_bytes), dtype=np.uint8))
        d_pub = _alloc(bufs, total * 32).ptr
        d_st = _alloc(bufs, total * 4)
        worker.memset_dev(d_st.ptr, 0, total * 4)
        worker.fr_from_bytes_dev(d_raw, 32, total, d_pub, 4, d_st.ptr, 1)
        st = d_st.download((total,), dtype=np.uint32)
        decode = decode | np.array([np.bitwise_or.reduce(st[int(off[j]):int(off[j + 1])], initial=0) for j in range(K)], dtype=np.uint32)
    return d_recs.ptr, d_pub, off, np.ascontiguousarray(decode, dtype=np.uint32)


def _one_key_launch(bufs: DeviceScope, vk: dict, num_inputs: int, K: int, d_recs: int, d_pub: int):
    """The launch of `plonk_verify_batch_dev` under vk for _launch_pairs, the key's 18 commitments uploaded.  A key of the wrong shape raises."""
    curve = bufs.worker.curve_name
    if len(vk["selector_comms"]) != 13 or len(vk["sigma_comms"]) != 5:
        raise ValueError("verifying key shape")
    key = _vk_state(curve, vk, num_inputs)
    key.d_comms = _upload(bufs, np.concatenate([_point_xy(curve, c) for c in list(vk["selector_comms"]) + list(vk["sigma_comms"])]))
    return lambda *outputs: bufs.worker.verify_batch_dev(key, K, d_recs, d_pub if num_inputs else 0, *outputs)


def _multi_launch(worker, keys: "VerifyKeySet", K: int, d_recs: int, d_idx: int, d_pub: int, d_off: int, pub_total: int):
    """The launch of `plonk_verify_batch_multi_dev` for _launch_pairs: proof j under keys[idx[j]] on its span of the public inputs."""
    return lambda *outputs: worker.verify_batch_multi_dev(keys.keys, keys.n_vks, K, d_recs, d_idx, d_pub if pub_total else 0, d_off, pub_total, *outputs)


def _launch_pairs(bufs: DeviceScope, K: int, rho: np.ndarray, debug: bool, launch):
    """The per-proof kernels, enqueued: rho uploaded, the buffers of the K output pairs [rho B, rho A], the K status words and (debug) the
    K x 9 intermediate scalars allocated, and launch(d_rho, d_out, d_status, d_debug or 0) called on their pointers.  (d_out, d_status,
    d_debug or None): DeviceBuffers that bufs owns."""
    d_rho = _upload(bufs, np.ascontiguousarray(rho, dtype=np.uint64))
    d_out = _alloc(bufs, K * 2 * 2 * _q64(bufs.worker.curve_name) * 8)
    d_status = _alloc(bufs, K * 4)
    d_dbg = _alloc(bufs, K * 9 * 32) if debug else None
    if debug:
        bufs.worker.memset_dev(d_dbg.ptr, 0, K * 9 * 32)
    launch(d_rho, d_out.ptr, d_status.ptr, d_dbg.ptr if debug else 0)
    return d_out, d_status, d_dbg


def _download_pairs(K: int, d_out, d_status, d_dbg):
    """(points [K, 2, 2Q] u64, status [K] u32, debug [K, 9, 4] or None) as the device_verify functions return them."""
    return d_out.download((K, 2, d_out.worker.q64 * 2)), d_status.download((K,), dtype=np.uint32), d_dbg.download((K, 9, 4)) if d_dbg else None


def _rhos(curve: str, K: int, seed: Optional[int]) -> np.ndarray:
    f = _fr.FIELDS[curve]
    draw = (lambda: secrets.randbelow(f.p - 1) + 1) if seed is None else (lambda r=random.Random(seed): r.randrange(1, f.p))
    return np.stack([f.to_limbs(draw()) for _ in range(K)]) if K else np.zeros((0, 4), np.uint64)


def check_srs(worker, open_key: OpenKey, count: int, seed: Optional[int] = None) -> bool:
    """The resident commit key P_0..P_count is powers of the tau in open_key.beta_h:
    e(sum rho_i P_(i+1), H) == e(sum rho_i P_i, beta H) over i < count, both sums by the resident-base MSM (plonk_msm_dev)."""
    curve = worker.curve_name
    f = _fr.FIELDS[curve]
    draw = (lambda: secrets.randbelow(f.p - 1) + 1) if seed is None else (lambda r=random.Random(seed): r.randrange(1, f.p))
    rho = np.array([[(x >> (64 * j)) & (2 ** 64 - 1) for j in range(4)] for x in (draw() for _ in range(count))], dtype=np.uint64)   # canonical
    with DeviceScope(worker) as bufs:
        d = _alloc(bufs, rho.nbytes).upload(rho)
        s0, inf0 = worker.g1_to_affine(worker.msm_dev(0, count, d.ptr))
        s1, inf1 = worker.g1_to_affine(worker.msm_dev(1, count + 1, d.ptr))
    if inf0 or inf1:
        return False
    s0 = s0.reshape(-1)
    s1 = s1.reshape(-1)
    return pairing_check(curve, [s1, _g1_neg(curve, s0)], [open_key.h, open_key.beta_h])


# ------------------------------------------------------------------------------------------------ a key per proof
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
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            d_comms = self._scope.alloc(len(vks) * 18 * 2 * n64 * 8).upload(np.concatenate(comms))
            for i, vk in enumerate(vks):
                key = _vk_state(curve, vk, counts[i])
                key.d_comms = d_comms.ptr + i * 18 * 2 * n64 * 8
                self.keys[i] = key

    def close(self):
        self._scope.close()

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
    with DeviceScope(worker) as bufs:
        launch = _multi_launch(worker, keys, K, *_upload_multi(bufs, vk_index, pis, proofs, _offsets))
        return _download_pairs(K, *_launch_pairs(bufs, K, rho, debug, launch))


def _upload_multi(bufs: DeviceScope, vk_index, pis, proofs, offsets=None):
    """_upload_batch with the key indices and the K + 1 offsets of the ragged public-input list: (d_recs, d_idx, d_pub, d_off, pub_total)."""
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pis])]).astype(np.uint64) if offsets is None else np.asarray(offsets, dtype=np.uint64)
    if off.shape != (len(proofs) + 1,):
        raise ValueError("K + 1 offsets")
    d_recs, d_pub, d_idx, d_off = _upload_batch(bufs, proofs, pis, np.asarray(vk_index, dtype=np.uint32), off)
    return d_recs, d_idx, d_pub, d_off, sum(p.shape[0] for p in pis)


# ------------------------------------------------------------------------------------------------ the fold on the device, and the batch functions
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
    with DeviceScope(worker) as bufs:
        d_mask = _upload(bufs, np.ascontiguousarray(mask, dtype=np.uint32).reshape(K)) if mask is not None else 0
        d_tree = _alloc(bufs, (2 * tree_leaves(K) - 1) * 4 * n64 * 8)
        worker.g1_sum_tree_dev(_upload(bufs, points), K, d_mask, d_tree.ptr)
        return d_tree.download((2 * tree_leaves(K) - 1, 2, 2 * n64))


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


def _fold(bufs: DeviceScope, open_key: OpenKey, K: int, rho: np.ndarray, launch, decode: Optional[np.ndarray], stats: Optional[dict]) -> list:
    """The fold of every batch function, and the one place that fills `stats`: the per-proof pairs (_launch_pairs), the sum tree over
    them (`plonk_g1_sum_tree_dev`) masked by the status words — ORed with the decode words of the bytes route, where a proof that did not
    decode has to stay out of every sum —, and the bisection over its nodes.  Only status words and tree nodes are read back, never the K
    pairs.  An empty batch launches nothing.  "kernel_ms" is the device time of the two entry points (plonk_last_kernel_ms: each read
    waits for its kernels, so it is read only when stats are asked for)."""
    worker = bufs.worker
    status, verdict, checks = np.zeros((0,), np.uint32), [], 0
    kms = {} if stats is not None else None
    if K:
        d_out, d_status, _ = _launch_pairs(bufs, K, rho, False, launch)
        if kms is not None:
            kms["verify"] = worker.last_kernel_ms()
        d_mask, mask = d_status, None
        if decode is not None:
            status = d_status.download((K,), dtype=np.uint32)
            mask = status | decode
            d_mask = _alloc(bufs, K * 4).upload(mask)
        d_tree = _alloc(bufs, (2 * tree_leaves(K) - 1) * 2 * 2 * _q64(worker.curve_name) * 8)
        worker.g1_sum_tree_dev(d_out.ptr, K, d_mask.ptr, d_tree.ptr)
        if kms is not None:
            kms["tree"] = worker.last_kernel_ms()
        if mask is None:                                      # the tree is masked by the status words where they are: read them behind it
            mask = status = d_status.download((K,), dtype=np.uint32)
        verdict, checks = _bisect_on_device_tree(worker, open_key, d_tree, K, [m == 0 for m in mask])
    if stats is not None:
        stats["pairing_checks"] = checks
        stats["status"] = [int(s) for s in status]
        stats["kernel_ms"] = kms
        if decode is not None:
            stats["decode_status"] = [int(s) for s in decode]
    return verdict


def _curve(worker, open_key: OpenKey) -> str:
    if open_key.curve != worker.curve_name:
        raise ValueError("open key and worker are on different curves")
    return worker.curve_name


def batch_verify(worker, vk: dict, open_key: OpenKey, public_inputs_list, proofs, seed: Optional[int] = None, stats: Optional[dict] = None,
                 _rho: Optional[np.ndarray] = None) -> list:
    """One verdict per proof, all proofs under one verifying key with the same number of public inputs (another count is a ValueError).
    `stats` (a dict, optional) receives "pairing_checks", the status word of every proof ("status") and "kernel_ms" (the device time of
    the two entry points, "verify" and "tree")."""
    curve = _curve(worker, open_key)
    K = len(proofs)
    rho = _rhos(curve, K, seed) if _rho is None else _rho
    pis, num_inputs = _one_key_inputs(K, public_inputs_list, rho)
    with DeviceScope(worker) as bufs:
        d_recs, d_pub = _upload_batch(bufs, proofs, pis)
        return _fold(bufs, open_key, K, rho, _one_key_launch(bufs, vk, num_inputs, K, d_recs, d_pub), None, stats)


def batch_verify_bytes(worker, vk: dict, open_key: OpenKey, public_inputs_bytes, proof_blobs, seed: Optional[int] = None,
                       stats: Optional[dict] = None) -> list:
    """batch_verify on what a prover sends: proof_blobs[i] a serialized `Proof` (transcript.serialize_proof), public_inputs_bytes[i] its
    public inputs, 32 bytes each.  Proofs and inputs are decoded on the device (_decode_batch) and the records go to plonk_verify_batch_dev
    where they are.  A proof or an input that does not decode masks its proof out of the fold and rejects it without touching the others;
    `stats` receives "decode_status" beside batch_verify's "pairing_checks", "status" and "kernel_ms"."""
    curve = _curve(worker, open_key)
    K = len(proof_blobs)
    if len(public_inputs_bytes) != K:
        raise ValueError("one public-input blob per proof")
    pubs = [bytes(p) for p in public_inputs_bytes]
    if any(len(p) % 32 or len(p) != len(pubs[0]) for p in pubs):
        raise ValueError("every proof of a batch needs the same number of public inputs, 32 bytes each")
    num_inputs = len(pubs[0]) // 32 if K else 0
    with DeviceScope(worker) as bufs:
        d_recs, d_pub, _, decode = _decode_batch(bufs, pubs, proof_blobs)
        launch = _one_key_launch(bufs, vk, num_inputs, K, d_recs, d_pub) if K else None     # an empty batch does not look at the key
        return _fold(bufs, open_key, K, _rhos(curve, K, seed), launch, decode, stats)


def verify(worker, vk: dict, open_key: OpenKey, public_inputs, proof: dict, stats: Optional[dict] = None) -> bool:
    """One proof, the single check of jf-plonk's verify (rho = 1)."""
    one = _fr.FIELDS[worker.curve_name].to_limbs(1)[None, :]
    return batch_verify(worker, vk, open_key, [public_inputs], [proof], stats=stats, _rho=one)[0]


def batch_verify_multi(worker, keys, open_key: OpenKey, vk_index, public_inputs_list, proofs, seed: Optional[int] = None,
                       stats: Optional[dict] = None, _rho: Optional[np.ndarray] = None) -> list:
    """jf-plonk's batch_verify: one verdict per proof, proof j checked under keys[vk_index[j]] (a VerifyKeySet, or a list of key dicts
    wrapped and closed here) with public_inputs_list[j].  A key index out of range and a list of another length than its key's count are
    verdicts (status 32 / 64), not errors.  `stats` receives "pairing_checks", "status" and "kernel_ms" as batch_verify's does."""
    curve = _curve(worker, open_key)
    K = len(proofs)
    if len(vk_index) != K or len(public_inputs_list) != K:
        raise ValueError("one key index and one public-input list per proof")
    pis = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in public_inputs_list]
    keyset, owned = _key_set(worker, keys, vk_index, pis)
    try:
        with DeviceScope(worker) as bufs:
            rho = _rhos(curve, K, seed) if _rho is None else _rho
            return _fold(bufs, open_key, K, rho, _multi_launch(worker, keyset, K, *_upload_multi(bufs, vk_index, pis, proofs)), None, stats)
    finally:
        if owned:
            keyset.close()


def batch_verify_multi_bytes(worker, keys, open_key: OpenKey, vk_index, public_inputs_bytes, proof_blobs, seed: Optional[int] = None,
                             stats: Optional[dict] = None) -> list:
    """batch_verify_multi on what provers send: proof_blobs[j] a serialized `Proof`, public_inputs_bytes[j] its public inputs, 32 bytes each
    and as many as ITS circuit has (blobs of different lengths; one that is no multiple of 32 bytes is a ValueError).  Decoded on the device
    as in batch_verify_bytes, which is this with spans of one length; `stats` receives "decode_status" beside "pairing_checks", "status"
    and "kernel_ms"."""
    curve = _curve(worker, open_key)
    K = len(proof_blobs)
    if len(public_inputs_bytes) != K or len(vk_index) != K:
        raise ValueError("one key index and one public-input blob per proof")
    pubs = [bytes(p) for p in public_inputs_bytes]
    if any(len(p) % 32 for p in pubs):
        raise ValueError("public inputs are 32 bytes each")
    keyset, owned = _key_set(worker, keys, vk_index, [np.zeros((len(p) // 32, 4), np.uint64) for p in pubs])
    try:
        with DeviceScope(worker) as bufs:
            d_recs, d_pub, off, decode = _decode_batch(bufs, pubs, proof_blobs)
            d_idx, d_off = _upload(bufs, np.asarray(vk_index, dtype=np.uint32)), _upload(bufs, off)
            launch = _multi_launch(worker, keyset, K, d_recs, d_idx, d_pub, d_off, int(off[-1]))
            return _fold(bufs, open_key, K, _rhos(curve, K, seed), launch, decode, stats)
    finally:
        if owned:
            keyset.close()

