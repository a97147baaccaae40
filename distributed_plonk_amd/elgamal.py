"""Public-key encryption to a point of the embedded Edwards curve, computed on the device and provable in a circuit: the ElGamal / Rescue
hybrid in jellyfish's structure (csrc/elgamal_kernels.hpp behind plonk_edwards_dh_key_dev and plonk_rescue_stream_dev, over edwards.py's
plonk_edwards_fixed_mul_dev and plonk_edwards_check_dev), as the Schnorr half of edwards.py is for signatures.  jf-rescue's constants and
its byte encodings of keys and ciphertexts are not pinned here; the parameters are injectable, the structure is the one below.

Over the EdwardsParams and RescueParams of one curve, with permute, hash3 and the counter-mode stream of rescue.py (the capacity carries the
domain: hash3 uses 0, the sponge L, the stream -1):

    keys       the decryption key is a scalar dk, the encryption key the point ek = [dk] G
    encrypt(ek, m[0 : L], r),  0 <= r < l:      E = [r] G,   S = [r] ek,   k = hash3(S.x, S.y, 0),
                                                ct_i = m_i + ks_{i div 3}[i mod 3]   with   ks_j = permute((k, j, 0, -1))[0 : 3]
                                                the ciphertext is (E, ct)
    decrypt(dk, (E, ct)):                       S = [dk] E,  the same k,   m_i = ct_i - ks_{i div 3}[i mod 3],
                                                and a verdict per ciphertext: E is on the curve and in the subgroup of order l

A decryption whose E is not in the subgroup is FLAGGED, not refused: the messages come back with ok = False.  An E off the curve is taken
for the identity before it is multiplied (plonk_edwards_dh_key_dev does that itself), and its messages are unspecified.  There is no
authentication: whoever changes ct_i changes m_i by as much.  The randomness r is the caller's: fresh and secret per ciphertext.

A point crosses this module affine, (.., 2, 4) uint64; a scalar is a field element, (.., 4) Montgomery limbs, and stands for its canonical
residue, as everywhere in edwards.py; a message or ciphertext is (count, L, 4).  What the circuit of `elgamal_circuit` does and does not prove
stands in builder.CircuitBuilder.elgamal_encrypt.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import edwards as _ed
from . import rescue as _rescue
from .builder import BuiltCircuit, CircuitBuilder
from .edwards import EdwardsParams
from .worker import DeviceScope, PlonkWorker

keygen = _ed.fixed_mul                                # ek = [dk] G: (count, 4) -> (count, 2, 4)


def _texts(a, what: str) -> np.ndarray:
    x = np.ascontiguousarray(a, dtype=np.uint64)
    if x.ndim != 3 or x.shape[2] != 4 or x.shape[1] == 0:
        raise ValueError(f"{what}: shape {x.shape}, expected (count, L, 4) with L >= 1")
    return x


# ---------------------------------------------------------------------------------------------- device pointers in, device pointers out
def dh_key_dev(worker: PlonkWorker, params: EdwardsParams, rescue, d_scalars: int, d_points: int, count: int, d_keys: int):
    """d_keys[i] = hash3(S.x, S.y, 0) for S = [scalars[i]] points[i]: two launches (the multiplication, the permutation) with the shared
    points in a context-owned buffer between them.  Ordered on the worker's stream, not synchronised."""
    _ed._check(worker, params)
    worker.edwards_dh_key_dev(params.limbs(), _ed._rescue_params(params, rescue).limbs(), d_scalars, d_points, count, d_keys)


def encrypt_dev(worker: PlonkWorker, params: EdwardsParams, d_ek: int, d_msg: int, d_r: int, L: int, count: int, d_E: int, d_ct: int, d_keys: int, rescue=None):
    """d_E[i] = [r_i] G and d_ct[i][0 : L] = the encryption of d_msg[i][0 : L] under d_ek[i]: fixed_mul_dev, dh_key_dev and rescue.stream_dev
    enqueued one behind the other on the worker's stream, with no host round trip in between and no synchronisation.  d_keys: count Fr of
    working space (it receives the stream keys: wipe or free it).  d_ct may be d_msg.  The caller vouches for r < l and for ek."""
    _ed._check(worker, params)
    rp = _ed._rescue_params(params, rescue)
    _ed.fixed_mul_dev(worker, params, d_r, count, d_E)
    dh_key_dev(worker, params, rp, d_r, d_ek, count, d_keys)
    _rescue.stream_dev(worker, rp, d_keys, d_msg, L, count, d_ct, decrypt=False)


def decrypt_dev(worker: PlonkWorker, params: EdwardsParams, d_dk: int, d_E: int, d_ct: int, L: int, count: int, d_msg: int, d_flags: int, d_keys: int, rescue=None):
    """d_msg[i][0 : L] = the decryption of (d_E[i], d_ct[i][0 : L]) under d_dk[i], and d_flags[i] (u32) = edwards.ON_CURVE | IN_SUBGROUP as they
    hold for E_i: check_dev, dh_key_dev and rescue.stream_dev enqueued one behind the other, no host round trip in between, not synchronised.
    d_keys: count Fr of working space.  d_msg may be d_ct."""
    _ed._check(worker, params)
    rp = _ed._rescue_params(params, rescue)
    _ed.check_dev(worker, params, d_E, count, d_flags)
    dh_key_dev(worker, params, rp, d_dk, d_E, count, d_keys)
    _rescue.stream_dev(worker, rp, d_keys, d_ct, L, count, d_msg, decrypt=True)


# ---------------------------------------------------------------------------------------------- host arrays in, host arrays out
def dh_key(worker: PlonkWorker, params: EdwardsParams, scalars, points, rescue=None) -> np.ndarray:
    """scalars (count, 4), points (count, 2, 4) -> hash3(S.x, S.y, 0) of S = [scalar] point, (count, 4)"""
    _ed._check(worker, params)
    rp = _ed._rescue_params(params, rescue)
    s, p = _ed._scalars(scalars), _ed._points(points)
    count = _ed._same_count(s, p)
    if count == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    return _ed._run(worker, (s, p), (count, 4), np.uint64, lambda ds, dp, do: dh_key_dev(worker, params, rp, ds, dp, count, do))


def encrypt(worker: PlonkWorker, params: EdwardsParams, ek, msg, r, rescue=None):
    """ek (count, 2, 4), msg (count, L, 4), r (count, 4) -> (E (count, 2, 4), ct (count, L, 4)).  ValueError for an r >= l (compared on
    the host; the rest runs on the device)."""
    _ed._check(worker, params)
    rp = _ed._rescue_params(params, rescue)
    ek, m, r = _ed._points(ek), _texts(msg, "msg"), _ed._scalars(r)
    count = _ed._same_count(ek, m, r)
    L = m.shape[1]
    big = [i for i, x in enumerate(_ed._residues(params.field, r)) if x >= params.order]
    if big:
        raise ValueError(f"r[{big[0]}] >= l: the randomness is a residue below the subgroup order")
    if count == 0:
        return ek.copy(), m.copy()
    with DeviceScope(worker) as s:
        d_ek, d_m, d_r = (s.upload(a) for a in (ek, m, r))
        d_E, d_keys = s.alloc(count * 64), s.alloc(count * 32)
        encrypt_dev(worker, params, d_ek.ptr, d_m.ptr, d_r.ptr, L, count, d_E.ptr, d_m.ptr, d_keys.ptr, rp)
        return d_E.download((count, 2, 4)), d_m.download(m.shape)


def decrypt(worker: PlonkWorker, params: EdwardsParams, dk, ciphertext, rescue=None):
    """dk (count, 4), ciphertext = (E (count, 2, 4), ct (count, L, 4)) -> (msg (count, L, 4), ok (count,) bool).  ok[i]: E_i is on the curve and
    in the subgroup of order l; where it is False the message is still computed (an E off the curve counts as the identity) and is the
    caller's to discard."""
    _ed._check(worker, params)
    rp = _ed._rescue_params(params, rescue)
    dk, E, ct = _ed._scalars(dk), _ed._points(ciphertext[0]), _texts(ciphertext[1], "ct")
    count = _ed._same_count(dk, E, ct)
    L = ct.shape[1]
    if count == 0:
        return ct.copy(), np.zeros(0, dtype=bool)
    with DeviceScope(worker) as s:
        d_dk, d_E, d_ct = (s.upload(a) for a in (dk, E, ct))
        d_flags, d_keys = s.alloc(count * 4), s.alloc(count * 32)
        decrypt_dev(worker, params, d_dk.ptr, d_E.ptr, d_ct.ptr, L, count, d_ct.ptr, d_flags.ptr, d_keys.ptr, rp)
        flags = d_flags.download((count,), dtype=np.uint32)
        return d_ct.download(ct.shape), (flags & _ed.IN_SUBGROUP) != 0


# ---------------------------------------------------------------------------------------------- the circuit
def elgamal_circuit(curve: str, m: int, L: int, params: Optional[EdwardsParams] = None, rescue=None) -> BuiltCircuit:
    """m encryptions of L elements each in one circuit, as edwards.schnorr_circuit is for signatures.  Public inputs, m each: ek.x, ek.y, E.x,
    E.y, then ct_0 .. ct_{L-1}; private inputs, m each: r, then msg_0 .. msg_{L-1}.  CircuitBuilder.elgamal_encrypt over all m at once, its
    outputs tied to the public E and ct by enforce_equal."""
    if m < 1:
        raise ValueError(f"m = {m}: at least one ciphertext")
    if L < 1:
        raise ValueError(f"L = {L}: at least one message element")
    b = CircuitBuilder(curve)
    prm, rp = b._edwards_params(params), b._rescue_params(rescue)
    as_ids = lambda v: np.atleast_1d(np.asarray(v, dtype=np.int64))
    ekx, eky, Ex, Ey = (as_ids(b.public_input(m)) for _ in range(4))
    ct = [as_ids(b.public_input(m)) for _ in range(L)]
    r = as_ids(b.input(m))
    msg = [as_ids(b.input(m)) for _ in range(L)]
    E_out, ct_out = b.elgamal_encrypt((ekx, eky), msg, r, prm, rp)
    b.enforce_point_equal(E_out, (Ex, Ey))
    for got, want in zip(ct_out, ct):
        b.enforce_equal(got, want)
    return b.build()


def elgamal_witness_inputs(ek, r, msg, ciphertext):
    """-> (inputs ((1 + L) m, 4), public_inputs ((4 + L) m, 4)) in the order elgamal_circuit creates them: what BuiltCircuit.solve_dev /
    preprocess take"""
    ek, r, m = _ed._points(ek), _ed._scalars(r), _texts(msg, "msg")
    E, ct = _ed._points(ciphertext[0]), _texts(ciphertext[1], "ct")
    _ed._same_count(ek, r, m, E, ct)
    if m.shape[1] != ct.shape[1]:
        raise ValueError(f"mismatched lengths [{m.shape[1]}, {ct.shape[1]}]: message and ciphertext elements")
    L = m.shape[1]
    inputs = np.concatenate([r] + [m[:, i] for i in range(L)])
    public = np.concatenate([ek[:, 0], ek[:, 1], E[:, 0], E[:, 1]] + [ct[:, i] for i in range(L)])
    return inputs, public
