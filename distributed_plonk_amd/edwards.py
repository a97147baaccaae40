"""The embedded twisted Edwards curve over Fr, computed on the device (csrc/edwards_kernels.hpp behind plonk_edwards_mul_dev,
plonk_edwards_fixed_mul_dev, plonk_edwards_add_dev and plonk_edwards_check_dev), with the parameters that builder.CircuitBuilder's point
gadgets prove the same group with — as rescue.py is to rescue_permutation — and Schnorr signatures over it.

    E:  a x^2 + y^2 = 1 + d x^2 y^2  over the worker's Fr,        (x1, y1) + (x2, y2) = ( (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2),
                                                                                          (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2) )

With a a square and d a non-square (EdwardsParams refuses anything else) no denominator vanishes for points of E: the law is COMPLETE —
P + P, P + (-P), the identity (0, 1) and the points of order 2, 4 and 8 go through the same formula, in the kernels and in the gadgets.
The defaults are Baby Jubjub over BN254's Fr (a = 168700, d = 168696, circomlib's generator of the subgroup of prime order l) and Jubjub
over BLS12-381's (a = -1, d = -10240/10241, G = 8 x the point with y = 3 and the smaller x); both have cofactor 8.

A point crosses this module affine: (.., 2, 4) uint64, x then y, Montgomery limbs.  A SCALAR is a field element, (.., 4) Montgomery limbs,
and stands for its canonical residue in [0, r) — what a circuit variable holds, so a Rescue output multiplies a point as it is.

Schnorr, with hash3 of rescue.py:   pk = [sk] G;   sign: R = [nonce] G, c = hash3(hash3(R.x, R.y, pk.x), pk.y, m), s = nonce + c sk mod l;
verify: s < l, R and pk on E, [s] G = R + [c] pk.  The signature is (R, s).  What the circuit of `schnorr_circuit` does and does not prove
stands in builder.CircuitBuilder.schnorr_verify.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import fr as _fr
from . import rescue as _rescue
from .builder import BuiltCircuit, CircuitBuilder
from .worker import DeviceScope, PlonkWorker

NUM_PARAM_WORDS = 20                                  # a, d, G.x, G.y (4 limbs each, Montgomery), l (4 plain limbs)
ON_CURVE, IN_SUBGROUP = 1, 2                          # bits of plonk_edwards_check_dev's flags


class EdwardsParams:
    """curve: "bn254" or "bls12_381"; a, d: the curve's coefficients; generator: (x, y) of order `order` (a prime l < r); cofactor: #E / l.
    Python ints, a, d and the coordinates reduced mod r here.  ValueError unless a is a non-zero square, d a non-square and G on the curve."""

    _defaults = {}

    def __init__(self, curve: str, a: int, d: int, generator: Sequence[int], order: int, cofactor: int):
        if curve not in _fr.FIELDS:
            raise ValueError(f"unknown curve {curve!r} (one of {', '.join(_fr.FIELDS)})")
        self.curve, self.field = curve, _fr.FIELDS[curve]
        p = self.field.p
        self.a, self.d = int(a) % p, int(d) % p
        if len(generator) != 2:
            raise ValueError("generator: a pair (x, y)")
        self.generator = (int(generator[0]) % p, int(generator[1]) % p)
        self.order, self.cofactor = int(order), int(cofactor)
        if self.a == 0 or pow(self.a, (p - 1) // 2, p) != 1:
            raise ValueError("a is not a non-zero square: the addition law would not be complete")
        if pow(self.d, (p - 1) // 2, p) != p - 1:
            raise ValueError("d is not a non-square: the addition law would not be complete")
        if not 1 < self.order < p:
            raise ValueError("order: the scalar kernels take 1 < l < r")
        x, y = self.generator
        if (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % p:
            raise ValueError("the generator is not on the curve")
        self._limbs = None

    @classmethod
    def default(cls, curve: str) -> "EdwardsParams":
        if curve not in cls._defaults:
            if curve == "bn254":
                prm = cls(curve, 168700, 168696,
                          (5299619240641551281634865583518297030282874472190772894086521144482721001553,
                           16950150798460657717958625567821834550301663161624707787222815936182638968203),
                          2736030358979909402780800718157159386076813972158567259200215660948447373041, 8)
            elif curve == "bls12_381":
                p = _fr.FIELDS[curve].p
                prm = cls(curve, -1, -10240 * pow(10241, -1, p),
                          (26425721312295396735536009845259662215154440146657062145727563247428679108070,
                           33870355149453697655464584064870436861767017640968433840972803788419917420560),
                          0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7, 8)
            else:
                raise ValueError(f"unknown curve {curve!r} (one of {', '.join(_fr.FIELDS)})")
            cls._defaults[curve] = prm
        return cls._defaults[curve]

    def add_int(self, P, Q):
        """P + Q on Python integers (the constants of builder.fixed_base_mul come from here; bulk work belongs to the device)"""
        p = self.field.p
        (x1, y1), (x2, y2) = P, Q
        t = self.d * x1 * x2 * y1 * y2 % p
        return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, p) % p, (y1 * y2 - self.a * x1 * x2) * pow(1 - t, -1, p) % p)

    def mul_int(self, k: int, P):
        """[k] P on Python integers, k >= 0"""
        acc, base = (0, 1), P
        while k:
            if k & 1:
                acc = self.add_int(acc, base)
            base = self.add_int(base, base)
            k >>= 1
        return acc

    def limbs(self) -> np.ndarray:
        """(20,) uint64: a, d, G.x, G.y as Montgomery limbs, then l plain — what the plonk_edwards_* entry points take as `params`"""
        if self._limbs is None:
            f = self.field
            raw = b"".join((x * f.R % f.p).to_bytes(32, "little") for x in (self.a, self.d) + self.generator) + self.order.to_bytes(32, "little")
            self._limbs = np.frombuffer(raw, dtype=np.uint64).copy()
            self._limbs.setflags(write=False)
        return self._limbs


def _check(worker: PlonkWorker, params: EdwardsParams):
    if not isinstance(params, EdwardsParams):
        raise ValueError("params: an edwards.EdwardsParams")
    if worker.curve_name != params.curve:
        raise ValueError(f"parameters over {params.curve}, worker over {worker.curve_name}")


def _points(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 2, 4)


def _scalars(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def _residues(field, limbs) -> list:
    """(count, 4) Montgomery limbs -> Python ints"""
    raw, R_inv, p = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes(), field.R_inv, field.p
    return [int.from_bytes(raw[i:i + 32], "little") * R_inv % p for i in range(0, len(raw), 32)]


def _same_count(*arrays):
    counts = sorted({a.shape[0] for a in arrays})
    if len(counts) != 1:
        raise ValueError(f"mismatched lengths {counts}")
    return counts[0]


# ---------------------------------------------------------------------------------------------- device pointers in, device pointers out
def mul_dev(worker: PlonkWorker, params: EdwardsParams, d_scalars: int, d_points: int, count: int, d_out: int):
    """d_out[i] = [scalars[i]] points[i].  Ordered on the worker's stream, not synchronised; d_out may be d_points."""
    _check(worker, params)
    worker.edwards_mul_dev(params.limbs(), d_scalars, d_points, count, d_out)


def fixed_mul_dev(worker: PlonkWorker, params: EdwardsParams, d_scalars: int, count: int, d_out: int):
    """d_out[i] = [scalars[i]] G from the context's window table (rebuilt when `params` changes).  Not synchronised."""
    _check(worker, params)
    worker.edwards_fixed_mul_dev(params.limbs(), d_scalars, count, d_out)


def add_dev(worker: PlonkWorker, params: EdwardsParams, d_p: int, d_q: int, count: int, d_out: int):
    """d_out[i] = p[i] + q[i].  Not synchronised; d_out may be d_p or d_q."""
    _check(worker, params)
    worker.edwards_add_dev(params.limbs(), d_p, d_q, count, d_out)


def check_dev(worker: PlonkWorker, params: EdwardsParams, d_points: int, count: int, d_flags: int):
    """d_flags[i] (u32) = ON_CURVE | IN_SUBGROUP as they hold for points[i].  Not synchronised."""
    _check(worker, params)
    worker.edwards_check_dev(params.limbs(), d_points, count, d_flags)


# ---------------------------------------------------------------------------------------------- host arrays in, host arrays out
def _run(worker: PlonkWorker, arrays, out_shape, out_dtype, call):
    """upload `arrays`, call(pointers..., d_out), download d_out"""
    with DeviceScope(worker) as s:
        ptrs = [s.upload(a).ptr for a in arrays]
        out = s.alloc(int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize)
        call(*ptrs, out.ptr)
        return out.download(out_shape, dtype=out_dtype)


def mul(worker: PlonkWorker, params: EdwardsParams, scalars, points) -> np.ndarray:
    """scalars (count, 4), points (count, 2, 4) on the curve -> [scalar] point, (count, 2, 4)"""
    _check(worker, params)
    s, p = _scalars(scalars), _points(points)
    count = _same_count(s, p)
    if count == 0:
        return p.copy()
    return _run(worker, (s, p), p.shape, np.uint64, lambda ds, dp, do: mul_dev(worker, params, ds, dp, count, do))


def fixed_mul(worker: PlonkWorker, params: EdwardsParams, scalars) -> np.ndarray:
    """scalars (count, 4) -> [scalar] G, (count, 2, 4)"""
    _check(worker, params)
    s = _scalars(scalars)
    count = s.shape[0]
    if count == 0:
        return np.zeros((0, 2, 4), dtype=np.uint64)
    return _run(worker, (s,), (count, 2, 4), np.uint64, lambda ds, do: fixed_mul_dev(worker, params, ds, count, do))


def add(worker: PlonkWorker, params: EdwardsParams, p, q) -> np.ndarray:
    """p, q (count, 2, 4) on the curve -> p + q"""
    _check(worker, params)
    p, q = _points(p), _points(q)
    count = _same_count(p, q)
    if count == 0:
        return p.copy()
    return _run(worker, (p, q), p.shape, np.uint64, lambda dp, dq, do: add_dev(worker, params, dp, dq, count, do))


def check(worker: PlonkWorker, params: EdwardsParams, points) -> np.ndarray:
    """points (count, 2, 4), any field elements -> (count,) u32 of ON_CURVE | IN_SUBGROUP"""
    _check(worker, params)
    p = _points(points)
    count = p.shape[0]
    if count == 0:
        return np.zeros(0, dtype=np.uint32)
    return _run(worker, (p,), (count,), np.uint32, lambda dp, do: check_dev(worker, params, dp, count, do))


def on_curve(worker: PlonkWorker, params: EdwardsParams, points) -> np.ndarray:
    """-> (count,) bool: the point satisfies the curve equation"""
    return (check(worker, params, points) & ON_CURVE) != 0


def in_subgroup(worker: PlonkWorker, params: EdwardsParams, points) -> np.ndarray:
    """-> (count,) bool: the point is on the curve and [l] point = (0, 1)"""
    return (check(worker, params, points) & IN_SUBGROUP) != 0


# ---------------------------------------------------------------------------------------------- Schnorr
def keygen(worker: PlonkWorker, params: EdwardsParams, secret_scalars) -> np.ndarray:
    """pk = [sk] G -> (count, 2, 4)"""
    return fixed_mul(worker, params, secret_scalars)


def _rescue_params(params: EdwardsParams, rescue):
    if rescue is None:
        return _rescue.RescueParams.default(params.curve)
    if not isinstance(rescue, _rescue.RescueParams) or rescue.curve != params.curve:
        raise ValueError(f"rescue: a rescue.RescueParams over {params.curve}")
    return rescue


def challenge(worker: PlonkWorker, params: EdwardsParams, R, pks, messages, rescue=None) -> np.ndarray:
    """c = hash3(hash3(R.x, R.y, pk.x), pk.y, m) with the device's Rescue kernel -> (count, 4)"""
    _check(worker, params)
    rp = _rescue_params(params, rescue)
    R, pk, m = _points(R), _points(pks), _scalars(messages)
    _same_count(R, pk, m)
    h = _rescue.hash3(worker, rp, np.stack([R[:, 0], R[:, 1], pk[:, 0]], axis=1))
    return _rescue.hash3(worker, rp, np.stack([h, pk[:, 1], m], axis=1))


def schnorr_sign(worker: PlonkWorker, params: EdwardsParams, sk, nonce, message, rescue=None):
    """sk, nonce, message: (count, 4) each -> (R (count, 2, 4), s (count, 4)).  R = [nonce] G and the challenge on the device; s = nonce + c sk
    mod l in Python integers on the host (signing is not the hot path).  The nonce is the caller's: fresh and secret per signature."""
    _check(worker, params)
    sk, nonce, message = _scalars(sk), _scalars(nonce), _scalars(message)
    _same_count(sk, nonce, message)
    f = params.field
    both = fixed_mul(worker, params, np.concatenate([nonce, sk]))
    R, pk = both[:nonce.shape[0]], both[nonce.shape[0]:]
    c = challenge(worker, params, R, pk, message, rescue)
    s = [(k + ci * x) % params.order for k, ci, x in zip(_residues(f, nonce), _residues(f, c), _residues(f, sk))]
    raw = b"".join((x * f.R % f.p).to_bytes(32, "little") for x in s)
    return R, np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def schnorr_verify(worker: PlonkWorker, params: EdwardsParams, pks, messages, sigs, rescue=None) -> np.ndarray:
    """pks (count, 2, 4), messages (count, 4), sigs = (R (count, 2, 4), s (count, 4)) -> (count,) bool: s < l, R and pk on the curve, and
    [s] G = R + [c] pk.  The curve check, both multiplications and the addition run on the device, over the whole batch; the two sides are
    compared limb for limb.  An off-curve R or pk is replaced by the identity before it is multiplied, and gives False."""
    _check(worker, params)
    pk, m = _points(pks), _scalars(messages)
    R, s = _points(sigs[0]), _scalars(sigs[1])
    count = _same_count(pk, m, R, s)
    if count == 0:
        return np.zeros(0, dtype=bool)
    f = params.field
    ok = np.array([x < params.order for x in _residues(f, s)], dtype=bool)
    good = on_curve(worker, params, np.concatenate([pk, R]))
    good = good[:count] & good[count:]
    ok &= good
    identity = np.stack([np.zeros(4, dtype=np.uint64), f.to_limbs(1)])
    pk, R = pk.copy(), R.copy()
    pk[~good], R[~good] = identity, identity
    c = challenge(worker, params, R, pk, m, rescue)
    with DeviceScope(worker) as scope:
        d_s, d_c, d_pk, d_R = (scope.upload(a) for a in (s, c, pk, R))
        d_lhs = scope.alloc(R.nbytes)
        fixed_mul_dev(worker, params, d_s.ptr, count, d_lhs.ptr)
        mul_dev(worker, params, d_c.ptr, d_pk.ptr, count, d_pk.ptr)
        add_dev(worker, params, d_R.ptr, d_pk.ptr, count, d_R.ptr)
        lhs, rhs = d_lhs.download(R.shape), d_R.download(R.shape)
    return ok & (lhs == rhs).all(axis=(1, 2))


def schnorr_circuit(curve: str, m: int, params: Optional[EdwardsParams] = None, rescue=None) -> BuiltCircuit:
    """m signature verifications in one circuit, as membership.membership_circuit is for memberships: public inputs pk.x, pk.y, message (m
    each, in that order), private inputs R.x, R.y, s (m each); CircuitBuilder.schnorr_verify over all m at once."""
    if m < 1:
        raise ValueError(f"m = {m}: at least one signature")
    b = CircuitBuilder(curve)
    as_ids = lambda v: np.atleast_1d(np.asarray(v, dtype=np.int64))
    pkx, pky, msg = (as_ids(b.public_input(m)) for _ in range(3))
    rx, ry, s = (as_ids(b.input(m)) for _ in range(3))
    b.schnorr_verify((pkx, pky), msg, (rx, ry), s, params, rescue)
    return b.build()


def schnorr_witness_inputs(pks, messages, sigs):
    """-> (inputs (3 m, 4), public_inputs (3 m, 4)) in the order schnorr_circuit creates them: what BuiltCircuit.solve_dev / preprocess take"""
    pk, msg = _points(pks), _scalars(messages)
    R, s = _points(sigs[0]), _scalars(sigs[1])
    _same_count(pk, msg, R, s)
    return np.concatenate([R[:, 0], R[:, 1], s]), np.concatenate([pk[:, 0], pk[:, 1], msg])
