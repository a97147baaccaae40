"""KZG polynomial commitments as a scheme of their own: commit, open at many points on the device, verify and batch-verify openings.

An opening (C, pi, z, y) of the commitment C = [f(tau)]_1 claims f(z) = y with the proof pi = [(f(tau) - y) / (tau - z)]_1, the commitment
of the quotient (f - y) / (X - z).  It holds iff

    e(pi, [tau]_2) = e(C - y G + z pi, [1]_2).

`open_many` makes the values and the quotient rows of all points of a chunk in one `plonk_poly_open_many_dev` call — the points stay on the
device, nothing per point happens on the host — and commits the rows with one `plonk_commit_many_dev`.  `batch_verify` turns every opening
into its pair A = rho pi, B = rho C + (rho z) pi - (rho y) G (`plonk_kzg_pairs_dev`) and goes through the fold of the PLONK batch verifier
(`verifier._fold`): the sum tree on the device, one pairing check e(sum A, beta_h) e(-sum B, h) == 1, and the bisection over tree nodes
when it fails.  Only status words and tree nodes are read back.

Scalars are Montgomery limbs (4 u64) as everywhere in the library, points affine x || y with all zeros for infinity.  Every function is
call-scoped: the device buffers it makes are freed when it returns or raises (`DeviceScope`).

Not here: one proof for a set of points (it needs more powers of tau in G2 than `OpenKey` holds), FK20-style openings at all roots of
unity, and openings as bytes.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _ffi
from . import fr as _fr
from . import verifier as _vf
from .worker import DeviceBuffer, DeviceScope

STATUS_BITS = {1: "point off the curve", 2: "point outside the r-subgroup", 8: "non-canonical encoding"}
MAX_POINTS_PER_CALL = 4096                                # plonk_commit_many_dev takes at most 4096 polynomials (plonk_poly_open_many_dev: 2^16 points)


class Opening(NamedTuple):
    point: np.ndarray                                     # z, (4,) Montgomery limbs
    value: np.ndarray                                     # y = f(z), (4,) Montgomery limbs
    proof_xy: np.ndarray                                  # pi, (2Q,) x || y, all zeros for infinity


def tile() -> int:
    """Coefficients per tile of the kernels of `plonk_poly_open_many_dev`."""
    return int(_ffi.lib().plonk_poly_open_many_tile())


def top_lanes() -> int:
    """Lanes of the per-point top scan of `plonk_poly_open_many_dev`: above top_lanes() * tile() quotient coefficients a lane scans two tiles."""
    return int(_ffi.lib().plonk_poly_open_many_top_lanes())


def _points(curve: str, points) -> np.ndarray:
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
    f = _fr.FIELDS[curve]
    for j, z in enumerate(pts):
        if f.p <= sum(int(v) << (64 * i) for i, v in enumerate(z)):
            raise ValueError(f"point {j} is not a canonical residue")
    return pts


def _poly(bufs: DeviceScope, coeffs_or_dev):
    """(device pointer, length) of the polynomial: a `(DeviceBuffer | ptr, len)` pair as it is, host limbs uploaded into a buffer of bufs."""
    if isinstance(coeffs_or_dev, tuple) and len(coeffs_or_dev) == 2 and isinstance(coeffs_or_dev[0], (DeviceBuffer, int)):
        d, n = coeffs_or_dev
        return (d.ptr if isinstance(d, DeviceBuffer) else int(d)), int(n)
    c = np.ascontiguousarray(coeffs_or_dev, dtype=np.uint64).reshape(-1, 4)
    return (bufs.upload(c).ptr if c.shape[0] else 0), c.shape[0]


def _affine(worker, jac: np.ndarray) -> np.ndarray:
    xy, inf = worker.g1_to_affine(jac)
    return np.zeros(2 * worker.q64, np.uint64) if inf else np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1)


def commit(worker, coeffs):
    """The commitment of (len, 4) coefficient limbs against the resident key: (xy, is_infinity) as `Prover` returns points."""
    with worker.scope() as s:
        d, n = _poly(s, coeffs)
        if n > worker.n_bases:
            raise ValueError(f"{n} coefficients for a commit key of {worker.n_bases} points")
        return worker.g1_to_affine(worker.commit_dev(d, n))


def evaluate(worker, coeffs_or_dev, points) -> np.ndarray:
    """f at every point, (M, 4): `plonk_poly_open_many_dev` without quotient rows."""
    pts = _points(worker.curve_name, points)
    M = pts.shape[0]
    if M == 0:
        return np.zeros((0, 4), np.uint64)
    out = []
    with worker.scope() as s:
        d, n = _poly(s, coeffs_or_dev)
        for lo in range(0, M, 1 << 16):
            m = min(1 << 16, M - lo)
            d_pts, d_val, d_st = s.upload(pts[lo:lo + m]), s.alloc(m * 32), s.alloc(m * 4)
            worker.poly_open_many_dev(d, n, d_pts.ptr, m, d_val.ptr, 0, 0, d_st.ptr)
            out.append(d_val.download((m, 4)))
            for b in (d_pts, d_val, d_st):
                s.free(b)
    return np.concatenate(out)


def open_many(worker, coeffs_or_dev, points, max_scratch_bytes: int = 1 << 30) -> list:
    """Openings of one polynomial at M points, in point order.  The points go in chunks whose quotient rows (len - 1 coefficients each) fit
    max_scratch_bytes, at least one point and at most 4096 per chunk: one `plonk_poly_open_many_dev` and one `plonk_commit_many_dev` each.
    len - 1 must not exceed the resident commit key, and every point has to be a canonical residue: ValueError before any launch."""
    pts = _points(worker.curve_name, points)
    M = pts.shape[0]
    with worker.scope() as s:
        d, n = _poly(s, coeffs_or_dev)
        row = max(n - 1, 0)
        if row > worker.n_bases:
            raise ValueError(f"a quotient of {row} coefficients for a commit key of {worker.n_bases} points")
        if M == 0:
            return []
        chunk = max(1, min(M, MAX_POINTS_PER_CALL, max_scratch_bytes // (32 * row) if row else M))
        d_pts, d_val, d_st = s.upload(pts), s.alloc(chunk * 32), s.alloc(chunk * 4)
        d_q = s.alloc(chunk * row * 32) if row else None
        inf = np.zeros(2 * worker.q64, np.uint64)
        out = []
        for lo in range(0, M, chunk):
            m = min(chunk, M - lo)
            worker.poly_open_many_dev(d, n, d_pts.ptr + lo * 32, m, d_val.ptr, d_q.ptr if row else 0, row, d_st.ptr)
            proofs = [_affine(worker, j) for j in worker.commit_many_dev([(d_q.ptr + i * row * 32, row) for i in range(m)])] if row else [inf] * m
            if d_st.download((m,), dtype=np.uint32).any():
                raise ValueError("a point is not a canonical residue")          # checked on the host above: not reached
            vals = d_val.download((m, 4))
            out += [Opening(pts[lo + i].copy(), vals[i], proofs[i]) for i in range(m)]
        return out


def opening_record(curve: str, comm, op: Opening) -> np.ndarray:
    """One `plonk_kzg_pairs_dev` record: C, pi, z, y.  comm: (xy, is_infinity) or x || y limbs."""
    c = _vf._point_xy(curve, comm) if isinstance(comm, tuple) else np.ascontiguousarray(comm, dtype=np.uint64).reshape(-1)
    parts = [c, np.ascontiguousarray(op.proof_xy, dtype=np.uint64).reshape(-1)]
    if any(p.shape != (2 * _vf._q64(curve),) for p in parts):
        raise ValueError(f"a point of the opening is not on {curve}")
    return np.concatenate(parts + [np.ascontiguousarray(op.point, dtype=np.uint64).reshape(4), np.ascontiguousarray(op.value, dtype=np.uint64).reshape(4)])


def batch_verify(worker, open_key: "_vf.OpenKey", comms: Sequence, openings: Sequence[Opening], seed: Optional[int] = None, stats: Optional[dict] = None,
                 _rho: Optional[np.ndarray] = None) -> list:
    """One verdict per opening, comms[i] the commitment that openings[i] opens.  `stats` receives "pairing_checks", "status" (the status word
    of every opening, STATUS_BITS) and "kernel_ms" as verifier.batch_verify's does.  An opening with a status is rejected and leaves the
    others alone."""
    curve = _vf._curve(worker, open_key)
    K = len(openings)
    if len(comms) != K:
        raise ValueError("one commitment per opening")
    rho = _vf._rhos(curve, K, seed) if _rho is None else _rho
    if rho.shape[0] != K:
        raise ValueError("one rho per opening")
    recs = [opening_record(curve, c, o) for c, o in zip(comms, openings)]
    with worker.scope() as bufs:
        d_recs = _vf._upload(bufs, np.stack(recs)) if K else 0
        launch = lambda d_rho, d_out, d_status, _d_debug: worker.kzg_pairs_dev(K, d_recs, d_rho, open_key.g, d_out, d_status)
        return _vf._fold(bufs, open_key, K, rho, launch, None, stats)


def verify(worker, open_key: "_vf.OpenKey", comm, opening: Opening, stats: Optional[dict] = None) -> bool:
    """One opening, the single pairing check (rho = 1)."""
    one = _fr.FIELDS[worker.curve_name].to_limbs(1)[None, :]
    return batch_verify(worker, open_key, [comm], [opening], stats=stats, _rho=one)[0]
