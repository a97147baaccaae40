"""The Rescue permutation and Merkle trees over it, computed on the device (csrc/rescue_kernels.hpp behind plonk_rescue_permute_dev and
plonk_rescue_merkle_dev), with the parameters that `builder.CircuitBuilder.rescue_permutation` proves the same function with.

State s in Fr^4, MDS matrix M (4 x 4), round keys K[0 .. 24] (4 elements each), alpha = 5 on both scalar fields — the structure of
jellyfish's jf-rescue (width 4, 12 rounds, 25 round keys):

    permute(s):  s <- s + K[0]
                 for i in 0 .. 11:   s <- M (s_j^(1/5))_j + K[2i+1]          x^(1/5) = x^d, d = 5^-1 mod (r - 1); 0 -> 0
                                     s <- M (s_j^5)_j     + K[2i+2]
    hash2(l, r) = permute((l, r, 0, 0))[0]

The DEFAULT parameters are this project's own (jellyfish's tables are not vendored): M[i][j] = 1 / (i + j + 4), a Cauchy matrix with
x_i = i, y_j = -(j + 4) and hence MDS, and K[t][i] = SHAKE-256("distributed_plonk_amd.rescue.v1|<curve>|" + bytes([t, i])), 64 bytes read
little-endian and reduced mod r.  Whoever holds other tables passes them: RescueParams(curve, mds, round_keys).

A Merkle tree over L = 2^k leaves lives in one buffer of 2L - 1 Fr in heap order: node 0 is the root, the children of node m are 2m + 1
(left) and 2m + 2 (right), leaf i is node L - 1 + i, and node[m] = hash2(node[2m+1], node[2m+2]).

Field elements cross this module as everywhere in the package: (.., 4) uint64 Montgomery limbs.
"""
from __future__ import annotations

import hashlib
from typing import Sequence

import numpy as np

from . import fr as _fr
from .worker import PlonkWorker

WIDTH, ROUNDS = 4, 12
NUM_KEYS = 2 * ROUNDS + 1
NUM_PARAMS = WIDTH * WIDTH + WIDTH * NUM_KEYS         # 116
DOMAIN = b"distributed_plonk_amd.rescue.v1|"


class RescueParams:
    """curve: "bn254" or "bls12_381"; mds: 4 rows of 4 residues; round_keys: 25 rows of 4 residues (Python ints, reduced mod r here)."""

    _defaults = {}

    def __init__(self, curve: str, mds: Sequence[Sequence[int]], round_keys: Sequence[Sequence[int]]):
        if curve not in _fr.FIELDS:
            raise ValueError(f"unknown curve {curve!r} (one of {', '.join(_fr.FIELDS)})")
        self.curve, self.field = curve, _fr.FIELDS[curve]
        p = self.field.p
        if (p - 1) % 5 == 0:
            raise ValueError(f"5 divides r - 1 on {curve}: x -> x^5 is no permutation of the field")
        self.mds = [[int(x) % p for x in row] for row in mds]
        self.round_keys = [[int(x) % p for x in row] for row in round_keys]
        if len(self.mds) != WIDTH or any(len(r) != WIDTH for r in self.mds):
            raise ValueError(f"the MDS matrix is {WIDTH} x {WIDTH}")
        if len(self.round_keys) != NUM_KEYS or any(len(r) != WIDTH for r in self.round_keys):
            raise ValueError(f"{NUM_KEYS} round keys of {WIDTH} elements each")
        self._limbs = None

    @classmethod
    def default(cls, curve: str) -> "RescueParams":
        if curve not in cls._defaults:
            p = _fr.FIELDS[curve].p
            mds = [[pow(i + j + 4, -1, p) for j in range(WIDTH)] for i in range(WIDTH)]
            keys = [[int.from_bytes(hashlib.shake_256(DOMAIN + curve.encode() + b"|" + bytes([t, i])).digest(64), "little") % p for i in range(WIDTH)]
                    for t in range(NUM_KEYS)]
            cls._defaults[curve] = cls(curve, mds, keys)
        return cls._defaults[curve]

    def residues(self) -> list:
        """the 116 parameters in the order of the C ABI: M row-major, then K[0], K[1], ..."""
        return [x for row in self.mds for x in row] + [x for row in self.round_keys for x in row]

    def limbs(self) -> np.ndarray:
        """(116, 4) uint64 Montgomery limbs: what plonk_rescue_permute_dev / plonk_rescue_merkle_dev take as `params`"""
        if self._limbs is None:
            f = self.field
            raw = b"".join((x * f.R % f.p).to_bytes(32, "little") for x in self.residues())
            self._limbs = np.frombuffer(raw, dtype=np.uint64).reshape(NUM_PARAMS, 4).copy()
            self._limbs.setflags(write=False)
        return self._limbs


def _check(worker: PlonkWorker, params: RescueParams):
    if worker.curve_name != params.curve:
        raise ValueError(f"parameters over {params.curve}, worker over {worker.curve_name}")


def permute_dev(worker: PlonkWorker, params: RescueParams, d_states: int, count: int):
    """`count` states [count][4] Fr at the device pointer, permuted in place.  Ordered on the worker's stream, not synchronised."""
    _check(worker, params)
    worker.rescue_permute_dev(params.limbs(), d_states, count)


def permute(worker: PlonkWorker, params: RescueParams, states) -> np.ndarray:
    """states: (count, 4, 4) Montgomery limbs (or anything that reshapes to it) -> the permuted states, same shape"""
    _check(worker, params)
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, WIDTH, 4)
    if s.shape[0] == 0:
        return s.copy()
    buf = worker.alloc(s.nbytes)
    try:
        buf.upload(s)
        permute_dev(worker, params, buf.ptr, s.shape[0])
        return buf.download(s.shape)
    finally:
        buf.free()


def merkle_dev(worker: PlonkWorker, params: RescueParams, d_nodes: int, log_leaves: int):
    """d_nodes: 2^(log_leaves + 1) - 1 Fr in heap order with the leaves (the last 2^log_leaves) filled; every inner node is written.  Ordered
    on the worker's stream, not synchronised."""
    _check(worker, params)
    worker.rescue_merkle_dev(params.limbs(), d_nodes, log_leaves)


class MerkleTree:
    """The tree over `leaves` ((L, 4) Montgomery limbs, L a power of two), built on the device at construction.  d_nodes: the device buffer
    of 2L - 1 Fr in heap order (close() frees it); nodes / root / path() read it back once."""

    def __init__(self, worker: PlonkWorker, params: RescueParams, leaves):
        _check(worker, params)
        lv = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        L = lv.shape[0]
        if L == 0 or L & (L - 1):
            raise ValueError(f"{L} leaves: a power of two, at least 1")
        self.worker, self.params = worker, params
        self.num_leaves, self.log_leaves = L, L.bit_length() - 1
        self._nodes = None
        self.d_nodes = worker.alloc((2 * L - 1) * 32)
        try:
            worker.write_bytes(self.d_nodes.offset((L - 1) * 32), lv)
            merkle_dev(worker, params, self.d_nodes.ptr, self.log_leaves)
        except BaseException:
            self.d_nodes.free()
            raise

    @property
    def nodes(self) -> np.ndarray:
        """(2L - 1, 4) Montgomery limbs, heap order"""
        if self._nodes is None:
            self._nodes = self.d_nodes.download((2 * self.num_leaves - 1, 4))
        return self._nodes

    @property
    def root(self) -> np.ndarray:
        return self.nodes[0]

    def path(self, i: int):
        """-> (siblings (log_leaves, 4) limbs, index_bits: log_leaves ints), from the leaf to the root.  index_bits[j] = 1: the node on the
        path is the RIGHT child at depth j and the sibling the left one — bit j of i; what builder.merkle_root takes."""
        if not 0 <= i < self.num_leaves:
            raise ValueError(f"leaf {i} of {self.num_leaves}")
        m = self.num_leaves - 1 + i
        sibs, bits = [], []
        while m:
            right = m % 2 == 0
            sibs.append(self.nodes[m - 1 if right else m + 1])
            bits.append(int(right))
            m = (m - 1) // 2
        return (np.stack(sibs) if sibs else np.zeros((0, 4), dtype=np.uint64)), bits

    def close(self):
        if self.d_nodes.ptr:
            self.d_nodes.free()
