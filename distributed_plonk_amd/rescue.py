"""The Rescue permutation, Merkle trees, the ternary accumulator, the sponge and the counter-mode stream over it, computed on the device
(csrc/rescue_kernels.hpp, csrc/rescue_acc_kernels.hpp and csrc/elgamal_kernels.hpp behind plonk_rescue_permute_dev, plonk_rescue_merkle_dev,
plonk_rescue_acc_build_dev, plonk_rescue_acc_paths_dev, plonk_rescue_sponge_dev and plonk_rescue_stream_dev), with the parameters that
`builder.CircuitBuilder.rescue_permutation` proves the same function with.

State s in Fr^4, MDS matrix M (4 x 4), round keys K[0 .. 24] (4 elements each), alpha = 5 on both scalar fields — the structure of
jellyfish's jf-rescue (width 4, 12 rounds, 25 round keys):

    permute(s):  s <- s + K[0]
                 for i in 0 .. 11:   s <- M (s_j^(1/5))_j + K[2i+1]          x^(1/5) = x^d, d = 5^-1 mod (r - 1); 0 -> 0
                                     s <- M (s_j^5)_j     + K[2i+2]
    hash2(l, r) = permute((l, r, 0, 0))[0]
    hash3(a, b, c) = permute((a, b, c, 0))[0]

The DEFAULT parameters are this project's own (jellyfish's tables are not vendored): M[i][j] = 1 / (i + j + 4), a Cauchy matrix with
x_i = i, y_j = -(j + 4) and hence MDS, and K[t][i] = SHAKE-256("distributed_plonk_amd.rescue.v1|<curve>|" + bytes([t, i])), 64 bytes read
little-endian and reduced mod r.  Whoever holds other tables passes them: RescueParams(curve, mds, round_keys).

A Merkle tree over L = 2^k leaves lives in one buffer of 2L - 1 Fr in heap order: node 0 is the root, the children of node m are 2m + 1
(left) and 2m + 2 (right), leaf i is node L - 1 + i, and node[m] = hash2(node[2m+1], node[2m+2]).

The ACCUMULATOR Acc(height, elems[0 .. count)), 1 <= height <= 40, 1 <= count <= 3^height, is jellyfish's sparse, append-only 3-ary tree,
the one the reference's test circuit proves memberships in (height 32, 50 leaves):

    level 0    c_0 = count nodes:               node_0[i]     = hash3(0, i, elems[i])              (the uid i as a field element)
    level j+1  c_{j+1} = ceil(c_j / 3) nodes:   node_{j+1}[t] = hash3(x_0, x_1, x_2),   x_k = node_j[3t+k] if 3t+k < c_j else 0

An empty subtree is 0 — not hash3(0, 0, 0) — and no all-empty node is computed; the root is node_height[0].  One buffer holds the levels one
after another from the leaves up (offset_0 = 0, offset_{j+1} = offset_j + c_j), the root last.  The path of uid i has, per level j,
pos_j = floor(i / 3^j) mod 3 and the two OTHER members of its group of three (from 3 floor(i / 3^(j+1)) on, 0 beyond c_j) in ascending
position as sib1_j, sib2_j; builder.accumulator_root takes them with is_left_j = [pos_j = 0] and is_right_j = [pos_j = 2].  jellyfish's own
constants and its encoding of a leaf are not pinned here: the parameters are injectable, the structure is the one above.

The fourth state element is the CAPACITY and carries the domain: hash2 and hash3 use 0, the sponge starts at L, the stream uses -1.

    sponge(x_0 .. x_{L-1}; n_out)   1 <= L < 2^32, n_out in (1, 2, 3):   s = (0, 0, 0, L);   for each block b = 0 .. ceil(L / 3) - 1:
                                    s[j] += x[3b + j] for j < 3 and 3b + j < L, then s = permute(s);   the result is s[0 : n_out]
    stream                          block j >= 0 of the keystream under key k is ks_j = permute((k, j, 0, -1))[0 : 3]; element i of a text of
                                    L elements uses ks_{i div 3}[i mod 3]: encryption adds it, decryption subtracts it

The length in the capacity separates (a) from (a, 0) from (a, 0, 0, 0).  sponge((a, b, c); 1) = permute((a, b, c, 3))[0] DIFFERS from
hash3(a, b, c) = permute((a, b, c, 0))[0], by design: the two are different domains.  builder.rescue_sponge and builder.rescue_stream prove
the same two functions; elgamal.py encrypts with the stream.

Field elements cross this module as everywhere in the package: (.., 4) uint64 Montgomery limbs.
"""
from __future__ import annotations

import hashlib
from typing import Sequence

import numpy as np

from . import fr as _fr
from .worker import DeviceScope, PlonkWorker, closing_on_error

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
    with DeviceScope(worker) as scope:
        buf = scope.upload(s)
        permute_dev(worker, params, buf.ptr, s.shape[0])
        return buf.download(s.shape)


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
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            self.d_nodes = self._scope.alloc((2 * L - 1) * 32)
            worker.write_bytes(self.d_nodes.offset((L - 1) * 32), lv)
            merkle_dev(worker, params, self.d_nodes.ptr, self.log_leaves)

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
        self._scope.close()


# ---------------------------------------------------------------------------------------------- the ternary accumulator
MAX_HEIGHT = 40


def hash3(worker: PlonkWorker, params: RescueParams, triples) -> np.ndarray:
    """triples: (count, 3, 4) Montgomery limbs (a, b, c) -> (count, 4): hash3(a, b, c) = permute((a, b, c, 0))[0]"""
    t = np.ascontiguousarray(triples, dtype=np.uint64).reshape(-1, 3, 4)
    states = np.zeros((t.shape[0], WIDTH, 4), dtype=np.uint64)
    states[:, :3] = t
    return permute(worker, params, states)[:, 0].copy()


def acc_level_counts(height: int, count: int) -> list:
    """c_0 .. c_height of Acc(height, count elems)"""
    if not 1 <= height <= MAX_HEIGHT:
        raise ValueError(f"height = {height}: 1 .. {MAX_HEIGHT}")
    if not 1 <= count <= 3 ** height:
        raise ValueError(f"count = {count}: 1 .. 3^{height}")
    counts = [count]
    for _ in range(height):
        counts.append((counts[-1] + 2) // 3)
    return counts


def acc_build_dev(worker: PlonkWorker, params: RescueParams, d_elems: int, count: int, height: int, d_nodes: int):
    """d_elems: count Fr; d_nodes: sum(acc_level_counts(height, count)) Fr, every one written.  Ordered on the worker's stream, not
    synchronised."""
    _check(worker, params)
    worker.rescue_acc_build_dev(params.limbs(), d_elems, count, height, d_nodes)


def acc_paths_dev(worker: PlonkWorker, d_nodes: int, count: int, height: int, d_elems: int, d_uids: int, m: int, d_inputs_out: int):
    """d_uids: m u64; d_inputs_out: (2 + 4 height, m) Fr — uid, elem, then per level sib1, sib2, is_left, is_right: the inputs of
    membership.membership_circuit in their order.  Synchronises; a uid >= count is a PlonkError."""
    worker.rescue_acc_paths_dev(d_nodes, count, height, d_elems, d_uids, m, d_inputs_out)


class Accumulator:
    """Acc(height, elems) built on the device at construction; elems: (count, 4) Montgomery limbs.  d_elems / d_nodes: the device buffers
    (close() frees them); level_counts[j] = c_j and level_offsets[j] for j = 0 .. height; nodes / root / path() read the nodes back once."""

    def __init__(self, worker: PlonkWorker, params: RescueParams, elems, height: int):
        _check(worker, params)
        el = np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1, 4)
        self.level_counts = acc_level_counts(height, el.shape[0])
        self.level_offsets = [sum(self.level_counts[:j]) for j in range(height + 1)]
        self.worker, self.params, self.height, self.count = worker, params, height, el.shape[0]
        self.num_nodes = sum(self.level_counts)
        self._nodes = None
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            self.d_elems = self._scope.alloc(el.nbytes)
            self.d_nodes = self._scope.alloc(self.num_nodes * 32)
            self.d_elems.upload(el)
            acc_build_dev(worker, params, self.d_elems.ptr, self.count, height, self.d_nodes.ptr)

    @property
    def nodes(self) -> np.ndarray:
        """(sum c_j, 4) Montgomery limbs: level j is nodes[level_offsets[j]:][:level_counts[j]]"""
        if self._nodes is None:
            self._nodes = self.d_nodes.download((self.num_nodes, 4))
        return self._nodes

    @property
    def root(self) -> np.ndarray:
        return self.nodes[-1]

    def level(self, j: int) -> np.ndarray:
        return self.nodes[self.level_offsets[j]:self.level_offsets[j] + self.level_counts[j]]

    def path(self, i: int):
        """-> (sib1 (height, 4), sib2 (height, 4) limbs, positions: height ints in (0, 1, 2)), from the leaves up"""
        if not 0 <= i < self.count:
            raise ValueError(f"uid {i} of {self.count}")
        sib1, sib2 = np.zeros((self.height, 4), dtype=np.uint64), np.zeros((self.height, 4), dtype=np.uint64)
        positions = []
        for j in range(self.height):
            lvl, q = self.level(j), i // 3 ** j
            pos, g = q % 3, q - q % 3
            for dst, k in zip((sib1, sib2), [k for k in range(3) if k != pos]):
                if g + k < lvl.shape[0]:
                    dst[j] = lvl[g + k]
            positions.append(pos)
        return sib1, sib2, positions

    def witness_inputs_dev(self, uids):
        """-> a device buffer (the caller frees it) of (2 + 4 height, len(uids)) Fr: what BuiltCircuit.solve_dev / preprocess take as d_inputs for
        membership.membership_circuit(curve, height, len(uids)).  Gathered on the device from d_nodes and d_elems; only the uids go up."""
        u = np.ascontiguousarray(uids, dtype=np.uint64).reshape(-1)
        m = u.shape[0]
        with DeviceScope(self.worker) as s:
            out = s.alloc(max(1, (2 + 4 * self.height) * m) * 32)
            d_uids = s.alloc(max(1, m) * 8)
            if m:
                d_uids.upload(u)
            acc_paths_dev(self.worker, self.d_nodes.ptr, self.count, self.height, self.d_elems.ptr, d_uids.ptr, m, out.ptr)
            return s.release(out)

    def close(self):
        self._scope.close()


# ---------------------------------------------------------------------------------------------- the sponge and the counter-mode stream
MAX_SPONGE_LEN = (1 << 32) - 1


def _text_shape(L: int, what: str):
    if not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= MAX_SPONGE_LEN:
        raise ValueError(f"{what}: L = {L!r} (1 .. 2^32 - 1)")


def sponge_dev(worker: PlonkWorker, params: RescueParams, d_inputs: int, L: int, count: int, n_out: int, d_out: int):
    """d_out[i][0 : n_out] = sponge(d_inputs[i][0 : L]; n_out): inputs (count, L) Fr row-major, outputs (count, n_out).  One launch, ordered
    on the worker's stream, not synchronised.  sponge((a, b, c); 1) is NOT hash3(a, b, c): the capacity starts at L = 3, hash3's at 0."""
    _check(worker, params)
    _text_shape(L, "sponge")
    if n_out not in (1, 2, 3):
        raise ValueError(f"sponge: n_out = {n_out!r} (1, 2 or 3)")
    worker.rescue_sponge_dev(params.limbs(), d_inputs, int(L), count, n_out, d_out)


def sponge(worker: PlonkWorker, params: RescueParams, inputs, n_out: int = 1) -> np.ndarray:
    """inputs: (count, L, 4) Montgomery limbs, L >= 1 -> (count, n_out, 4): the sponge of each row (see the module docstring; it differs from
    hash3 on three elements by design)"""
    _check(worker, params)
    x = np.ascontiguousarray(inputs, dtype=np.uint64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError(f"sponge: inputs of shape {x.shape}, expected (count, L, 4)")
    count, L = x.shape[0], x.shape[1]
    _text_shape(L, "sponge")
    if n_out not in (1, 2, 3):
        raise ValueError(f"sponge: n_out = {n_out!r} (1, 2 or 3)")
    if count == 0:
        return np.zeros((0, n_out, 4), dtype=np.uint64)
    with DeviceScope(worker) as s:
        d_in, d_out = s.alloc(x.nbytes), s.alloc(count * n_out * 32)
        d_in.upload(x)
        sponge_dev(worker, params, d_in.ptr, L, count, n_out, d_out.ptr)
        return d_out.download((count, n_out, 4))


def stream_dev(worker: PlonkWorker, params: RescueParams, d_keys: int, d_in: int, L: int, count: int, d_out: int, decrypt: bool = False):
    """d_out[i][t] = d_in[i][t] + ks (or - ks with decrypt) for the keystream under d_keys[i]: keys (count,) Fr, texts (count, L) Fr row-major.
    One launch of count x ceil(L / 3) lanes, ordered on the worker's stream, not synchronised; d_out may be d_in."""
    _check(worker, params)
    _text_shape(L, "stream")
    worker.rescue_stream_dev(params.limbs(), d_keys, d_in, int(L), count, bool(decrypt), d_out)


def stream(worker: PlonkWorker, params: RescueParams, keys, texts, decrypt: bool = False) -> np.ndarray:
    """keys (count, 4), texts (count, L, 4) Montgomery limbs -> texts + keystream (decrypt: - keystream), same shape"""
    _check(worker, params)
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 4)
    x = np.ascontiguousarray(texts, dtype=np.uint64)
    if x.ndim != 3 or x.shape[2] != 4:
        raise ValueError(f"stream: texts of shape {x.shape}, expected (count, L, 4)")
    if k.shape[0] != x.shape[0]:
        raise ValueError(f"mismatched lengths [{k.shape[0]}, {x.shape[0]}]: one key per text")
    count, L = x.shape[0], x.shape[1]
    _text_shape(L, "stream")
    if count == 0:
        return x.copy()
    with DeviceScope(worker) as s:
        d_k, d_x = s.alloc(k.nbytes), s.alloc(x.nbytes)
        d_k.upload(k)
        d_x.upload(x)
        stream_dev(worker, params, d_k.ptr, d_x.ptr, L, count, d_x.ptr, decrypt)
        return d_x.download(x.shape)
