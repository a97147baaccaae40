"""A pure-Python reference of the Rescue permutation and its Merkle tree (a helper of the Rescue tests, not a test; imports no project code).

Written from the definition with Python integers and pow.  State s in Fr^4, MDS matrix M (4 x 4), round keys K[0 .. 24] (4 elements each):

    permute(s):  s <- s + K[0]
                 for i in 0 .. 11:   s <- M (s_j^(1/5))_j + K[2i+1]          x^(1/5) = x^d, d = 5^-1 mod (r - 1); 0 -> 0
                                     s <- M (s_j^5)_j     + K[2i+2]
    hash2(l, r) = permute((l, r, 0, 0))[0]

Default parameters per curve: M[i][j] = (i + j + 4)^-1 mod r, K[t][i] = SHAKE-256(b"distributed_plonk_amd.rescue.v1|" + curve + b"|" +
bytes([t, i])), 64 bytes little-endian, mod r.  Merkle tree over L = 2^k leaves, heap order in one list of 2L - 1 residues: node 0 the
root, children of m at 2m + 1 (left) and 2m + 2 (right), leaf i at L - 1 + i, node[m] = hash2(node[2m+1], node[2m+2])."""
import hashlib
import random

MODULI = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}
CURVES = tuple(MODULI)
WIDTH, ROUNDS = 4, 12
NUM_KEYS = 2 * ROUNDS + 1


def default_params(curve: str):
    """-> (M: 4 rows of 4, K: 25 rows of 4), plain residues"""
    r = MODULI[curve]
    M = [[pow(i + j + 4, -1, r) for j in range(WIDTH)] for i in range(WIDTH)]
    K = [[int.from_bytes(hashlib.shake_256(b"distributed_plonk_amd.rescue.v1|" + curve.encode() + b"|" + bytes([t, i])).digest(64), "little") % r
          for i in range(WIDTH)] for t in range(NUM_KEYS)]
    return M, K


def flat_params(curve: str, params=None):
    """the 116 parameters in the C ABI's order: M row-major, then K[0], K[1], ..."""
    M, K = params or default_params(curve)
    return [x for row in M for x in row] + [x for row in K for x in row]


def params_sha256(curve: str, params=None) -> str:
    return hashlib.sha256(b"".join(x.to_bytes(32, "little") for x in flat_params(curve, params))).hexdigest()


def root5(x: int, r: int) -> int:
    y = pow(x, pow(5, -1, r - 1), r)
    assert pow(y, 5, r) == x
    return y


def _affine(M, t, k, r):
    return [(sum(M[i][j] * t[j] for j in range(WIDTH)) + k[i]) % r for i in range(WIDTH)]


def permute(curve: str, state, params=None):
    r = MODULI[curve]
    M, K = params or default_params(curve)
    assert len(state) == WIDTH and all(0 <= x < r for x in state)
    s = [(x + k) % r for x, k in zip(state, K[0])]
    for i in range(ROUNDS):
        s = _affine(M, [root5(x, r) for x in s], K[2 * i + 1], r)
        s = _affine(M, [pow(x, 5, r) for x in s], K[2 * i + 2], r)
    return s


def hash2(curve: str, l: int, r_: int, params=None) -> int:
    return permute(curve, [l, r_, 0, 0], params)[0]


def merkle(curve: str, leaves, params=None):
    """-> the 2L - 1 nodes in heap order"""
    L = len(leaves)
    assert L and L & (L - 1) == 0
    params = params or default_params(curve)
    nodes = [0] * (L - 1) + [int(x) for x in leaves]
    for m in range(L - 2, -1, -1):
        nodes[m] = hash2(curve, nodes[2 * m + 1], nodes[2 * m + 2], params)
    return nodes


def root_from_path(curve: str, leaf: int, siblings, index_bits, params=None) -> int:
    """index_bits[j] = 1: the node on the path is the right child at depth j (from the leaf)"""
    cur = leaf
    for sib, bit in zip(siblings, index_bits):
        assert bit in (0, 1)
        cur = hash2(curve, sib, cur, params) if bit else hash2(curve, cur, sib, params)
    return cur


def fixture_inputs(curve: str):
    """the 8 input states of tests/golden/rescue_<curve>.json: all-zero, all r - 1, (1, 0, 0, 0) and 5 seeded random; and its 8 leaves"""
    r = MODULI[curve]
    rnd = random.Random("rescue fixture " + curve)
    states = [[0] * 4, [r - 1] * 4, [1, 0, 0, 0]] + [[rnd.randrange(r) for _ in range(4)] for _ in range(5)]
    leaves = [rnd.randrange(r) for _ in range(8)]
    return states, leaves
