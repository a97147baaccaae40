"""Reference restatements, wirings, random circuits and proved instances shared by the circuit / solver / verifier tests and by
tools/fuzz_abi.py (a helper of those, not a test): the stable-argsort copy permutation and the id_perm table, the `wiring` kinds, the
random layered circuits of the solver tests (fixed shape per log_n) and `layered_circuit`, the same mix of operations with the number
of rounds and the width chosen by the caller, and synthetic instances proved under the trapdoor key."""
import copy
import random

import numpy as np

from distributed_plonk_amd import builder as BD
from distributed_plonk_amd import fr as _fr

TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3


# ---------------------------------------------------------------------------------------------- the copy permutation
def ref_perm_idx(wire_vars: np.ndarray) -> np.ndarray:
    """jellyfish compute_wire_permutation: the positions of one variable in increasing order form a cycle, the last links to the first."""
    flat = np.asarray(wire_vars, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    sv = flat[order]
    nxt = np.roll(order, -1)
    starts = np.flatnonzero(np.r_[True, sv[1:] != sv[:-1]])
    ends = np.r_[starts[1:], len(sv)] - 1
    nxt[ends] = order[starts]
    out = np.empty(flat.size, dtype=np.uint64)
    out[order] = nxt.astype(np.uint64)
    return out


def ref_id_perm(oracle, cid: int, n: int, k: np.ndarray) -> np.ndarray:
    """k_i * w^j by vector doubling of the powers of w (oracle field ops)."""
    from oracle import bigint_ref as B
    from oracle import prover_ref as P
    f = P.CURVE_OBJ[cid].fr
    g = B.Radix2Domain(f, n).group_gen
    pw = np.zeros((n, 4), dtype=np.uint64)
    pw[0] = P.fr_to_limbs(f, 1)
    filled = 1
    while filled < n:
        cnt = min(filled, n - filled)
        step = np.broadcast_to(P.fr_to_limbs(f, pow(g, filled, f.p)), (cnt, 4)).copy()
        pw[filled:filled + cnt] = oracle.field_op(cid, 0, "mul", pw[:cnt], step)
        filled += cnt
    return np.concatenate([oracle.field_op(cid, 0, "mul", pw, np.broadcast_to(k[i], (n, 4)).copy()) for i in range(5)])


def wiring(kind: str, n: int, seed: int):
    rs = np.random.RandomState(seed)
    if kind == "identity":
        return np.arange(5 * n, dtype=np.uint32).reshape(5, n), 5 * n
    if kind == "single":
        return np.zeros((5, n), dtype=np.uint32), 1
    if kind == "random":
        nv = max(2, 2 * n)
        return rs.randint(0, nv, size=(5, n)).astype(np.uint32), nv
    if kind == "heavy":                      # half the positions on variable 0, like padding
        nv = max(2, n)
        wv = rs.randint(1, nv, size=5 * n).astype(np.uint32)
        wv[rs.permutation(5 * n)[:5 * n // 2]] = 0
        return wv.reshape(5, n), nv
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------- random layered circuits
def random_layered(curve: str, log_n: int, seed: int):
    """-> (BuiltCircuit of exactly 2^log_n gates after padding, input residues, public-input residues).  Rounds of `width` gates, every
    operation of the builder in turn, operands drawn from everything defined so far; gate() with 12 random selectors and q_o random,
    1 or -1; constraint gates (not solved for, some unsatisfied) in between."""
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed)
    p = _fr.FIELDS[curve].p
    n = 1 << log_n
    rounds, width, tail = (5, 1, False) if log_n == 3 else (14, ((n - 7) // 14), True)
    b = BD.CircuitBuilder(curve)
    pub = b.public_input()
    ins = b.input(3 * width)
    pool = np.concatenate([[b.zero, b.one, pub], ins])
    pick = lambda: pool[rs.randint(0, len(pool), size=width)]
    coef = lambda: [rnd.randrange(p) for _ in range(width)]
    kinds = ["add", "sub", "mul", "lc", "mul_add", "pow5_lc", "gate"]
    for r in range(rounds):
        kind = kinds[r % len(kinds)]
        if kind == "add":
            new = b.add(pick(), pick())
        elif kind == "sub":
            new = b.sub(pick(), pick())
        elif kind == "mul":
            new = b.mul(pick(), pick())
        elif kind == "lc":
            new = b.lc([pick(), pick(), pick(), pick()], [coef(), rnd.randrange(p), coef(), -1], const=coef())
        elif kind == "mul_add":
            new = b.mul_add(pick(), pick(), pick(), pick(), q0=coef(), q1=rnd.randrange(p))
        elif kind == "pow5_lc":
            new = b.pow5_lc([pick(), pick(), pick()], [coef(), 1, coef()], const=rnd.randrange(p))
        else:
            q_o = [(1, p - 1, rnd.randrange(1, p))[min(rnd.randrange(4), 2)] for _ in range(width)]
            sel = {name: coef() for name in BD.SELECTOR_INDEX if name not in ("q_o",)}
            new = b.gate([pick(), pick(), pick(), pick()], {**sel, "q_o": q_o})
        pool = np.concatenate([pool, np.atleast_1d(new)])
    if tail:
        x, y = int(pool[-1]), int(pool[-2])
        b.enforce_equal(x, x)
        b.enforce_mul(x, y, int(pool[-3]))                  # not satisfied: the solver does not look at constraints
        b.enforce_bool(b.one)
        b.enforce_constant(b.one, 1)
    built = b.build()
    assert built.n == n, (built.n, n)
    return built, [rnd.randrange(p) for _ in range(len(built.input_vars))], [rnd.randrange(p)]


def random_layered_hints(curve: str, log_n: int, seed: int):
    """-> (BuiltCircuit of 2^log_n gates after padding, input residues, public-input residues).  Rounds of `width` gates, the old builder
    operations and the hinted ones in turn, operands drawn from everything defined so far; 0, 1 and r - 1 are among the input values."""
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed)
    p = _fr.FIELDS[curve].p
    n = 1 << log_n
    small = ["inv", "div", "root5", "bit", "add"]
    medium = ["add", "inv_or_zero", "mul", "inv", "pow5_lc", "div", "gate", "root5", "lc", "bit", "is_zero", "select", "to_bits", "sub", "mul_add", "is_equal"]
    cost = {"is_zero": 3, "to_bits": 7, "is_equal": 4, "less_than": 19}   # gates per element
    kinds = small if log_n == 3 else medium if log_n == 5 else medium + ["less_than"]
    per_width = sum(cost.get(k, 1) for k in kinds)
    width = 1 if log_n <= 5 else (n - 3) // per_width
    b = BD.CircuitBuilder(curve)
    pub = b.public_input()
    ins = b.input(3 * width)
    pool = np.concatenate([[b.zero, b.one, pub], ins])
    pick = lambda: pool[rs.randint(0, len(pool), size=width)]
    coef = lambda: [rnd.randrange(p) for _ in range(width)]
    for kind in kinds:
        before = b.num_gates
        if kind in ("add", "sub", "mul", "div", "is_equal"):
            new = getattr(b, kind)(pick(), pick())
        elif kind in ("inv", "inv_or_zero", "root5", "is_zero"):
            new = getattr(b, kind)(pick())
        elif kind == "bit":
            new = b.bit(pick(), rs.randint(0, 256, size=width))
        elif kind == "select":
            new = b.select(pick(), pick(), pick())                          # c need not be boolean for the solver
        elif kind == "to_bits":
            new = np.concatenate([np.atleast_1d(v) for v in b.to_bits(pick(), 5)])      # mostly unsatisfied: the solver does not look at constraints
        elif kind == "less_than":
            new = b.less_than(pick(), pick(), 4)
        elif kind == "lc":
            new = b.lc([pick(), pick(), pick(), pick()], [coef(), rnd.randrange(p), coef(), -1], const=coef())
        elif kind == "mul_add":
            new = b.mul_add(pick(), pick(), pick(), pick(), q0=coef(), q1=rnd.randrange(p))
        elif kind == "pow5_lc":
            new = b.pow5_lc([pick(), pick(), pick()], [coef(), 1, coef()], const=rnd.randrange(p))
        else:
            q_o = [(1, p - 1, rnd.randrange(1, p))[min(rnd.randrange(4), 2)] for _ in range(width)]
            sel = {name: coef() for name in BD.SELECTOR_INDEX if name not in ("q_o",)}
            new = b.gate([pick(), pick(), pick(), pick()], {**sel, "q_o": q_o})
        assert b.num_gates - before == cost.get(kind, 1) * width, kind
        pool = np.concatenate([pool, np.atleast_1d(new)])
    built = b.build()
    assert built.n == n, (built.n, n)
    inputs = [rnd.randrange(p) for _ in range(len(built.input_vars))]
    inputs[:3] = [0, 1, p - 1]
    return built, inputs, [rnd.randrange(p)]


PLAIN_KINDS = ["add", "sub", "mul", "lc", "mul_add", "pow5_lc", "gate"]
HINT_KINDS = ["inv", "inv_or_zero", "div", "root5", "bit"]


def layered_circuit(curve: str, depth: int, width: int, seed: int, hints: bool, max_gates: int, satisfied: bool = True):
    """The operations of random_layered / random_layered_hints with the shape chosen by the caller: up to `depth` rounds of `width` gates
    (fewer once `max_gates` gates are used), one operation per round drawn at random; the first operand of a round is, with probability
    3 / 4, the previous round's output, so that the dependency depth follows the number of rounds.  `hints`: the one-gate hinted operations
    (inv, inv_or_zero, div, root5, bit) are in the draw.  satisfied: only constraints that hold are added at the end (one that does not,
    otherwise); every defining gate holds by construction, but an `inv` or `div` hint that meets a zero leaves its own gate unsatisfied,
    so with `hints` the caller asks a reference which gates hold.  -> (BuiltCircuit, input residues, public-input residues); 0, 1 and
    r - 1 are among the input values."""
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed & 0x7FFFFFFF)
    p = _fr.FIELDS[curve].p
    kinds = PLAIN_KINDS + (HINT_KINDS if hints else [])
    b = BD.CircuitBuilder(curve)
    pub = b.public_input()
    ins = np.atleast_1d(b.input(3 * width))
    pool = np.concatenate([[b.zero, b.one, pub], ins])
    last = ins[:width]
    pick = lambda: pool[rs.randint(0, len(pool), size=width)]
    first = lambda: last if rnd.random() < 0.75 else pick()
    coef = lambda: [rnd.randrange(p) for _ in range(width)]
    for _ in range(depth):
        if b.num_gates + width + 4 > max_gates:
            break
        kind = kinds[rnd.randrange(len(kinds))]
        if kind in ("add", "sub", "mul", "div"):
            new = getattr(b, kind)(first(), pick())
        elif kind in ("inv", "inv_or_zero", "root5"):
            new = getattr(b, kind)(first())
        elif kind == "bit":
            new = b.bit(first(), rs.randint(0, 256, size=width))
        elif kind == "lc":
            new = b.lc([first(), pick(), pick(), pick()], [coef(), rnd.randrange(p), coef(), -1], const=coef())
        elif kind == "mul_add":
            new = b.mul_add(first(), pick(), pick(), pick(), q0=coef(), q1=rnd.randrange(p))
        elif kind == "pow5_lc":
            new = b.pow5_lc([first(), pick(), pick()], [coef(), 1, coef()], const=rnd.randrange(p))
        else:
            q_o = [(1, p - 1, rnd.randrange(1, p))[min(rnd.randrange(4), 2)] for _ in range(width)]
            sel = {name: coef() for name in BD.SELECTOR_INDEX if name not in ("q_o",)}
            new = b.gate([first(), pick(), pick(), pick()], {**sel, "q_o": q_o})
        last = np.atleast_1d(new)
        pool = np.concatenate([pool, last])
    x = int(pool[-1])
    b.enforce_equal(x, x)
    b.enforce_bool(b.one)
    b.enforce_constant(b.one, 1)
    if not satisfied:
        b.enforce_constant(b.one, 2)
    built = b.build()
    assert built.n <= max(2, 1 << (max_gates - 1).bit_length()), (built.n, max_gates)
    inputs = [rnd.randrange(p) for _ in range(len(built.input_vars))]
    inputs[:3] = [0, 1, p - 1]
    return built, inputs, [rnd.randrange(p)]


# ---------------------------------------------------------------------------------------------- proved synthetic instances
_CACHE = {}


def _blinders(oracle, cid, seed):
    return dict(wires=oracle.rand_fr(cid, seed, 10).reshape(5, 2, 4), perm=oracle.rand_fr(cid, seed + 1, 3))


def prove_synthetic(w, oracle, cid, log_n, nproofs, seed, num_inputs=3, tau=TAU):
    """(vk, public inputs, [proofs with different blinders]) of one synthetic instance proved on worker `w` under the trapdoor key of `tau`"""
    from distributed_plonk_amd.prover import Prover
    from distributed_plonk_amd.synthetic import SyntheticInstance
    inst = SyntheticInstance(w, log_n, seed=seed, num_inputs=num_inputs, tau=tau)
    pv = Prover(w, log_n)
    try:
        pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
        pub = inst.public_inputs()
        proofs = [pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, _blinders(oracle, cid, 40 + 3 * i), pv.fiat_shamir(pub))
                  for i in range(nproofs)]
        vk = copy.deepcopy(pv.verifying_key())
    finally:
        pv.close()
        inst.close()
    return vk, pub, proofs


def _proved(gpu_workers, oracle, curve, cid, log_n=10, nproofs=3, seed=3):
    """(worker, vk, public inputs, [proofs with different blinders]) of one synthetic instance under the trapdoor key; cached."""
    key = (curve, log_n, nproofs, seed)
    if key not in _CACHE:
        _CACHE[key] = prove_synthetic(gpu_workers(curve), oracle, cid, log_n, nproofs, seed)
    return (gpu_workers(curve),) + _CACHE[key]
