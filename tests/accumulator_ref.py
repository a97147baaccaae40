"""A pure-Python reference of the ternary Rescue accumulator (a helper of the accumulator tests, not a test; imports tests/rescue_ref.py
only, no project code).

    hash3(a, b, c) = permute((a, b, c, 0))[0]

Acc(height, elems[0 .. count)), 1 <= height <= 40, 1 <= count <= 3^height: a sparse, append-only, 3-ary Merkle tree.
    level 0     c_0 = count nodes:                node_0[i]     = hash3(0, i, elems[i])              (the uid i as a field element)
    level j+1   c_{j+1} = ceil(c_j / 3) nodes:    node_{j+1}[t] = hash3(x_0, x_1, x_2),   x_k = node_j[3t+k] if 3t+k < c_j else 0
An empty subtree has the value 0 — NOT hash3(0, 0, 0) — and no all-empty node is ever computed.  The root is node_height[0]; once a level
holds one node the rest is the chain hash3(x, 0, 0).

Path of uid i, for j = 0 .. height-1: pos_j = floor(i / 3^j) mod 3; the group of three at level j starts at g = 3 floor(i / 3^(j+1));
sib1_j, sib2_j are the two OTHER members of the group in ascending position (0 beyond c_j); is_left_j = [pos_j = 0], is_right_j = [pos_j = 2]."""
try:
    from tests import rescue_ref as R
except ImportError:                                   # run from tools/ with tests/ on the path
    import rescue_ref as R

MODULI, CURVES = R.MODULI, R.CURVES
MAX_HEIGHT = 40


def hash3(curve: str, a: int, b: int, c: int, params=None) -> int:
    return R.permute(curve, [a, b, c, 0], params)[0]


def level_counts(height: int, count: int) -> list:
    """c_0 .. c_height"""
    assert 1 <= height <= MAX_HEIGHT and 1 <= count <= 3 ** height
    cs = [count]
    for _ in range(height):
        cs.append((cs[-1] + 2) // 3)
    assert cs[-1] == 1
    return cs


def acc_nodes(curve: str, height: int, elems, params=None) -> list:
    """-> height + 1 lists, the nodes of level 0 (the leaf hashes) .. level `height` (the root alone)"""
    r = MODULI[curve]
    params = params or R.default_params(curve)
    cs = level_counts(height, len(elems))
    levels = [[hash3(curve, 0, i % r, int(e), params) for i, e in enumerate(elems)]]
    for j in range(height):
        below = levels[-1]
        at = lambda i: below[i] if i < len(below) else 0
        levels.append([hash3(curve, at(3 * t), at(3 * t + 1), at(3 * t + 2), params) for t in range(cs[j + 1])])
    assert [len(l) for l in levels] == cs
    return levels


def acc_path(levels, uid: int):
    """-> (sib1s, sib2s, positions), one entry per level from the leaves up; positions[j] in (0, 1, 2)"""
    assert 0 <= uid < len(levels[0])
    sib1, sib2, pos = [], [], []
    for j in range(len(levels) - 1):
        lvl = levels[j]
        p = uid // 3 ** j % 3
        g = 3 * (uid // 3 ** (j + 1))
        others = [lvl[g + k] if g + k < len(lvl) else 0 for k in range(3) if k != p]
        sib1.append(others[0])
        sib2.append(others[1])
        pos.append(p)
    return sib1, sib2, pos


def root_from_path(curve: str, uid: int, elem: int, sib1s, sib2s, positions, params=None) -> int:
    cur = hash3(curve, 0, uid % MODULI[curve], elem, params)
    for s1, s2, p in zip(sib1s, sib2s, positions):
        assert p in (0, 1, 2)
        group = [s1, s2]
        group.insert(p, cur)
        cur = hash3(curve, *group, params)
    return cur


def fixture_elems(curve: str) -> list:
    """the 10 elems of tests/golden/accumulator_<curve>.json: 0 first, r - 1 last, 8 seeded random between"""
    import random
    r = MODULI[curve]
    rnd = random.Random("accumulator fixture " + curve)
    return [0] + [rnd.randrange(r) for _ in range(8)] + [r - 1]
