"""The embedded Edwards curves on the device (csrc/edwards_kernels.hpp behind plonk_edwards_mul_dev, plonk_edwards_fixed_mul_dev,
plonk_edwards_add_dev, plonk_edwards_check_dev and distributed_plonk_amd/edwards.py) against the pure-Python reference tests/edwards_ref.py,
limb for limb: the four kernels at counts around the workgroup size, on the scalars 0, 1, 2, l - 1, l, l + 1, r - 1, the single bits at the
seams of the fixed-base table's windows and words, and random ones; on the identity, (0, -1), the points of order 4 and 8, G, -G and random
points inside and outside the subgroup; fixed_mul against mul with G; the flags of points off the curve and outside the subgroup; an injected
generator; count 0 and the argument errors; Schnorr signatures signed and verified on the device, with every rejection; and, at the end of
the file, the four kernels on an isomorphic scaled curve (other a, d and generator than the defaults), mul and add with the output over an
input, the generator's table rebuilt between three launches that are only enqueued, and fixed_mul after plonk_trim and after a round under
a new commit key.  tools/fuzz_abi.py (`--ops curve`) draws the same kernels with random counts, chains and parameter sets.

The reference costs ~20 ms per scalar multiplication, so each kind of expected value is computed once per curve for a few dozen distinct
operands, and the lanes of a launch repeat them.  tests/test_hostemu_edwards.py runs a selection of this file on the CPU."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd._ffi import PlonkError
from tests import edwards_ref as E

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
CIRC_THREADS = 256                                      # csrc/circuit_kernels.hpp
COUNTS = [1, 3, CIRC_THREADS - 1, CIRC_THREADS, CIRC_THREADS + 1]


def to_limbs(curve, values) -> np.ndarray:
    f = _fr.FIELDS[curve]
    raw = b"".join((int(x) % f.p * f.R % f.p).to_bytes(32, "little") for x in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def from_limbs(curve, limbs) -> list:
    f = _fr.FIELDS[curve]
    return [int.from_bytes(row.tobytes(), "little") * f.R_inv % f.p for row in np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)]


def pts_to_limbs(curve, points) -> np.ndarray:
    return to_limbs(curve, [v for P in points for v in P]).reshape(-1, 2, 4)


def pts_from_limbs(curve, limbs) -> list:
    flat = from_limbs(curve, limbs)
    return [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]


_pool = {}


def pool(curve):
    """The distinct operands and their reference results, once per curve:
    scalars / points — the edge values first; mul[(i, j)] = [scalars[i]] points[j] for the pairs of `pairs`; fixed[i] = [scalars[i]] G"""
    if curve not in _pool:
        r, c = E.MODULI[curve], E.PARAMS[curve]
        l, G = c["l"], c["G"]
        rnd = random.Random("gpu edwards " + curve)
        seams = [1 << k for k in (3, 4, 31, 32, 63, 64, 127, 128, 247, 248, 251, 252, 253, 254) if 1 << k < r]
        scalars = [0, 1, 2, l - 1, l, l + 1, r - 1] + seams + [rnd.randrange(r) for _ in range(6)]
        small = E.small_order_points(curve)
        sub = [E.mul(curve, rnd.randrange(1, l), G) for _ in range(2)]
        non = []
        while len(non) < 2:
            P = E.random_point(curve, rnd)
            if not E.in_subgroup(curve, P):
                non.append(P)
        points = [E.IDENTITY, small[2], small[4], small[8], G, E.neg(curve, G)] + sub + non
        # every edge scalar with a random subgroup point and a random point outside; every edge point with r - 1 and a random scalar
        pairs = [(i, 6) for i in range(len(scalars))] + [(i, 8) for i in range(7)] + [(6, j) for j in range(len(points))] + \
                [(len(scalars) - 1, j) for j in range(len(points))]
        pairs = list(dict.fromkeys(pairs))
        _pool[curve] = dict(scalars=scalars, points=points, pairs=pairs, small=small,
                            mul={(i, j): E.mul(curve, scalars[i], points[j]) for i, j in pairs},
                            fixed=[E.mul(curve, k, G) for k in scalars],
                            subgroup=[E.in_subgroup(curve, P) for P in points])
        assert _pool[curve]["subgroup"] == [True, False, False, False, True, True, True, True, False, False]
    return _pool[curve]


def lanes(count, distinct, seed):
    """`count` indices into `distinct` operands: in order first (the edge values in the first lanes), then shuffled repeats, and the first
    three again in the last lanes"""
    idx = [i % distinct for i in range(count)]
    rnd = random.Random(seed)
    tail = idx[distinct:]
    rnd.shuffle(tail)
    idx[distinct:] = tail
    if count > 8:
        idx[-3:] = [0, 1, 2]
    return idx


# ---------------------------------------------------------------------------------------------- the four kernels
@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_mul_matches_the_reference(gpu_workers, curve, cid, count):
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    pairs = [p["pairs"][i] for i in lanes(count, len(p["pairs"]), count)]
    got = ED.mul(w, prm, to_limbs(curve, [p["scalars"][i] for i, _ in pairs]), pts_to_limbs(curve, [p["points"][j] for _, j in pairs]))
    assert got.shape == (count, 2, 4)
    assert pts_from_limbs(curve, got) == [p["mul"][ij] for ij in pairs]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_fixed_mul_matches_the_reference_and_mul_with_the_generator(gpu_workers, curve, cid, count):
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    idx = lanes(count, len(p["scalars"]), count)
    scalars = to_limbs(curve, [p["scalars"][i] for i in idx])
    got = ED.fixed_mul(w, prm, scalars)
    assert got.shape == (count, 2, 4)
    assert pts_from_limbs(curve, got) == [p["fixed"][i] for i in idx]
    assert np.array_equal(got, ED.mul(w, prm, scalars, pts_to_limbs(curve, [E.PARAMS[curve]["G"]] * count)))


_sums = {}


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_add_matches_the_reference(gpu_workers, curve, cid, count):
    """every pair of the pool's points: P + P, P + (-P), the identity on either side, the small orders among themselves"""
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    n = len(p["points"])
    if curve not in _sums:
        _sums[curve] = {(i, j): E.add(curve, p["points"][i], p["points"][j]) for i in range(n) for j in range(n)}
    pairs = [divmod(k, n) for k in lanes(count, n * n, count)]
    a, b = pts_to_limbs(curve, [p["points"][i] for i, _ in pairs]), pts_to_limbs(curve, [p["points"][j] for _, j in pairs])
    got = ED.add(w, prm, a, b)
    assert pts_from_limbs(curve, got) == [_sums[curve][ij] for ij in pairs]
    if count == 3:                                      # in place: d_out = d_p
        buf_p, buf_q = w.alloc(a.nbytes).upload(a), w.alloc(b.nbytes).upload(b)
        try:
            ED.add_dev(w, prm, buf_p.ptr, buf_q.ptr, count, buf_p.ptr)
            assert np.array_equal(buf_p.download(a.shape), got)
        finally:
            buf_p.free()
            buf_q.free()


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_check_flags_curve_and_subgroup(gpu_workers, curve, cid, count):
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    r = E.MODULI[curve]
    G = E.PARAMS[curve]["G"]
    off = [(G[0], (G[1] + 1) % r), (0, 0), (1, 1), (r - 1, r - 1), (G[1], G[0])]
    assert not any(E.on_curve(curve, P) for P in off)
    points = p["points"] + off
    want = [1 | (2 if s else 0) for s in p["subgroup"]] + [0] * len(off)
    idx = lanes(count, len(points), count)
    limbs = pts_to_limbs(curve, [points[i] for i in idx])
    flags = ED.check(w, prm, limbs)
    assert flags.dtype == np.uint32 and flags.tolist() == [want[i] for i in idx]
    assert ED.on_curve(w, prm, limbs).tolist() == [bool(want[i] & 1) for i in idx]
    assert ED.in_subgroup(w, prm, limbs).tolist() == [bool(want[i] & 2) for i in idx]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_two_runs_give_identical_bytes(gpu_workers, curve, cid):
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    scalars = to_limbs(curve, [p["scalars"][i % len(p["scalars"])] for i in range(64)])
    points = pts_to_limbs(curve, [p["points"][i % len(p["points"])] for i in range(64)])
    assert ED.mul(w, prm, scalars, points).tobytes() == ED.mul(w, prm, scalars, points).tobytes()
    assert ED.fixed_mul(w, prm, scalars).tobytes() == ED.fixed_mul(w, prm, scalars).tobytes()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_injected_generator_rebuilds_the_table(gpu_workers, curve, cid):
    """another generator through EdwardsParams(...), then the default one again on the same context"""
    w, c, p = gpu_workers(curve), E.PARAMS[curve], pool(curve)
    G2 = E.mul(curve, 7, c["G"])
    prm2 = ED.EdwardsParams(curve, c["a"], c["d"], G2, c["l"], 8)
    idx = [1, 2, 7, len(p["scalars"]) - 1]
    scalars = to_limbs(curve, [p["scalars"][i] for i in idx])
    assert pts_from_limbs(curve, ED.fixed_mul(w, ED.EdwardsParams.default(curve), scalars)) == [p["fixed"][i] for i in idx]
    assert pts_from_limbs(curve, ED.fixed_mul(w, prm2, scalars)) == [E.mul(curve, 7 * p["scalars"][i], c["G"]) for i in idx]
    assert pts_from_limbs(curve, ED.fixed_mul(w, ED.EdwardsParams.default(curve), scalars)) == [p["fixed"][i] for i in idx]


# ---------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("curve,cid", CURVES)
def test_count_zero_and_argument_errors(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    prm = ED.EdwardsParams.default(curve)
    limbs = prm.limbs()
    data = np.arange(4 * 2 * 4, dtype=np.uint64).reshape(4, 2, 4)
    buf = w.alloc(data.nbytes).upload(data)
    try:
        def fails(call, *mentions):
            with pytest.raises(PlonkError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for m in mentions:
                assert m in str(e.value), str(e.value)

        p = buf.ptr
        fails(lambda: w.edwards_mul_dev(None, p, p, 1, p), "plonk_edwards_mul_dev", "params")
        fails(lambda: w.edwards_mul_dev(limbs, 0, p, 1, p), "plonk_edwards_mul_dev", "d_scalars")
        fails(lambda: w.edwards_mul_dev(limbs, p, 0, 1, p), "plonk_edwards_mul_dev", "d_points")
        fails(lambda: w.edwards_mul_dev(limbs, p, p, 1, 0), "plonk_edwards_mul_dev", "d_out")
        fails(lambda: w.edwards_fixed_mul_dev(None, p, 1, p), "plonk_edwards_fixed_mul_dev", "params")
        fails(lambda: w.edwards_fixed_mul_dev(limbs, 0, 1, p), "plonk_edwards_fixed_mul_dev", "d_scalars")
        fails(lambda: w.edwards_fixed_mul_dev(limbs, p, 1, 0), "plonk_edwards_fixed_mul_dev", "d_out")
        fails(lambda: w.edwards_add_dev(None, p, p, 1, p), "plonk_edwards_add_dev", "params")
        fails(lambda: w.edwards_add_dev(limbs, 0, p, 1, p), "plonk_edwards_add_dev", "d_p")
        fails(lambda: w.edwards_add_dev(limbs, p, 0, 1, p), "plonk_edwards_add_dev", "d_q")
        fails(lambda: w.edwards_add_dev(limbs, p, p, 1, 0), "plonk_edwards_add_dev", "d_out")
        fails(lambda: w.edwards_check_dev(None, p, 1, p), "plonk_edwards_check_dev", "params")
        fails(lambda: w.edwards_check_dev(limbs, 0, 1, p), "plonk_edwards_check_dev", "d_points")
        fails(lambda: w.edwards_check_dev(limbs, p, 1, 0), "plonk_edwards_check_dev", "d_flags")
        fails(lambda: w.edwards_mul_dev(limbs, p, p, 1 << 40, p), "plonk_edwards_mul_dev", "exceeds one launch")
        # the no-ops return OK and touch nothing
        w.edwards_mul_dev(limbs, p, p, 0, p)
        w.edwards_fixed_mul_dev(limbs, p, 0, p)
        w.edwards_add_dev(limbs, p, p, 0, p)
        w.edwards_check_dev(limbs, p, 0, p)
        assert np.array_equal(buf.download(data.shape), data)
    finally:
        buf.free()
    empty = np.zeros((0, 2, 4), dtype=np.uint64)
    assert ED.mul(w, prm, np.zeros((0, 4), dtype=np.uint64), empty).shape == (0, 2, 4) and ED.fixed_mul(w, prm, np.zeros((0, 4), dtype=np.uint64)).shape == (0, 2, 4)
    assert ED.add(w, prm, empty, empty).shape == (0, 2, 4) and ED.check(w, prm, empty).shape == (0,)
    other = ED.EdwardsParams.default("bls12_381" if curve == "bn254" else "bn254")
    with pytest.raises(ValueError):
        ED.fixed_mul(w, other, np.zeros((1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        ED.mul(w, prm, np.zeros((2, 4), dtype=np.uint64), np.zeros((3, 2, 4), dtype=np.uint64))


# ---------------------------------------------------------------------------------------------- Schnorr
@pytest.mark.parametrize("curve,cid", CURVES)
def test_sign_then_verify_with_every_rejection(gpu_workers, curve, cid):
    w, prm = gpu_workers(curve), ED.EdwardsParams.default(curve)
    r, c = E.MODULI[curve], E.PARAMS[curve]
    l, G = c["l"], c["G"]
    rnd = random.Random("schnorr gpu " + curve)
    m = 3
    sks, nonces, msgs = ([rnd.randrange(1, r) for _ in range(m)] for _ in range(3))
    msgs[0] = 0
    pk = ED.keygen(w, prm, to_limbs(curve, sks))
    assert pts_from_limbs(curve, pk) == [E.mul(curve, sk, G) for sk in sks]
    assert ED.in_subgroup(w, prm, pk).all()
    R, s = ED.schnorr_sign(w, prm, to_limbs(curve, sks), to_limbs(curve, nonces), to_limbs(curve, msgs))
    want = [E.schnorr_sign(curve, sk, k, msg) for sk, k, msg in zip(sks, nonces, msgs)]
    assert pts_from_limbs(curve, R) == [Rw for Rw, _ in want] and from_limbs(curve, s) == [sw for _, sw in want]
    m_limbs = to_limbs(curve, msgs)
    assert ED.schnorr_verify(w, prm, pk, m_limbs, (R, s)).tolist() == [True] * m
    # one batch, one defect per signature: s + 1, another message, another pk
    s_int = from_limbs(curve, s)
    bad_s = to_limbs(curve, [(s_int[0] + 1) % l, s_int[1], s_int[2]])
    bad_m = to_limbs(curve, [msgs[0], (msgs[1] + 1) % r, msgs[2]])
    bad_pk = pk.copy()
    bad_pk[2] = pk[0]
    assert ED.schnorr_verify(w, prm, pk, m_limbs, (R, bad_s)).tolist() == [False, True, True]
    assert ED.schnorr_verify(w, prm, pk, bad_m, (R, s)).tolist() == [True, False, True]
    assert ED.schnorr_verify(w, prm, bad_pk, m_limbs, (R, s)).tolist() == [True, True, False]
    # s + l names the same multiple of G and is refused for s >= l; R or pk off the curve
    assert s_int[1] + l < r
    assert ED.schnorr_verify(w, prm, pk, m_limbs, (R, to_limbs(curve, [s_int[0], s_int[1] + l, s_int[2]]))).tolist() == [True, False, True]
    off_R, off_pk = R.copy(), pk.copy()
    off_R[0, 1], off_pk[1, 0] = to_limbs(curve, [(want[0][0][1] + 1) % r])[0], to_limbs(curve, [5])[0]
    assert ED.schnorr_verify(w, prm, pk, m_limbs, (off_R, s)).tolist() == [False, True, True]
    assert ED.schnorr_verify(w, prm, off_pk, m_limbs, (R, s)).tolist() == [True, False, True]


# ---------------------------------------------------------------------------------------------- a scaled curve, aliasing, the table between launches
SCALE_U = 0x1F2E3D4C5B6A79880123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A69 // 3
_scaled = {}


def scaled(curve):
    """The curve (a u^2, d u^2) with the generator (G.x / u, G.y): (x, y) -> (x / u, y) is an isomorphism from the default curve, so a u^2 is
    still a square and d u^2 a non-square.  -> dict(prm: EdwardsParams, ref: the reference's prm=, to: the map, and per kernel the distinct
    operands with the reference's results UNDER prm=, each also equal to the default curve's result carried over), once per curve"""
    if curve not in _scaled:
        r, c, p = E.MODULI[curve], E.PARAMS[curve], pool(curve)
        u = SCALE_U % r
        ui = pow(u, -1, r)
        to = lambda P: (P[0] * ui % r, P[1])
        ref = dict(a=c["a"] * u * u % r, d=c["d"] * u * u % r, cofactor=8, l=c["l"], G=to(c["G"]))
        assert ref["a"] != c["a"] and ref["d"] != c["d"] and E.on_curve(curve, ref["G"], ref)
        n_s = len(p["scalars"])
        pairs = [(3, 6), (5, 8), (6, 3), (n_s - 1, 9), (n_s - 2, 6), (0, 8)]       # l - 1, l + 1, r - 1, 0 and random scalars; order 8, outside, inside
        assert set(pairs) <= set(p["pairs"])
        fixed = [1, 3, 4, 6, 19, n_s - 1]                                           # 1, l - 1, l, r - 1, 2^253, a random one
        checked = [0, 1, 3, 4, 6, 8]
        G = c["G"]
        off = [(G[0], (G[1] + 1) % r), (0, 0), (G[1], G[0])]                        # off the default curve, hence off the scaled one as they map
        out = dict(prm=ED.EdwardsParams(curve, ref["a"], ref["d"], ref["G"], ref["l"], 8), ref=ref, to=to,
                   mul=[(p["scalars"][i], to(p["points"][j]), E.mul(curve, p["scalars"][i], to(p["points"][j]), ref)) for i, j in pairs],
                   fixed=[(p["scalars"][i], E.mul(curve, p["scalars"][i], ref["G"], ref)) for i in fixed],
                   add=[(to(P), to(Q), E.add(curve, to(P), to(Q), ref)) for P in p["points"] for Q in p["points"]],
                   check=[(to(p["points"][j]), 1 | (2 if E.in_subgroup(curve, to(p["points"][j]), ref) else 0)) for j in checked]
                         + [(to(P), 1 if E.on_curve(curve, to(P), ref) else 0) for P in off])
        # the reference's own parameter plumbing: every value above is the default curve's, mapped
        assert [x[2] for x in out["mul"]] == [to(p["mul"][ij]) for ij in pairs]
        assert [x[1] for x in out["fixed"]] == [to(p["fixed"][i]) for i in fixed]
        assert [x[2] for x in out["add"]] == [to(E.add(curve, P, Q)) for P in p["points"] for Q in p["points"]]
        assert [x[1] for x in out["check"]] == [1 | (2 if p["subgroup"][j] else 0) for j in checked] + [0] * len(off)
        _scaled[curve] = out
    return _scaled[curve]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", [3, CIRC_THREADS + 1], ids=lambda c: f"count{c}")
def test_the_four_kernels_on_a_scaled_curve(gpu_workers, curve, cid, count):
    """a and d travel as kernel arguments and are the two defaults in every test above: here another pair, with its own generator"""
    w, sc = gpu_workers(curve), scaled(curve)
    prm = sc["prm"]
    ops = [sc["mul"][i] for i in lanes(count, len(sc["mul"]), count)]
    got = ED.mul(w, prm, to_limbs(curve, [k for k, _, _ in ops]), pts_to_limbs(curve, [P for _, P, _ in ops]))
    assert pts_from_limbs(curve, got) == [x for _, _, x in ops]
    ops = [sc["fixed"][i] for i in lanes(count, len(sc["fixed"]), count)]
    got = ED.fixed_mul(w, prm, to_limbs(curve, [k for k, _ in ops]))
    assert pts_from_limbs(curve, got) == [x for _, x in ops]
    ops = [sc["add"][i] for i in lanes(count, len(sc["add"]), count)]
    got = ED.add(w, prm, pts_to_limbs(curve, [P for P, _, _ in ops]), pts_to_limbs(curve, [Q for _, Q, _ in ops]))
    assert pts_from_limbs(curve, got) == [x for _, _, x in ops]
    ops = [sc["check"][i] for i in lanes(count, len(sc["check"]), count)]
    assert ED.check(w, prm, pts_to_limbs(curve, [P for P, _ in ops])).tolist() == [x for _, x in ops]
    # and the default table comes back on the same context
    p = pool(curve)
    assert pts_from_limbs(curve, ED.fixed_mul(w, ED.EdwardsParams.default(curve), to_limbs(curve, p["scalars"][:3]))) == p["fixed"][:3]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_mul_over_its_points_and_add_over_its_second_operand(gpu_workers, curve, cid):
    """what include/plonk_hip.h promises beside add's d_out == d_p: mul with d_out == d_points, add with d_out == d_q — the bytes of the
    out-of-place launch, which are the reference's"""
    w, prm, p = gpu_workers(curve), ED.EdwardsParams.default(curve), pool(curve)
    pairs = [(3, 6), (6, 3), (len(p["scalars"]) - 1, 9)]
    scalars, points = to_limbs(curve, [p["scalars"][i] for i, _ in pairs]), pts_to_limbs(curve, [p["points"][j] for _, j in pairs])
    others = pts_to_limbs(curve, [p["points"][j] for j in (3, 9, 5)])
    prod, total = ED.mul(w, prm, scalars, points), ED.add(w, prm, points, others)
    assert pts_from_limbs(curve, prod) == [p["mul"][ij] for ij in pairs]
    assert pts_from_limbs(curve, total) == [E.add(curve, p["points"][j], p["points"][k]) for (_, j), k in zip(pairs, (3, 9, 5))]
    bufs = [w.alloc(a.nbytes).upload(a) for a in (scalars, points, points, others)]
    try:
        d_s, d_pts, d_p, d_q = bufs
        ED.mul_dev(w, prm, d_s.ptr, d_pts.ptr, 3, d_pts.ptr)
        ED.add_dev(w, prm, d_p.ptr, d_q.ptr, 3, d_q.ptr)
        assert d_pts.download(points.shape).tobytes() == prod.tobytes()
        assert d_q.download(points.shape).tobytes() == total.tobytes()
        assert d_p.download(points.shape).tobytes() == points.tobytes() and d_s.download(scalars.shape).tobytes() == scalars.tobytes()
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_three_fixed_mul_launches_under_sets_a_b_a_without_a_synchronisation(gpu_workers, curve, cid):
    """the table is rebuilt on the context's stream between launches that are only enqueued: the first launch still reads the old table,
    the second the new one, the third the first again — each result is its own set's"""
    w, sc, p = gpu_workers(curve), scaled(curve), pool(curve)
    set_a, set_b = ED.EdwardsParams.default(curve), sc["prm"]
    idx = [i % len(sc["fixed"]) for i in range(CIRC_THREADS + 1)]
    scalars = to_limbs(curve, [sc["fixed"][i][0] for i in idx])
    want_b = [sc["fixed"][i][1] for i in idx]
    r = E.MODULI[curve]
    want_a = [(P[0] * (SCALE_U % r) % r, P[1]) for P in want_b]     # back through the isomorphism: the default curve's [k] G
    assert want_a[:2] == [p["fixed"][1], p["fixed"][3]]
    d_s = w.alloc(scalars.nbytes).upload(scalars)
    outs = [w.alloc(len(idx) * 64) for _ in range(3)]
    try:
        w.sync()
        for prm, out in zip((set_a, set_b, set_a), outs):
            ED.fixed_mul_dev(w, prm, d_s.ptr, len(idx), out.ptr)
        got = [pts_from_limbs(curve, out.download((len(idx), 2, 4))) for out in outs]
        assert got[0] == want_a and got[1] == want_b and got[2] == want_a
    finally:
        d_s.free()
        for b in outs:
            b.free()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_fixed_mul_after_trim_and_after_a_round_with_a_new_commit_key(oracle, curve, cid):
    """the table is not one of the caches plonk_trim gives back, and neither a new commit key nor the MSM workspace of a round disturbs it
    (a context of its own: the key would outlive the test on the shared one)"""
    from distributed_plonk_amd.worker import PlonkWorker
    p, prm = pool(curve), ED.EdwardsParams.default(curve)
    idx = lanes(40, len(p["scalars"]), 40)
    scalars, want = to_limbs(curve, [p["scalars"][i] for i in idx]), [p["fixed"][i] for i in idx]
    w = PlonkWorker(me=0, device=0, curve=curve)
    try:
        assert pts_from_limbs(curve, ED.fixed_mul(w, prm, scalars)) == want
        w.trim()
        assert pts_from_limbs(curve, ED.fixed_mul(w, prm, scalars)) == want
        n = 64
        bases = oracle.gen_bases(cid, 71, n + 2, n + 2)
        w.init(bases, n, 8 * n)
        evals, bl = oracle.rand_fr(cid, 72, n), oracle.rand_fr(cid, 73, 2)
        poly, cm = oracle.round1(cid, bases, evals, bl, np.zeros(n + 2, dtype=np.uint8), threads=4)
        got_cm = w.round1(evals, bl)
        assert np.array_equal(w.get_wire(n + 2), poly)
        g, o = w.g1_to_affine(got_cm), oracle.jac_to_affine(cid, cm)
        assert g[1] == o[1] and np.array_equal(g[0], o[0])
        assert pts_from_limbs(curve, ED.fixed_mul(w, prm, scalars)) == want
        w.trim()
        sc = scaled(curve)
        assert pts_from_limbs(curve, ED.fixed_mul(w, sc["prm"], to_limbs(curve, [k for k, _ in sc["fixed"]]))) == [x for _, x in sc["fixed"]]
    finally:
        w.close()
