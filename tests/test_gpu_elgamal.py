"""The Rescue sponge, the counter-mode stream and the ElGamal shared key on the device (csrc/elgamal_kernels.hpp behind plonk_rescue_sponge_dev,
plonk_rescue_stream_dev, plonk_edwards_dh_key_dev; distributed_plonk_amd/rescue.py and elgamal.py) against the pure-Python reference
tests/elgamal_ref.py, limb for limb: the sponge at every L around the block size with every n_out, at one lane, three and one lane past a
workgroup; the stream at L around the block size, with a text's blocks straddling a workgroup, there and back, in place, and with a guard
element behind the buffer; the key on the scalars 0, 1, l, r - 1 and random ones and on the identity, G, the points of small order, random
points and one off the curve; whole encryptions and decryptions with an E of small order flagged; injected Edwards and Rescue parameters;
three launches under alternating Rescue tables that are only enqueued; plonk_trim, count 0 and every argument error.

The reference costs ~3 ms per permutation and ~7 ms per scalar multiplication, so each kind of expected value is computed once per curve
for a few distinct operands, and the lanes of a launch repeat them.  tests/test_hostemu_elgamal.py runs a selection of this file on the CPU;
tools/fuzz_abi.py (`--ops wire`) draws the same kernels with random lengths, counts, tables and spoiled ciphertexts between other work."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import edwards as ED
from distributed_plonk_amd import elgamal as EG
from distributed_plonk_amd import rescue as RS
from distributed_plonk_amd._ffi import PlonkError
from tests import edwards_ref as E
from tests import elgamal_ref as G
from tests import rescue_ref as R
from tests.test_gpu_edwards import CIRC_THREADS, from_limbs, lanes, pool, pts_from_limbs, pts_to_limbs, scaled, to_limbs

pytestmark = pytest.mark.gpu

CURVES = [("bn254", 0), ("bls12_381", 1)]
COUNTS = [1, 3, CIRC_THREADS + 1]
SPONGE_LENGTHS = [1, 2, 3, 4, 6, 7]


def texts_to_limbs(curve, rows) -> np.ndarray:
    return to_limbs(curve, [x for row in rows for x in row]).reshape(len(rows), -1, 4)


def texts_from_limbs(curve, limbs) -> list:
    a = np.ascontiguousarray(limbs, dtype=np.uint64)
    flat = from_limbs(curve, a)
    L = a.shape[1]
    return [flat[i * L:(i + 1) * L] for i in range(a.shape[0])]


def other_rescue(curve):
    """-> (RescueParams, the reference's params) with every round key moved: another table of the same structure"""
    M, K = R.default_params(curve)
    K2 = [[(x + 1000 * t + i + 1) % R.MODULI[curve] for i, x in enumerate(row)] for t, row in enumerate(K)]
    return RS.RescueParams(curve, M, K2), (M, K2)


# ---------------------------------------------------------------------------------------------- the sponge
_sponges = {}


def sponge_rows(curve, L, rescue=None, tag="default"):
    """6 distinct messages of L elements and their sponge with n_out = 3 (n_out = 1, 2 are its prefixes), once per curve and L"""
    key = (curve, L, tag)
    if key not in _sponges:
        r = R.MODULI[curve]
        rnd = random.Random(f"gpu sponge {curve} {L}")
        rows = [[0] * L, [r - 1] * L, [1] + [0] * (L - 1)] + [[rnd.randrange(r) for _ in range(L)] for _ in range(3)]
        _sponges[key] = (rows, [G.sponge(curve, row, 3, rescue) for row in rows])
    return _sponges[key]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
@pytest.mark.parametrize("n_out", [1, 2, 3], ids=lambda n: f"out{n}")
@pytest.mark.parametrize("L", SPONGE_LENGTHS, ids=lambda L: f"L{L}")
def test_sponge_matches_the_reference(gpu_workers, curve, cid, L, n_out, count):
    w, prm = gpu_workers(curve), RS.RescueParams.default(curve)
    rows, want = sponge_rows(curve, L)
    idx = lanes(count, len(rows), count)
    got = RS.sponge(w, prm, texts_to_limbs(curve, [rows[i] for i in idx]), n_out)
    assert got.shape == (count, n_out, 4)
    assert texts_from_limbs(curve, got) == [want[i][:n_out] for i in idx]


@pytest.mark.parametrize("curve,cid", CURVES)
def test_sponge_of_three_is_not_hash3(gpu_workers, curve, cid):
    w, prm = gpu_workers(curve), RS.RescueParams.default(curve)
    rows, _ = sponge_rows(curve, 3)
    x = texts_to_limbs(curve, rows)
    s, h = RS.sponge(w, prm, x, 1)[:, 0], RS.hash3(w, prm, x)
    assert not (s == h).all(axis=1).any()
    assert from_limbs(curve, h) == [R.permute(curve, row + [0])[0] for row in rows]


# ---------------------------------------------------------------------------------------------- the stream
_streams = {}


def stream_keys(curve, rescue=None, tag="default"):
    """3 keys and the 9 first elements of each one's keystream, once per curve"""
    if (curve, tag) not in _streams:
        r = R.MODULI[curve]
        keys = [0, r - 1, random.Random("gpu stream " + curve).randrange(r)]
        _streams[(curve, tag)] = (keys, [G.keystream(curve, k, 9, rescue) for k in keys])
    return _streams[(curve, tag)]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("L,count", [(L, c) for L in (1, 3, 4, 7) for c in (1, 3)] + [(7, 100)],
                         ids=[f"L{L}-count{c}" for L in (1, 3, 4, 7) for c in (1, 3)] + ["L7-straddle100"])
def test_stream_there_and_back_in_place_and_within_its_bounds(gpu_workers, curve, cid, L, count):
    """count 100 at L = 7 is 300 lanes: text 85's blocks lie in two workgroups"""
    w, prm = gpu_workers(curve), RS.RescueParams.default(curve)
    r = R.MODULI[curve]
    keys, ks = stream_keys(curve)
    rnd = random.Random(f"texts {curve} {L} {count}")
    idx = lanes(count, len(keys), count)
    texts = [[0] * L, [r - 1] * L][:count] + [[rnd.randrange(r) for _ in range(L)] for _ in range(max(0, count - 2))]
    want = [[(x + z) % r for x, z in zip(t, ks[i][:L])] for t, i in zip(texts, idx)]
    k_limbs, t_limbs = to_limbs(curve, [keys[i] for i in idx]), texts_to_limbs(curve, texts)
    ct = RS.stream(w, prm, k_limbs, t_limbs)
    assert ct.shape == (count, L, 4) and texts_from_limbs(curve, ct) == want
    assert np.array_equal(RS.stream(w, prm, k_limbs, ct, decrypt=True), t_limbs)
    # out of place with a guard element behind the output, then in place over the input
    guard = np.full((1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_k, d_in, d_out = w.alloc(k_limbs.nbytes).upload(k_limbs), w.alloc(t_limbs.nbytes + 32), w.alloc(t_limbs.nbytes + 32)
    try:
        for d in (d_in, d_out):
            d.upload(np.concatenate([t_limbs.reshape(-1, 4), guard]))
        RS.stream_dev(w, prm, d_k.ptr, d_in.ptr, L, count, d_out.ptr)
        out = d_out.download((count * L + 1, 4))
        assert np.array_equal(out[:-1].reshape(ct.shape), ct) and np.array_equal(out[-1:], guard)
        assert np.array_equal(d_in.download((count * L + 1, 4))[:-1].reshape(ct.shape), t_limbs)
        RS.stream_dev(w, prm, d_k.ptr, d_in.ptr, L, count, d_in.ptr)
        out = d_in.download((count * L + 1, 4))
        assert np.array_equal(out[:-1].reshape(ct.shape), ct) and np.array_equal(out[-1:], guard)
        RS.stream_dev(w, prm, d_k.ptr, d_in.ptr, L, count, d_in.ptr, decrypt=True)
        out = d_in.download((count * L + 1, 4))
        assert np.array_equal(out[:-1].reshape(ct.shape), t_limbs) and np.array_equal(out[-1:], guard)
    finally:
        for d in (d_k, d_in, d_out):
            d.free()


# ---------------------------------------------------------------------------------------------- the shared key
_keys = {}


def key_pool(curve):
    """(scalar, point, key) for the scalars 0, 1, l, r - 1 and random ones on a subgroup point and a point outside, r - 1 and a random scalar on
    the identity, the points of order 2, 4, 8, G, -G and random points, and a point off the curve — the products are test_gpu_edwards.py's"""
    if curve not in _keys:
        p, r = pool(curve), E.MODULI[curve]
        n_s = len(p["scalars"])
        assert [p["scalars"][i] for i in (0, 1, 4, 6)] == [0, 1, E.PARAMS[curve]["l"], r - 1]
        pairs = [(i, j) for j in (6, 8) for i in (0, 1, 4)] + [(i, j) for i in (6, n_s - 1) for j in range(len(p["points"]))]
        out = []
        for i, j in pairs:
            S = p["mul"][(i, j)]
            out.append((p["scalars"][i], p["points"][j], R.permute(curve, [S[0], S[1], 0, 0])[0]))
        Gp = E.PARAMS[curve]["G"]
        off = (Gp[0], (Gp[1] + 1) % r)
        assert not E.on_curve(curve, off)
        out.append((p["scalars"][n_s - 1], off, R.permute(curve, [0, 1, 0, 0])[0]))
        assert out[0][2] == out[-1][2]                    # [0] P is the identity too
        _keys[curve] = out
    return _keys[curve]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_dh_key_matches_the_reference(gpu_workers, curve, cid, count):
    w, prm, ops = gpu_workers(curve), ED.EdwardsParams.default(curve), key_pool(curve)
    if count == 3:                                      # l on a point outside the subgroup, r - 1 on the point of order 8, the point off the curve
        ops = [ops[5], ops[9], ops[-1]]
    sel = [ops[i] for i in lanes(count, len(ops), count)]
    got = EG.dh_key(w, prm, to_limbs(curve, [k for k, _, _ in sel]), pts_to_limbs(curve, [P for _, P, _ in sel]))
    assert got.shape == (count, 4) and from_limbs(curve, got) == [x for _, _, x in sel]
    assert [G.dh_key(curve, k, P) for k, P, _ in sel[:1]] == [sel[0][2]]


# ---------------------------------------------------------------------------------------------- the whole scheme
def made(curve, count, L, prm=None, rescue=None, tag="default"):
    """`count` (dk, ek, r, msg, (E, ct)) of the reference"""
    rnd = random.Random(f"gpu elgamal {curve} {L} {tag}")
    r, l = R.MODULI[curve], E.PARAMS[curve]["l"]
    out = []
    for n in range(count):
        dk, rand = rnd.randrange(1, l), (0, l - 1)[n] if n < 2 else rnd.randrange(l)
        msg = [rnd.randrange(r) for _ in range(L)]
        ek = G.keygen(curve, dk, prm)
        out.append((dk, ek, rand, msg, G.encrypt(curve, ek, msg, rand, prm, rescue)))
    return out


def check_scheme(w, curve, prm, rp, cases, ref_prm=None, ref_rescue=None):
    L = len(cases[0][3])
    dk, ek, rand = to_limbs(curve, [c[0] for c in cases]), pts_to_limbs(curve, [c[1] for c in cases]), to_limbs(curve, [c[2] for c in cases])
    msg = texts_to_limbs(curve, [c[3] for c in cases])
    assert pts_from_limbs(curve, EG.keygen(w, prm, dk)) == [c[1] for c in cases]
    Ep, ct = EG.encrypt(w, prm, ek, msg, rand, rp)
    assert pts_from_limbs(curve, Ep) == [c[4][0] for c in cases] and texts_from_limbs(curve, ct) == [c[4][1] for c in cases]
    back, ok = EG.decrypt(w, prm, dk, (Ep, ct), rp)
    assert ok.dtype == bool and ok.tolist() == [True] * len(cases) and np.array_equal(back, msg)
    # an E of small order in the middle: flagged, its message the reference's, the others as before
    small = E.small_order_points(curve, ref_prm)[8]
    bad_E = Ep.copy()
    bad_E[1] = pts_to_limbs(curve, [small])[0]
    back, ok = EG.decrypt(w, prm, dk, (bad_E, ct), rp)
    assert ok.tolist() == [True, False] + [True] * (len(cases) - 2)
    assert np.array_equal(back[0], msg[0]) and np.array_equal(back[2:], msg[2:])
    assert texts_from_limbs(curve, back[1:2]) == [G.decrypt(curve, cases[1][0], (small, cases[1][4][1]), ref_prm, ref_rescue)[0]]
    assert L == back.shape[1]


@pytest.mark.parametrize("curve,cid", CURVES)
@pytest.mark.parametrize("L", [4, 7], ids=lambda L: f"L{L}")
def test_encrypt_equals_the_reference_and_decrypt_recovers_the_message(gpu_workers, curve, cid, L):
    w, prm = gpu_workers(curve), ED.EdwardsParams.default(curve)
    cases = made(curve, 3, L)
    check_scheme(w, curve, prm, None, cases)
    l = E.PARAMS[curve]["l"]
    with pytest.raises(ValueError, match="r\\[2\\] >= l"):
        EG.encrypt(w, prm, pts_to_limbs(curve, [c[1] for c in cases]), texts_to_limbs(curve, [c[3] for c in cases]), to_limbs(curve, [1, l - 1, l]))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_injected_edwards_parameters_and_rescue_tables(gpu_workers, curve, cid):
    """the scaled curve of test_gpu_edwards.py and a RescueParams with other round keys: the scheme, the sponge and the stream under them, and
    the defaults again on the same context"""
    w, sc = gpu_workers(curve), scaled(curve)
    rp, ref_rescue = other_rescue(curve)
    cases = made(curve, 3, 4, sc["ref"], ref_rescue, tag="injected")
    assert cases[2][4] != G.encrypt(curve, cases[2][1], cases[2][3], cases[2][2], sc["ref"])      # the tables matter
    check_scheme(w, curve, sc["prm"], rp, cases, sc["ref"], ref_rescue)
    rows, want = sponge_rows(curve, 4, ref_rescue, tag="injected")
    assert texts_from_limbs(curve, RS.sponge(w, rp, texts_to_limbs(curve, rows), 2)) == [x[:2] for x in want]
    keys, ks = stream_keys(curve, ref_rescue, tag="injected")
    zeros = np.zeros((len(keys), 7, 4), dtype=np.uint64)
    assert texts_from_limbs(curve, RS.stream(w, rp, to_limbs(curve, keys), zeros)) == [z[:7] for z in ks]
    rows, want = sponge_rows(curve, 4)
    assert texts_from_limbs(curve, RS.sponge(w, RS.RescueParams.default(curve), texts_to_limbs(curve, rows), 2)) == [x[:2] for x in want]
    check_scheme(w, curve, ED.EdwardsParams.default(curve), None, made(curve, 3, 4))


@pytest.mark.parametrize("curve,cid", CURVES)
def test_three_dh_key_launches_under_tables_a_b_a_without_a_synchronisation(gpu_workers, curve, cid):
    """the Rescue tables are uploaded again on the context's stream between launches that are only enqueued: each result is its own tables'"""
    w, prm, ops = gpu_workers(curve), ED.EdwardsParams.default(curve), key_pool(curve)
    set_a = RS.RescueParams.default(curve)
    set_b, ref_b = other_rescue(curve)
    sel = [ops[5], ops[9], ops[-1], ops[-2]]
    count = CIRC_THREADS + 1
    idx = [i % len(sel) for i in range(count)]
    want_a = [sel[i][2] for i in idx]
    want_b_of = [G.dh_key(curve, k, P, rescue=ref_b) for k, P, _ in sel]
    want_b = [want_b_of[i] for i in idx]
    assert all(a != b for a, b in zip(want_a, want_b))
    scalars, points = to_limbs(curve, [sel[i][0] for i in idx]), pts_to_limbs(curve, [sel[i][1] for i in idx])
    d_s, d_p = w.alloc(scalars.nbytes).upload(scalars), w.alloc(points.nbytes).upload(points)
    outs = [w.alloc(count * 32) for _ in range(3)]
    try:
        w.sync()
        for rp, out in zip((set_a, set_b, set_a), outs):
            EG.dh_key_dev(w, prm, rp, d_s.ptr, d_p.ptr, count, out.ptr)
        got = [from_limbs(curve, out.download((count, 4))) for out in outs]
        assert got[0] == want_a and got[1] == want_b and got[2] == want_a
    finally:
        d_s.free()
        d_p.free()
        for b in outs:
            b.free()


# ---------------------------------------------------------------------------------------------- trim and arguments
@pytest.mark.parametrize("curve,cid", CURVES)
def test_results_after_trim(gpu_workers, curve, cid):
    w, prm, rp = gpu_workers(curve), ED.EdwardsParams.default(curve), RS.RescueParams.default(curve)
    rows, want = sponge_rows(curve, 4)
    keys, ks = stream_keys(curve)
    ops = key_pool(curve)[5:8]
    zeros = np.zeros((len(keys), 4, 4), dtype=np.uint64)
    for _ in range(2):
        assert texts_from_limbs(curve, RS.sponge(w, rp, texts_to_limbs(curve, rows), 3)) == want
        assert texts_from_limbs(curve, RS.stream(w, rp, to_limbs(curve, keys), zeros)) == [z[:4] for z in ks]
        assert from_limbs(curve, EG.dh_key(w, prm, to_limbs(curve, [k for k, _, _ in ops]), pts_to_limbs(curve, [P for _, P, _ in ops]))) == [x for _, _, x in ops]
        w.trim()


@pytest.mark.parametrize("curve,cid", CURVES)
def test_count_zero_and_argument_errors(gpu_workers, curve, cid):
    w = gpu_workers(curve)
    ed, rs = ED.EdwardsParams.default(curve).limbs(), RS.RescueParams.default(curve).limbs()
    data = np.arange(16 * 4, dtype=np.uint64).reshape(16, 4)
    buf = w.alloc(data.nbytes).upload(data)
    try:
        def fails(call, *mentions):
            with pytest.raises(PlonkError) as e:
                call()
            assert e.value.code == -1, str(e.value)
            for m in mentions:
                assert m in str(e.value), str(e.value)

        p = buf.ptr
        who = "plonk_rescue_sponge_dev"
        fails(lambda: w.rescue_sponge_dev(None, p, 1, 1, 1, p), who, "params")
        fails(lambda: w.rescue_sponge_dev(rs, 0, 1, 1, 1, p), who, "d_inputs")
        fails(lambda: w.rescue_sponge_dev(rs, p, 1, 1, 1, 0), who, "d_out")
        fails(lambda: w.rescue_sponge_dev(rs, p, 0, 1, 1, p), who, "L = 0")
        fails(lambda: w.rescue_sponge_dev(rs, p, 1 << 32, 1, 1, p), who, "L = ")
        fails(lambda: w.rescue_sponge_dev(rs, p, 1, 1, 0, p), who, "n_out = 0")
        fails(lambda: w.rescue_sponge_dev(rs, p, 1, 1, 4, p), who, "n_out = 4")
        fails(lambda: w.rescue_sponge_dev(rs, p, 1, 1 << 40, 1, p), who, "exceed one launch")
        who = "plonk_rescue_stream_dev"
        fails(lambda: w.rescue_stream_dev(None, p, p, 1, 1, False, p), who, "params")
        fails(lambda: w.rescue_stream_dev(rs, 0, p, 1, 1, False, p), who, "d_keys")
        fails(lambda: w.rescue_stream_dev(rs, p, 0, 1, 1, False, p), who, "d_in")
        fails(lambda: w.rescue_stream_dev(rs, p, p, 1, 1, False, 0), who, "d_out")
        fails(lambda: w.rescue_stream_dev(rs, p, p, 0, 1, False, p), who, "L = 0")
        fails(lambda: w.rescue_stream_dev(rs, p, p, 1 << 32, 1, True, p), who, "L = ")
        fails(lambda: w.rescue_stream_dev(rs, p, p, 1, 1 << 40, False, p), who, "exceed one launch")
        fails(lambda: w.rescue_stream_dev(rs, p, p, 3 << 10, 1 << 30, False, p), who, "exceed one launch")       # 2^40 lanes from a count that alone would fit
        who = "plonk_edwards_dh_key_dev"
        fails(lambda: w.edwards_dh_key_dev(None, rs, p, p, 1, p), who, "edwards_params")
        fails(lambda: w.edwards_dh_key_dev(ed, None, p, p, 1, p), who, "rescue_params")
        fails(lambda: w.edwards_dh_key_dev(ed, rs, 0, p, 1, p), who, "d_scalars")
        fails(lambda: w.edwards_dh_key_dev(ed, rs, p, 0, 1, p), who, "d_points")
        fails(lambda: w.edwards_dh_key_dev(ed, rs, p, p, 1, 0), who, "d_keys")
        fails(lambda: w.edwards_dh_key_dev(ed, rs, p, p, 1 << 40, p), who, "exceeds one launch")
        # the no-ops return OK and touch nothing, and an argument error comes before the count is looked at
        w.rescue_sponge_dev(rs, p, 3, 0, 2, p)
        w.rescue_stream_dev(rs, p, p, 3, 0, False, p)
        w.edwards_dh_key_dev(ed, rs, p, p, 0, p)
        fails(lambda: w.rescue_sponge_dev(rs, p, 0, 0, 1, p), "plonk_rescue_sponge_dev", "L = 0")
        assert np.array_equal(buf.download(data.shape), data)
    finally:
        buf.free()
    prm, rp = ED.EdwardsParams.default(curve), RS.RescueParams.default(curve)
    assert RS.sponge(w, rp, np.zeros((0, 5, 4), dtype=np.uint64), 2).shape == (0, 2, 4)
    assert RS.stream(w, rp, np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 5, 4), dtype=np.uint64)).shape == (0, 5, 4)
    assert EG.dh_key(w, prm, np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 2, 4), dtype=np.uint64)).shape == (0, 4)
    Ep, ct = EG.encrypt(w, prm, np.zeros((0, 2, 4), dtype=np.uint64), np.zeros((0, 2, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
    assert Ep.shape == (0, 2, 4) and ct.shape == (0, 2, 4)
    msg, ok = EG.decrypt(w, prm, np.zeros((0, 4), dtype=np.uint64), (Ep, ct))
    assert msg.shape == (0, 2, 4) and ok.shape == (0,)
    other = "bls12_381" if curve == "bn254" else "bn254"
    with pytest.raises(ValueError):
        RS.sponge(w, RS.RescueParams.default(other), np.zeros((1, 1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        EG.dh_key(w, ED.EdwardsParams.default(other), np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 2, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        EG.dh_key(w, prm, np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 2, 4), dtype=np.uint64), rescue=RS.RescueParams.default(other))
    with pytest.raises(ValueError):
        EG.dh_key(w, prm, np.zeros((2, 4), dtype=np.uint64), np.zeros((3, 2, 4), dtype=np.uint64))
