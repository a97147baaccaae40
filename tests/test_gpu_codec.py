"""The byte codec on the device (csrc/codec_kernels.hpp behind plonk_g1_from_bytes_dev, plonk_g1_to_bytes_dev, plonk_fr_*_bytes_dev,
plonk_proofs_from_bytes_dev, plonk_codec_first_bad_dev, plonk_init_bytes; distributed_plonk_amd/codec.py) against the pure-Python reference
tests/codec_ref.py, bit for bit: round trips of SRS points in both forms at one lane, a partial wave, a wave seam and a block seam; 256
seeded random x with every flag; the named values (0, 1, q - 1, q, the largest 30-bit-short value, infinity and its malformed forms, both
flags, an off-curve pair, a sign bit where none belongs); scalars around r; odd strides, poisoned gaps, a shared status word; three enqueued
decodes; count 0 and every argument error; whole proofs with one bad element in the middle; an SRS loaded from bytes.
tests/test_hostemu_codec.py runs a selection of this file on the CPU; tools/fuzz_abi.py (`--only codec`, `--only proof_bytes`) draws the
same entry points with random offsets, strides, element kinds and several defects per batch."""
import random

import numpy as np
import pytest

from distributed_plonk_amd import codec as CD
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import transcript as TR
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd._ffi import PlonkError
from distributed_plonk_amd.transcript import FQ_MODULI
from distributed_plonk_amd.worker import PlonkWorker
from tests import codec_ref as R

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381"]
COUNTS = [1, 3, 65, 257]
ENCS = ["compressed", "uncompressed"]
TAU = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_1122334455667788 >> 3
POISON = 0xA5

_srs = {}


def srs_points(w, curve, n=1024):
    """(xy (n, 2Q) u64 of tau^i G made on the device, the same points as integer pairs), once per curve"""
    if curve not in _srs:
        f = _fr.FIELDS[curve]
        d = w.alloc(n * 16 * w.q64)
        try:
            w.synth_srs(f.to_limbs(TAU % f.p), n, d.ptr)
            w.sync()
            xy = d.download((n, 2 * w.q64))
        finally:
            d.free()
        _srs[curve] = (xy, [to_int_pt(curve, p) for p in xy[:257]])
    return _srs[curve]


def to_int_pt(curve, xy):
    q, n = FQ_MODULI[curve], R.NBYTES[curve] // 8
    if not np.asarray(xy).any():
        return None
    r_inv = pow(pow(2, 64 * n, q), -1, q)
    val = lambda l: sum(int(v) << (64 * i) for i, v in enumerate(l)) * r_inv % q
    return val(xy[:n]), val(xy[n:])


def want_limbs(curve, pts):
    return np.array([R.g1_limbs(curve, p) for p in pts], dtype=np.uint64).reshape(len(pts), -1)


def decode_and_compare(w, curve, blobs, encoding, check_subgroup):
    """every blob through the device and through the reference: same limbs, same status; returns the statuses"""
    xy, st = CD.g1_from_bytes(w, b"".join(blobs), encoding, check_subgroup)
    ref = [R.g1_decode(curve, b, encoding, check_subgroup) for b in blobs]
    assert [int(s) for s in st] == [s for _, s in ref]
    assert np.array_equal(xy, want_limbs(curve, [p for p, _ in ref]))
    return [s for _, s in ref]


# ---------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("encoding", ENCS)
@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
def test_round_trip_of_srs_points(gpu_workers, curve, encoding, count):
    w = gpu_workers(curve)
    xy, pts = srs_points(w, curve)
    blob = CD.g1_to_bytes(w, xy[:count], encoding)
    nb = CD.g1_nbytes(curve, encoding)
    assert blob == b"".join(R.g1_encode(curve, p, encoding) for p in pts[:count])
    if encoding == "compressed":
        assert blob == b"".join(TR.serialize_g1(curve, xy[i], False) for i in range(count))
    if count == 257 and encoding == "compressed":
        signs = {blob[nb * i + nb - 1] & 0x80 for i in range(count)}
        assert signs == {0, 0x80}                  # both signs of y occur
    got, st = CD.g1_from_bytes(w, blob, encoding, True)
    assert not st.any() and np.array_equal(got, xy[:count])


@pytest.mark.parametrize("curve", CURVES)
def test_infinity_round_trip_and_host_encoder(gpu_workers, curve):
    w = gpu_workers(curve)
    xy, _ = srs_points(w, curve)
    three = np.stack([xy[1], np.zeros_like(xy[0]), xy[2]])
    for encoding in ENCS:
        blob = CD.g1_to_bytes(w, three, encoding)
        nb = CD.g1_nbytes(curve, encoding)
        assert blob[nb:2 * nb] == bytes(nb - 1) + b"\x40" == R.g1_encode(curve, None, encoding)
        assert blob == b"".join(CD.g1_encode_host(curve, p, encoding) for p in three)
        got, st = CD.g1_from_bytes(w, blob, encoding)
        assert not st.any() and np.array_equal(got, three)


# ---------------------------------------------------------------------------------------------- random x
@pytest.mark.parametrize("curve", CURVES)
def test_random_x_with_each_flag(gpu_workers, curve):
    w = gpu_workers(curve)
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    rnd = random.Random(0x434f4445 + len(curve))
    xs = [rnd.randrange(q) for _ in range(256)]
    for flag in (0, 0x80, 0x40, 0xC0):
        blobs = [bytes(bytearray(x.to_bytes(nb, "little")[:-1]) + bytes([x.to_bytes(nb, "little")[-1] | flag])) for x in xs]
        sts = decode_and_compare(w, curve, blobs, "compressed", False)
        if flag in (0, 0x80):
            ok = sum(s == 0 for s in sts)
            assert ok == {"bn254": 122, "bls12_381": 125}[curve]
            assert ok >= 64 and sum(s == 1 for s in sts) >= 64 and ok + sum(s == 1 for s in sts) == 256
        else:
            assert sts == [8] * 256
    # a random x of BLS12-381 that has a point has one outside the subgroup: 16 of them with the check
    blobs = [x.to_bytes(nb, "little") for x in xs[:16]]
    sts = decode_and_compare(w, curve, blobs, "compressed", True)
    assert set(sts) <= ({0, 1} if curve == "bn254" else {1, 2})


# ---------------------------------------------------------------------------------------------- named values
def named_cases(curve):
    """[(name, blob, encoding, check_subgroup, the status it must have)]; the limbs are the reference's"""
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    le = lambda v: v.to_bytes(nb, "little")
    flag = lambda b, f: b[:-1] + bytes([b[-1] | f])
    gx, gy = VF._G1_GEN[curve]
    cases = []
    if curve == "bls12_381":                      # (0, +-2): on the curve, of order 3
        cases += [("x0 checked", le(0), "compressed", True, 2), ("x0 unchecked", le(0), "compressed", False, 0),
                  ("x0 sign unchecked", flag(le(0), 0x80), "compressed", False, 0),
                  ("x0 pair checked", le(0) + le(2), "uncompressed", True, 2), ("x0 pair unchecked", le(0) + le(2), "uncompressed", False, 0)]
    else:                                         # y^2 = 3 has no root mod q
        cases += [("x0", le(0), "compressed", True, 1), ("x1 generator", le(1), "compressed", True, 0),
                  ("x1 generator negated", flag(le(1), 0x80), "compressed", True, 0)]
    cases += [("generator", R.g1_encode(curve, (gx, gy)), "compressed", True, 0),
              ("generator pair", le(gx) + le(gy), "uncompressed", True, 0),
              ("x q-1", le(q - 1), "compressed", False, R.g1_decode(curve, le(q - 1), "compressed", False)[1]),
              ("x q", le(q), "compressed", True, 8),
              ("x all ones", le(2 ** (8 * nb - 2) - 1), "compressed", True, 8),
              ("pair x q", le(q) + le(gy), "uncompressed", True, 8), ("pair y q", le(gx) + le(q), "uncompressed", True, 8),
              ("infinity", flag(le(0), 0x40), "compressed", True, 0), ("infinity pair", le(0) + flag(le(0), 0x40), "uncompressed", True, 0),
              ("infinity with sign", flag(le(0), 0xC0), "compressed", True, 8), ("infinity x1", flag(le(1), 0x40), "compressed", True, 8),
              ("infinity pair y1", le(0) + flag(le(1), 0x40), "uncompressed", True, 8),
              ("infinity pair x1", le(1) + flag(le(0), 0x40), "uncompressed", True, 8),
              ("both flags", flag(le(gx), 0xC0), "compressed", True, 8),
              ("pair y+1", le(gx) + le(gy + 1), "uncompressed", True, 1),
              ("pair with sign", le(gx) + flag(le(gy), 0x80), "uncompressed", True, 8),
              ("pair negated", le(gx) + le(q - gy), "uncompressed", True, 0)]
    return cases


@pytest.mark.parametrize("curve", CURVES)
def test_named_values(gpu_workers, curve):
    w = gpu_workers(curve)
    cases = named_cases(curve)
    assert R.g1_decode(curve, cases[-1][1], "uncompressed")[0][1] == FQ_MODULI[curve] - VF._G1_GEN[curve][1]
    for encoding in ENCS:
        for check in (True, False):
            sel = [c for c in cases if c[2] == encoding and c[3] == check]
            if sel:
                sts = decode_and_compare(w, curve, [c[1] for c in sel], encoding, check)
                assert sts == [c[4] for c in sel], [c[0] for c, s in zip(sel, sts) if s != c[4]]


@pytest.mark.parametrize("curve", CURVES)
def test_fr_values(gpu_workers, curve):
    w = gpu_workers(curve)
    r = R.fr_modulus(curve)
    rnd = random.Random("codec fr " + curve)
    vals = [0, 1, r - 1, r, 2 ** 256 - 1] + [rnd.randrange(r) for _ in range(60)] + [rnd.randrange(r, 2 ** 256) for _ in range(4)]
    blob = b"".join(v.to_bytes(32, "little") for v in vals)
    limbs, st = CD.fr_from_bytes(w, blob)
    ref = [R.fr_decode(curve, v.to_bytes(32, "little")) for v in vals]
    assert [int(s) for s in st] == [s for _, s in ref] and [int(s) for s in st[:5]] == [0, 0, 0, 8, 8]
    assert np.array_equal(limbs, np.array([R.limbs_of(curve, v or 0, "r") for v, _ in ref], dtype=np.uint64))
    good = [i for i, (_, s) in enumerate(ref) if s == 0]
    back = CD.fr_to_bytes(w, limbs[good])
    assert back == b"".join(vals[i].to_bytes(32, "little") for i in good)
    assert back == b"".join(TR.serialize_fr(curve, limbs[i]) for i in good)


# ---------------------------------------------------------------------------------------------- strides, offsets, shared status
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("pad", [1, 7])
def test_strides_gaps_and_a_shared_status_word(gpu_workers, curve, pad):
    w = gpu_workers(curve)
    xy, pts = srs_points(w, curve)
    count, nb, n2 = 67, R.NBYTES[curve], 2 * w.q64
    blobs = [R.g1_encode(curve, p) for p in pts[:count]]
    blobs[40] = (FQ_MODULI[curve]).to_bytes(nb, "little")                       # status 8
    raw = np.full(3 + count * (nb + pad), POISON, np.uint8)                     # elements at odd addresses, nb + pad apart
    for i, b in enumerate(blobs):
        raw[3 + i * (nb + pad):3 + i * (nb + pad) + nb] = np.frombuffer(b, np.uint8)
    out_stride = n2 + 3
    d_in, d_out, d_st = w.alloc(raw.nbytes).upload(raw), w.alloc(count * out_stride * 8), w.alloc(count * 4 + 8)
    try:
        w.memset_dev(d_out.ptr, POISON, count * out_stride * 8)
        w.memset_dev(d_st.ptr, 0, count * 4 + 8)
        CD.g1_from_bytes_dev(w, d_in.ptr + 3, count, d_out.ptr, d_st.ptr, in_stride=nb + pad, out_stride_u64=out_stride, status_stride=1)
        CD.g1_from_bytes_dev(w, d_in.ptr + 3, count, d_out.ptr, d_st.ptr + count * 4, in_stride=nb + pad, out_stride_u64=out_stride, status_stride=0)
        w.sync()
        got = d_out.download((count, out_stride))
        st = d_st.download((count + 2,), dtype=np.uint32)
        want = want_limbs(curve, pts[:count])
        want[40] = 0
        assert np.array_equal(got[:, :n2], want)
        assert (got[:, n2:] == np.uint64(int.from_bytes(bytes([POISON] * 8), "little"))).all()      # the gaps are untouched
        assert [int(s) for s in st[:count]] == [8 if i == 40 else 0 for i in range(count)]
        assert int(st[count]) == 8 and int(st[count + 1]) == 0                                        # one word for all, its neighbour untouched
        assert w.codec_first_bad_dev(d_st.ptr, count) == 40 and w.codec_first_bad_dev(d_st.ptr, 40) == -1
        assert w.codec_first_bad_dev(d_st.ptr, 21, 2) == 20                                           # every second word: 40 is the 20th
        # encode into a strided, poisoned buffer
        d_b = w.alloc(5 + count * (nb + pad))
        try:
            w.memset_dev(d_b.ptr, POISON, 5 + count * (nb + pad))
            CD.g1_to_bytes_dev(w, d_out.ptr, count, d_b.ptr + 5, in_stride_u64=out_stride, out_stride=nb + pad)
            w.sync()
            back = d_b.download((5 + count * (nb + pad),), dtype=np.uint8)
        finally:
            d_b.free()
        assert (back[:5] == POISON).all()
        for i in range(count):
            at = 5 + i * (nb + pad)
            assert back[at:at + nb].tobytes() == (R.g1_encode(curve, None) if i == 40 else blobs[i]) and (back[at + nb:at + nb + pad] == POISON).all()
    finally:
        for b in (d_in, d_out, d_st):
            b.free()


@pytest.mark.parametrize("curve", CURVES)
def test_three_enqueued_decodes(gpu_workers, curve):
    w = gpu_workers(curve)
    xy, pts = srs_points(w, curve)
    nb, n2 = R.NBYTES[curve], 2 * w.q64
    parts = [(0, 5), (5, 70), (70, 73)]
    bufs = []
    try:
        for a, b in parts:
            raw = np.frombuffer(b"".join(R.g1_encode(curve, p) for p in pts[a:b]), np.uint8)
            d_in, d_out, d_st = w.alloc(raw.nbytes).upload(raw), w.alloc((b - a) * n2 * 8), w.alloc((b - a) * 4)
            bufs += [d_in, d_out, d_st]
            w.memset_dev(d_st.ptr, 0, (b - a) * 4)
        for k, (a, b) in enumerate(parts):
            CD.g1_from_bytes_dev(w, bufs[3 * k].ptr, b - a, bufs[3 * k + 1].ptr, bufs[3 * k + 2].ptr)
        w.sync()
        for k, (a, b) in enumerate(parts):
            assert np.array_equal(bufs[3 * k + 1].download((b - a, n2)), xy[a:b]) and not bufs[3 * k + 2].download((b - a,), dtype=np.uint32).any()
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("curve", CURVES)
def test_count_zero_and_argument_errors(gpu_workers, curve):
    w = gpu_workers(curve)
    nb, n2 = R.NBYTES[curve], 2 * w.q64
    d = w.alloc(4096)
    try:
        w.memset_dev(d.ptr, POISON, 4096)
        p = d.ptr
        # count 0: nothing launched, nothing needed
        w.g1_from_bytes_dev(0, nb, 0, 0, True, 0, n2, 0, 1)
        w.g1_to_bytes_dev(0, n2, 0, 0, 0, nb)
        w.fr_from_bytes_dev(0, 32, 0, 0, 4, 0, 1)
        w.fr_to_bytes_dev(0, 4, 0, 0, 32)
        w.proofs_from_bytes_dev(0, 0, 0, 0)
        assert w.codec_first_bad_dev(0, 0) == -1
        assert CD.g1_from_bytes(w, b"")[0].shape == (0, n2) and CD.g1_to_bytes(w, np.zeros((0, n2), np.uint64)) == b"" and CD.fr_to_bytes(w, []) == b""
        calls = [lambda: w.g1_from_bytes_dev(0, nb, 1, 0, True, p, n2, p, 1), lambda: w.g1_from_bytes_dev(p, nb, 1, 0, True, 0, n2, p, 1),
                 lambda: w.g1_from_bytes_dev(p, nb, 1, 0, True, p, n2, 0, 1), lambda: w.g1_from_bytes_dev(p, nb - 1, 1, 0, True, p, n2, p, 1),
                 lambda: w.g1_from_bytes_dev(p, 2 * nb - 1, 1, 1, True, p, n2, p, 1), lambda: w.g1_from_bytes_dev(p, nb, 1, 0, True, p, n2 - 1, p, 1),
                 lambda: w.g1_from_bytes_dev(p, nb, 1, 2, True, p, n2, p, 1), lambda: w.g1_from_bytes_dev(p, nb, 1, -1, True, p, n2, p, 1),
                 lambda: w.g1_to_bytes_dev(0, n2, 1, 0, p, nb), lambda: w.g1_to_bytes_dev(p, n2, 1, 0, 0, nb), lambda: w.g1_to_bytes_dev(p, n2 - 1, 1, 0, p, nb),
                 lambda: w.g1_to_bytes_dev(p, n2, 1, 0, p, nb - 1), lambda: w.g1_to_bytes_dev(p, n2, 1, 1, p, 2 * nb - 1), lambda: w.g1_to_bytes_dev(p, n2, 1, 7, p, nb),
                 lambda: w.fr_from_bytes_dev(0, 32, 1, p, 4, p, 1), lambda: w.fr_from_bytes_dev(p, 32, 1, 0, 4, p, 1), lambda: w.fr_from_bytes_dev(p, 32, 1, p, 4, 0, 1),
                 lambda: w.fr_from_bytes_dev(p, 31, 1, p, 4, p, 1), lambda: w.fr_from_bytes_dev(p, 32, 1, p, 3, p, 1),
                 lambda: w.fr_to_bytes_dev(0, 4, 1, p, 32), lambda: w.fr_to_bytes_dev(p, 4, 1, 0, 32), lambda: w.fr_to_bytes_dev(p, 3, 1, p, 32),
                 lambda: w.fr_to_bytes_dev(p, 4, 1, p, 31),
                 lambda: w.proofs_from_bytes_dev(0, 1, p, p), lambda: w.proofs_from_bytes_dev(p, 1, 0, p), lambda: w.proofs_from_bytes_dev(p, 1, p, 0),
                 lambda: w.codec_first_bad_dev(0, 1)]
        for i, call in enumerate(calls):
            with pytest.raises(PlonkError) as e:
                call()
            assert e.value.code == -1, i
        assert w.lib.plonk_codec_first_bad_dev(w.ctx, p, 1, 1, None) == -1
        w.sync()
        assert (d.download((4096,), dtype=np.uint8) == POISON).all()               # a refused call wrote nothing
        with pytest.raises(ValueError):
            CD.g1_from_bytes(w, bytes(nb + 1))
        with pytest.raises(ValueError):
            CD.fr_from_bytes(w, bytes(33))
        with pytest.raises(ValueError):
            CD.proofs_from_bytes_dev(w, [bytes(CD.proof_nbytes(curve) - 1)])
        with pytest.raises(ValueError):
            CD.commitments_from_bytes(w, (3).to_bytes(8, "little") + bytes(2 * nb))
        with pytest.raises((ValueError, KeyError)):
            w.init_bytes(bytes(nb), 1, 4, 32, encoding="packed")
        with pytest.raises(ValueError):
            w.init_bytes(bytes(nb + 1), 1, 4, 32)
    finally:
        d.free()


# ---------------------------------------------------------------------------------------------- proofs, Vec<Commitment>
def made_proofs(w, curve, K):
    """K proofs put together from SRS points (one of them infinity) and seeded scalars: nothing the decoder could tell from proved ones"""
    xy, _ = srs_points(w, curve)
    f = _fr.FIELDS[curve]
    rnd = random.Random(f"codec proofs {curve}")
    out = []
    for k in range(K):
        pts = [(xy[1 + 13 * k + i].copy(), False) for i in range(13)]
        if k == 1:
            pts[3] = (np.zeros_like(xy[0]), True)
        ev = [f.to_limbs(rnd.randrange(f.p)) for _ in range(10)]
        out.append({"wires_poly_comms": pts[:5], "prod_perm_poly_comm": pts[5], "split_quot_poly_comms": pts[6:11], "opening_proof": pts[11],
                    "shifted_opening_proof": pts[12], "wires_evals": ev[:5], "wire_sigma_evals": ev[5:9], "perm_next_eval": ev[9]})
    return out


def point_at(curve, i):
    nb = R.NBYTES[curve]
    return (8 if i < 6 else 16) + i * nb


def eval_at(curve, j):
    return 16 + 13 * R.NBYTES[curve] + (8 if j < 5 else 16) + 32 * j


def no_point_x(curve):
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    x = next(x for x in range(2, 100) if R.g1_decode(curve, x.to_bytes(nb, "little"), "compressed", False)[1] == 1)
    return x.to_bytes(nb, "little")


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("K", [1, 3, 5], ids=lambda k: f"K{k}")
def test_proofs_from_bytes(gpu_workers, curve, K):
    w = gpu_workers(curve)
    nb, n2 = R.NBYTES[curve], 2 * w.q64
    proofs = made_proofs(w, curve, K)
    blobs = [TR.serialize_proof(curve, p) for p in proofs]
    assert all(len(b) == CD.proof_nbytes(curve) for b in blobs)
    want = np.stack([VF.proof_record(curve, p) for p in proofs])
    mid = K // 2

    def run(bl):
        d, st = CD.proofs_from_bytes_dev(w, bl)
        try:
            return d.download(want.shape), [int(s) for s in st]
        finally:
            d.free()

    got, st = run(blobs)
    assert st == [0] * K and np.array_equal(got, want)
    back = CD.proof_from_bytes(w, blobs[mid])
    assert np.array_equal(VF.proof_record(curve, back), want[mid]) and TR.serialize_proof(curve, back) == blobs[mid]
    assert back["wires_poly_comms"][3][1] == (mid == 1)
    # one bad element in the middle proof: its status, its zeroed element, every other record exact
    for what, at, patch, status, zero in (("point", point_at(curve, 7), no_point_x(curve), 1, slice(7 * n2, 8 * n2)),
                                          ("first point", point_at(curve, 0), no_point_x(curve), 1, slice(0, n2)),
                                          ("scalar", eval_at(curve, 6), R.fr_modulus(curve).to_bytes(32, "little"), 8, slice(13 * n2 + 24, 13 * n2 + 28)),
                                          ("last scalar", eval_at(curve, 9), bytes([255] * 32), 8, slice(13 * n2 + 36, 13 * n2 + 40)),
                                          ("prefix", 8 + 6 * nb, (4).to_bytes(8, "little"), 16, None),
                                          ("last prefix", 16 + 13 * nb + 8 + 160, (5).to_bytes(8, "little"), 16, None)):
        bad = list(blobs)
        bad[mid] = bad[mid][:at] + patch + bad[mid][at + len(patch):]
        got, st = run(bad)
        exp = want.copy()
        if zero is not None:
            exp[mid, zero] = 0
        assert st == [status if k == mid else 0 for k in range(K)], what
        assert np.array_equal(got, exp), what
        with pytest.raises(ValueError, match=f"status {status}"):
            CD.proof_from_bytes(w, bad[mid])


@pytest.mark.parametrize("curve", CURVES)
def test_commitments_from_bytes(gpu_workers, curve):
    w = gpu_workers(curve)
    xy, pts = srs_points(w, curve)
    comms = [(xy[i].copy(), False) for i in range(1, 13)] + [(np.zeros_like(xy[0]), True)]
    blob = len(comms).to_bytes(8, "little") + b"".join(TR.serialize_g1(curve, *c) for c in comms)
    got = CD.commitments_from_bytes(w, blob)
    assert len(got) == 13 and all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, comms))
    with pytest.raises(ValueError, match="element 4"):
        CD.commitments_from_bytes(w, blob[:8 + 4 * R.NBYTES[curve]] + no_point_x(curve) + blob[8 + 5 * R.NBYTES[curve]:])


# ---------------------------------------------------------------------------------------------- an SRS from bytes
@pytest.mark.parametrize("curve", CURVES)
def test_init_bytes_commits_like_init(gpu_workers, curve):
    w = gpu_workers(curve)
    n = 1 << 10
    xy, _ = srs_points(w, curve)
    f = _fr.FIELDS[curve]
    rnd = random.Random("codec init " + curve)
    coeffs = np.stack([f.to_limbs(rnd.randrange(f.p)) for _ in range(n)])
    w2 = PlonkWorker(me=0, device=0, curve=curve)
    try:
        w2.init(xy, n, 8 * n)
        want = w2.g1_to_affine(w2.commit(coeffs))
        for encoding in ENCS:
            blob = CD.g1_to_bytes(w, xy, encoding)                 # encoded on the device
            w2.init(None, n, 8 * n)
            w2.init_bytes(blob, n, n, 8 * n, encoding=encoding)
            got = w2.g1_to_affine(w2.commit(coeffs))
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and not got[1]
        # point 517 spoiled: refused by index, and no bases are left behind
        nb = R.NBYTES[curve]
        blob = CD.g1_to_bytes(w, xy, "compressed")
        bad = blob[:517 * nb] + no_point_x(curve) + blob[518 * nb:]
        with pytest.raises(PlonkError, match="517") as e:
            w2.init_bytes(bad, n, n, 8 * n)
        assert e.value.code == -1 and "status 1" in str(e.value)
        assert w2.g1_to_affine(w2.commit(coeffs))[1]              # no bases: the empty commitment
        d = w2.alloc(32)
        try:
            with pytest.raises(PlonkError, match="resident bases"):
                w2.msm_dev(0, 1, d.ptr)
        finally:
            d.free()
        w2.init_bytes(blob, n, n, 8 * n)
        assert np.array_equal(w2.g1_to_affine(w2.commit(coeffs))[0], want[0])
    finally:
        w2.close()
