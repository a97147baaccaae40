"""The byte codec without a GPU: the pure-Python reference tests/codec_ref.py against the encoders tests/test_transcript.py already pins
(transcript.serialize_g1 / serialize_fr), and the host-only G2 entry points plonk_g2_from_bytes / plonk_g2_to_bytes against the reference —
the generator, multiples with both signs of y (the flag compares c1 first), twist points whose y lies in Fq (y.c1 = 0: the tie, decided by c0,
and the c1 = 0 branch of the Fq2 root) or in u Fq (y.c0 = 0), infinity, a twist point outside the subgroup, an x without a point,
non-canonical forms.  OpenKey.from_bytes, and the argument errors of the forms that need no device."""
import random
import types

import numpy as np
import pytest

from distributed_plonk_amd import codec as CD
from distributed_plonk_amd import fr as _fr
from distributed_plonk_amd import transcript as TR
from distributed_plonk_amd import verifier as VF
from distributed_plonk_amd.transcript import FQ_MODULI
from tests import codec_ref as R

CURVES = ["bn254", "bls12_381"]


def _multiples(curve, count, seed):
    rnd = random.Random(f"codec host {curve} {seed}")
    g = VF._G1_GEN[curve]
    return [R.g1_mul(curve, rnd.randrange(1, R.fr_modulus(curve)), g) for _ in range(count)]


@pytest.mark.parametrize("curve", CURVES)
def test_reference_encoder_is_the_transcript_encoder(curve):
    q = FQ_MODULI[curve]
    g = VF._G1_GEN[curve]
    pts = [g, (g[0], q - g[1]), None] + _multiples(curve, 64, 0)
    signs = set()
    for p in pts:
        limbs = np.array(R.g1_limbs(curve, p), dtype=np.uint64)
        enc = R.g1_encode(curve, p)
        assert enc == TR.serialize_g1(curve, limbs, p is None) == CD.g1_encode_host(curve, limbs)
        assert R.g1_encode(curve, p, "uncompressed") == CD.g1_encode_host(curve, limbs, "uncompressed")
        signs.add(enc[-1] & 0xC0)
        for encoding in ("compressed", "uncompressed"):
            assert R.g1_decode(curve, R.g1_encode(curve, p, encoding), encoding) == (p, 0)
    assert signs == {0, 0x80, 0x40}
    assert np.array_equal(VF.g1_generator(curve), np.array(R.g1_limbs(curve, g), dtype=np.uint64))
    f = _fr.FIELDS[curve]
    rnd = random.Random("codec host fr " + curve)
    for v in [0, 1, f.p - 1] + [rnd.randrange(f.p) for _ in range(64)]:
        assert R.fr_encode(curve, v) == TR.serialize_fr(curve, f.to_limbs(v)) and R.fr_decode(curve, R.fr_encode(curve, v)) == (v, 0)
        assert list(f.to_limbs(v)) == R.limbs_of(curve, v, "r")
    assert R.fr_decode(curve, f.p.to_bytes(32, "little")) == (None, 8)


def _int_g2(curve, limbs):
    q, n = FQ_MODULI[curve], R.NBYTES[curve] // 8
    if not np.asarray(limbs).any():
        return None
    r_inv = pow(pow(2, 64 * n, q), -1, q)
    c = [sum(int(v) << (64 * i) for i, v in enumerate(limbs[k * n:(k + 1) * n])) * r_inv % q for k in range(4)]
    return (c[0], c[1]), (c[2], c[3])


def _lib_decode(curve, blob):
    limbs, st = CD.g2_from_bytes(curve, blob)
    return _int_g2(curve, limbs), st


@pytest.mark.parametrize("curve", CURVES)
def test_g2_round_trips_through_the_library(curve):
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    f = _fr.FIELDS[curve]
    gen = VF.g2_generator(curve)
    G = _int_g2(curve, gen)
    assert R.g2_decode(curve, R.g2_encode(curve, G)) == (G, 0)             # the library's generator is a point of order r for the reference too
    rnd = random.Random("codec host g2 " + curve)
    seen = set()
    for i in range(10):
        k = 1 if i == 0 else rnd.randrange(1, f.p)
        limbs = VF.g2_mul(curve, f.to_limbs(k), gen)
        for sign in (1, -1):
            P = _int_g2(curve, limbs)
            if sign < 0:
                P = (P[0], ((-P[1][0]) % q, (-P[1][1]) % q))
            want = np.array(R.g2_limbs(curve, P), dtype=np.uint64)
            for encoding in ("compressed", "uncompressed"):
                blob = CD.g2_to_bytes(curve, want, encoding)
                assert blob == R.g2_encode(curve, P, encoding)
                got, st = CD.g2_from_bytes(curve, blob)
                assert st == 0 and np.array_equal(got, want)
            seen.add((R.g2_encode(curve, P)[-1] & 0x80, P[1][1] > (q - P[1][1]) % q))
    assert {s for s, _ in seen} == {0, 0x80} and all((s == 0x80) == big for s, big in seen)      # the flag follows c1
    assert R.f2_larger(q, (q - 1, 0)) and not R.f2_larger(q, (1, 0)) and R.f2_larger(q, (1, q - 1)) and not R.f2_larger(q, (q - 1, 1))
    # infinity
    for encoding, n in (("compressed", 2), ("uncompressed", 4)):
        inf = bytes(n * nb - 1) + b"\x40"
        assert CD.g2_to_bytes(curve, np.zeros(nb // 2, np.uint64), encoding) == inf == R.g2_encode(curve, None, encoding)
        assert _lib_decode(curve, inf) == (None, 0) == R.g2_decode(curve, inf)


def _twist_points_with_y_in_a_subfield(curve):
    """twist points (x, y) with rhs = x^3 + b' in Fq, so that y lies in Fq (rhs a residue) or in u Fq: for x = x0 + x1 u the u part of rhs
    is 3 x0^2 x1 - x1^3 + b'.c1, zero for x0 = sqrt((x1^3 - b'.c1) / (3 x1)).  -> ([points with y.c1 = 0], [points with y.c0 = 0])"""
    q, b = FQ_MODULI[curve], R.g2_b(curve)
    real, imag = [], []
    for x1 in range(1, 200):
        t = (x1 ** 3 - b[1]) * pow(3 * x1, -1, q) % q
        x0 = pow(t, (q + 1) // 4, q)
        if x0 * x0 % q != t:
            continue
        x = (x0, x1)
        rhs = R.f2_add(q, R.f2_mul(q, R.f2_mul(q, x, x), x), b)
        assert rhs[1] == 0
        y = R.f2_sqrt(q, rhs)
        assert y is not None and R.f2_mul(q, y, y) == rhs and (y[0] == 0) != (y[1] == 0)
        (real if y[1] == 0 else imag).append((x, y))
        if len(real) >= 2 and len(imag) >= 2:
            break
    return real[:2], imag[:2]


@pytest.mark.parametrize("curve", CURVES)
def test_g2_tie_break_and_roots_in_a_subfield(curve):
    """y.c1 = 0: the flag is decided by c0; y.c0 = 0: by c1 alone.  plonk_g2_to_bytes takes any point of the twist, so these points (which are
    outside the subgroup) encode; decoding them finds the root through the c1 = 0 branch of the Fq2 square root and reports status 2, where a
    wrong root or a missed one would report 1."""
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    real, imag = _twist_points_with_y_in_a_subfield(curve)
    assert len(real) == 2 and len(imag) == 2
    flags = {"real": set(), "imag": set()}
    for kind, pts in (("real", real), ("imag", imag)):
        for x, y in pts:
            for P in ((x, y), (x, ((-y[0]) % q, (-y[1]) % q))):
                limbs = np.array(R.g2_limbs(curve, P), dtype=np.uint64)
                comp = CD.g2_to_bytes(curve, limbs, "compressed")
                assert comp == R.g2_encode(curve, P, "compressed")
                unc = CD.g2_to_bytes(curve, limbs, "uncompressed")
                assert unc == R.g2_encode(curve, P, "uncompressed")
                c = P[1][0] if kind == "real" else P[1][1]
                assert bool(comp[-1] & 0x80) == (c > q - c)                      # the flag follows the one non-zero coefficient
                flags[kind].add(comp[-1] & 0x80)
                for blob in (comp, unc):
                    assert R.g2_decode(curve, blob) == (None, 2)
                    got, st = CD.g2_from_bytes(curve, blob)
                    assert st == 2 and not got.any()
    assert flags == {"real": {0, 0x80}, "imag": {0, 0x80}}                       # both outcomes of the tie-break, both of c1 alone


@pytest.mark.parametrize("curve", CURVES)
def test_g2_bad_encodings_have_the_reference_status(curve):
    q, nb = FQ_MODULI[curve], R.NBYTES[curve]
    le = lambda v: v.to_bytes(nb, "little")
    G = _int_g2(curve, VF.g2_generator(curve))
    good = R.g2_encode(curve, G)
    # small x: some have no point (1), the others a twist point outside the subgroup (2), with both signs
    sts = []
    for x0 in range(12):
        for flag in (0, 0x80):
            blob = le(x0) + le(1)[:-1] + bytes([flag])
            ref = R.g2_decode(curve, blob)
            assert _lib_decode(curve, blob) == ref
            sts.append(ref[1])
            if ref[1] == 2:                            # that point, uncompressed: still outside the subgroup; its y + 1: off the twist
                y = R.f2_sqrt(q, R.f2_add(q, R.f2_mul(q, R.f2_mul(q, (x0, 1), (x0, 1)), (x0, 1)), R.g2_b(curve)))
                pair = le(x0) + le(1) + le(y[0]) + le(y[1])
                assert _lib_decode(curve, pair) == R.g2_decode(curve, pair) == (None, 2)
                off = le(x0) + le(1) + le((y[0] + 1) % q) + le(y[1])
                assert _lib_decode(curve, off) == R.g2_decode(curve, off) == (None, 1)
    assert 1 in sts and 2 in sts and 0 not in sts
    # x in Fq
    for x0 in range(6):
        blob = le(x0) + le(0)
        assert _lib_decode(curve, blob) == R.g2_decode(curve, blob)
    bad = [le(q) + good[nb:], good[:nb] + le(q), good[:-1] + bytes([good[-1] | 0xC0]), good[:-1] + bytes([(good[-1] & 0x3F) | 0x40]),
           le(1) + bytes(nb - 1) + b"\x40", bytes(2 * nb - 1) + b"\xC0",
           R.g2_encode(curve, G, "uncompressed")[:-1] + bytes([R.g2_encode(curve, G, "uncompressed")[-1] | 0x80]),
           le(G[0][0]) + le(G[0][1]) + le(q) + le(G[1][1]), bytes(3 * nb) + le(1)[:-1] + b"\x40"]
    for blob in bad:
        assert _lib_decode(curve, blob) == R.g2_decode(curve, blob) == (None, 8)
    lib = CD._ffi.lib()
    out = np.zeros(nb // 2, np.uint64)
    assert lib.plonk_g2_from_bytes(CD._ffi.CURVES[curve], good, 2, out.ctypes.data, None) == -1
    assert lib.plonk_g2_to_bytes(CD._ffi.CURVES[curve], None, 0, None) == -1 and lib.plonk_g2_to_bytes(7, out.ctypes.data, 0, bytes(8 * nb)) == -1
    with pytest.raises(ValueError):
        CD.g2_from_bytes(curve, good[:-1])
    with pytest.raises(CD._ffi.PlonkError):                                # not on the twist
        CD.g2_to_bytes(curve, np.arange(1, nb // 2 + 1, dtype=np.uint64))


@pytest.mark.parametrize("curve", CURVES)
def test_open_key_from_bytes(curve):
    tau = 0x1234567 + len(curve)
    ref = VF.OpenKey.from_trapdoor(curve, tau)
    g = TR.serialize_g1(curve, ref.g, False)
    for encoding in ("compressed", "uncompressed"):
        key = VF.OpenKey.from_bytes(curve, CD.g1_encode_host(curve, ref.g, encoding), CD.g2_to_bytes(curve, ref.h, encoding),
                                    CD.g2_to_bytes(curve, ref.beta_h, encoding))
        assert np.array_equal(key.g, ref.g) and np.array_equal(key.h, ref.h) and np.array_equal(key.beta_h, ref.beta_h)
    h, bh = CD.g2_to_bytes(curve, ref.h), CD.g2_to_bytes(curve, ref.beta_h)
    nb = R.NBYTES[curve]
    with pytest.raises(ValueError, match="generator"):
        VF.OpenKey.from_bytes(curve, g[:-1] + bytes([g[-1] ^ 0x80]), h, bh)
    with pytest.raises(ValueError, match="beta_h"):
        VF.OpenKey.from_bytes(curve, g, h, (3).to_bytes(nb, "little") + (1).to_bytes(nb, "little"))
    with pytest.raises(ValueError, match="h"):
        VF.OpenKey.from_bytes(curve, g, bytes(2 * nb - 1) + b"\x40", bh)       # infinity decodes, and is no key


@pytest.mark.parametrize("curve", CURVES)
def test_argument_errors_before_any_device_work(curve):
    w = types.SimpleNamespace(curve_name=curve, q64=R.NBYTES[curve] // 8)      # no context: every call below fails before it needs one
    assert CD.proof_nbytes(curve) == {"bn254": 768, "bls12_381": 976}[curve]
    for blob in (b"", bytes(CD.proof_nbytes(curve) - 1), bytes(CD.proof_nbytes(curve) + 1)):
        with pytest.raises(ValueError, match="bytes"):
            CD.proof_from_bytes(w, blob)
    with pytest.raises(ValueError):
        CD.g1_from_bytes(w, bytes(R.NBYTES[curve] - 1))
    with pytest.raises(ValueError):
        CD.fr_from_bytes(w, bytes(31))
    with pytest.raises(ValueError):
        CD.commitments_from_bytes(w, bytes(7))
    with pytest.raises(ValueError):
        CD.commitments_from_bytes(w, (2).to_bytes(8, "little") + bytes(R.NBYTES[curve]))
    with pytest.raises(KeyError):
        CD.g1_nbytes(curve, "packed")
    assert "non-canonical" in CD.status_text(8) and "r-subgroup" in CD.status_text(10) and "Vec" in CD.status_text(16)
