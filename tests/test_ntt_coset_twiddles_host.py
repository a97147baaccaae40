"""The folded first pass's butterfly chain (csrc/ntt_kernels.hpp: ntt_butterflies with coset twiddles) compiled for the HOST and driven over
one 512-row column exactly as ntt_pass_kernel<9, 4, true, true, true> drives it — nine stages, every one with a prepared-constant product —
against Python integers, no GPU.  The twiddle table is built HERE from integers (s^(R / 2^(sigma+1)) * w_(2^(sigma+1))^j at index 2^sigma - 1 + j),
so the identity F_R(x; s)[k] = sum_a x[a] s^a w^(ak) is checked independently of the engine's table builder.

Inputs sit at the entry bounds of the CONTRACT in ntt_kernels.hpp: all p - 1 (raw canonical coefficients), the fold sum's bound 10.6p with the
largest normalised limbs below it, a column of random values below 10.6p, and a column that is zero but for three rows.  After every step the
column must be normalised (limbs 0..7 < 2^29, top limb < 2^29), its values below E + 4p * (stages done) — 46.6p < 2^261 after nine — and the
un-normalised result of the next add / sub (at most limb + 4p's lifted limb) below 2^31, the multiplier's operand range."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, LOG_R = 512, 9
MASK = (1 << 29) - 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ctw") / "ntt_coset_twiddles_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tests", "hostemu"), "-include", "hip/hip_runtime.h",
                           "-Wno-unknown-pragmas", "-Wno-attributes", os.path.join(ROOT, "tests", "host_cpp", "ntt_coset_twiddles_host.cpp"), "-o", so])
    return C.CDLL(so)


def limbs(v):
    """normalised 9 x 29-bit limbs, the excess in the top limb"""
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def brev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2)


@pytest.mark.parametrize("curve", [0, 1])
def test_nine_all_product_stages_from_the_entry_bounds(lib, curve):
    from oracle import prover_ref as P
    f = P.CURVE_OBJ[curve].fr
    p = f.p
    rng = random.Random(9100 + curve)
    w = f.root_of_unity(R)
    s = rng.randrange(2, p)
    tab = []
    for sg in range(LOG_R):
        sp, wr = pow(s, R >> (sg + 1), p), pow(w, R >> (sg + 1), p)
        for j in range(1 << sg):
            c = sp * pow(wr, j, p) % p
            cq = (c << 261) // p
            tab += limbs(c) + [(cq >> (29 * i)) & MASK for i in range(9)]
    assert len(tab) == 18 * (R - 1)
    tab = np.array(tab, dtype=np.uint32)
    c4p = np.zeros(9, dtype=np.uint32)
    lib.get_c4p(curve, c4p.ctypes.data_as(C.c_void_p))
    fold = (106 * p) // 10                                    # the fold sum stays below p + 7 * 1.36p < 10.6p
    worst = (((fold >> 232) - 1) << 232) | ((1 << 232) - 1)   # the largest value below it whose low limbs are all 2^29 - 1
    assert worst < fold and limbs(worst)[:8] == [MASK] * 8
    sparse = [0] * R
    sparse[0], sparse[257], sparse[511] = p - 1, worst, 1
    columns = {"p-1": ([p - 1] * R, p), "fold worst limbs": ([worst] * R, fold), "random below 10.6p": ([rng.randrange(fold) for _ in range(R)], fold),
               "zero rows": (sparse, fold)}
    spow = [pow(s, a, p) for a in range(R)]
    wpow = [pow(w, e, p) for e in range(R)]
    for name, (col, entry) in columns.items():
        x = np.array([limbs(v) for v in col], dtype=np.uint32)
        snaps = np.zeros((5, R, 9), dtype=np.uint32)
        lib.coset_chain(curve, x.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), snaps.ctypes.data_as(C.c_void_p))
        for i, done in enumerate((2, 4, 6, 8, 9)):
            snap = snaps[i]
            assert int(snap[:, :8].max()) < 1 << 29 and int(snap[:, 8].max()) < 1 << 29, (curve, name, done, "not normalised")
            assert int((snap.astype(np.uint64) + c4p).max()) < 1 << 31, (curve, name, done, "the next un-normalised add / sub leaves the operand range")
            top = max(value(row) for row in snap)
            assert top < entry + 4 * p * done, (curve, name, done, top / p)
            assert top < 1 << 261
        # stage by stage the column holds the partial transforms; after nine stages row k is the transform's output k
        xs = [v * sa % p for v, sa in zip(col, spow)]
        want = [sum(xa * wpow[a * k % R] for a, xa in enumerate(xs)) % p for k in range(R)]
        got = [value(row) % p for row in snaps[4]]
        assert got == want, (curve, name)
        # ... and after the first step (stages 0 and 1) row 4m + k is the 4-point transform of x[brev-ordered quadruple m] with scale s^(R/4)
        s4, w4 = pow(s, R // 4, p), pow(w, R // 4, p)
        for m in (0, 1, 77, 127):
            a = brev(m, LOG_R - 2)
            quad = [col[a + i * (R // 4)] for i in range(4)]
            for k in range(4):
                assert value(snaps[0][4 * m + k]) % p == sum(q * pow(s4, i, p) * pow(w4, i * k, p) for i, q in enumerate(quad)) % p, (curve, name, m, k)
