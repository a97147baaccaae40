"""The 9 x 29-bit limb arithmetic of csrc/fp29.hpp compiled for the HOST (its functions are __host__ __device__) against Python
integers — no GPU: the precomputed-quotient ("Shoup") constant multiplier the NTT butterflies use on BN254, its constant
preparation, the Montgomery multiplier on the same operands, and the product-free canonicalisation up to the bound the Shoup
butterflies reach (< 48p).  Operand ranges are the ones a butterfly produces: un-normalised limbs < 2^31, value < 2^259.4.
The vectors and the assertions live in tests/limb_vectors.py, which the device build of the same headers shares (test_gpu_limb_arith.py)."""
import ctypes as C
import os
import subprocess

import pytest

import limb_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fp29") / "fp29_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_cpp", "fp29_host.cpp"), "-o", so])
    return V.HostLibs(fp29=C.CDLL(so))


@pytest.mark.parametrize("curve", [0, 1])
def test_shoup_multiplier_against_integers(lib, curve):
    V.check_shoup_multiplier_against_integers(lib, curve, 40000)


@pytest.mark.parametrize("curve", [0, 1])
def test_canon_lazy_up_to_48p(lib, curve):
    V.check_canon_lazy_up_to_48p(lib, curve, 60000)
