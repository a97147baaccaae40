"""The MSM's device arithmetic compiled for the HOST against Python integers — no GPU: the unsaturated-limb Montgomery field of
csrc/flimb.hpp (9 x 29-bit limbs on BN254 Fq, 14 x 28-bit on BLS12-381 Fq; product, square, the two-product `fl_dot2`, the lifted
subtraction constants) and the lazy XYZZ formulas of csrc/ec_lazy.hpp that `msm_accumulate_kernel`, its redo / heavy kernels and the
reduction pyramid run (mixed addition with and without the fused Y3, complete addition, doubling, the fast paths' same-x abort).
Every result is compared with affine integer arithmetic on the curve, and the invariants ec_lazy.hpp states (X < 5.2p, Y < 3.3p,
ZZ, ZZZ < 2p, normalised limbs) are checked after every operation — also when the operands are lifted to the TOP of those ranges,
which is what the column accumulators' 64-bit head-room was sized for.  The GPU parity tests (test_gpu_msm.py) cover the kernels
around this arithmetic; this file keeps the arithmetic itself under test where no GPU exists.
The vectors and the assertions live in tests/limb_vectors.py, which the device build of the same headers shares (test_gpu_limb_arith.py)."""
import ctypes as C
import os
import subprocess

import pytest

import limb_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ecl") / "ec_lazy_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "host_cpp", "ec_lazy_host.cpp"), "-o", so])
    return V.HostLibs(ecl=C.CDLL(so))


@pytest.mark.parametrize("curve", [0, 1])
def test_limb_parameters(lib, curve):
    V.check_limb_parameters(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_field_products_up_to_the_lazy_bounds(lib, curve):
    V.check_field_products_up_to_the_lazy_bounds(lib, curve, 4000)


@pytest.mark.parametrize("curve", [0, 1])
def test_standard_form_round_trip(lib, curve):
    V.check_standard_form_round_trip(lib, curve, 300)


@pytest.mark.parametrize("curve", [0, 1])
def test_bucket_accumulation_chain(lib, curve):
    V.check_bucket_accumulation_chain(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_exceptional_cases(lib, curve):
    V.check_exceptional_cases(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_operands_at_the_top_of_their_ranges(lib, curve):
    V.check_operands_at_the_top_of_their_ranges(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_reduction_pyramid_chunk(lib, curve):
    V.check_reduction_pyramid_chunk(lib, curve)
