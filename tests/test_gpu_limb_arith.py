"""The limb arithmetic and curve formulas of the hot path as gfx950 code, against Python integers.

csrc/fp29.hpp (Fr in 9 x 29-bit limbs: Shoup and Montgomery multipliers, canonicalisation up to 48p), csrc/flimb.hpp (Fq in 9 x 29 or
14 x 28 limbs: product, square, dot2, lifted subtraction constants, standard-form conversion) and csrc/ec_lazy.hpp (lazy XYZZ madd_fast
with and without the fused Y3, complete madd and add, add_fast, dbl, dbl_affine, neg) are what msm_accumulate_kernel and ntt_pass_kernel
run.  test_fp29_host.py and test_ec_lazy_host.py check them as g++ output; for the device the same source takes another compiler and
another path (the accumulator pins exist only there, the column sums become v_mad_u64_u32 chains only there), and the parity tests
feed canonical inputs, so how far the intermediate values climb is decided by the kernels.  Here tests/device_cpp/limb_dev.hip wraps
the very functions in one kernel per operation and the vectors of tests/limb_vectors.py — the host tests' own, operands at the top of
the stated ranges included — run through them: exact congruence mod p, normalised limbs, the bounds the headers state (< 3p Shoup,
< 2p Montgomery, BOUND for accumulators), equality for canonical outputs.  Every operation gets 4 133 random vectors per curve BEHIND its
edge vectors (64 edge pairs for the Fr multipliers and the Fq products, 151 edge values for the canonicalisation), and every result is
checked, the Montgomery multiplier's included.  Batches leave the last workgroup ragged (4133 = 64 * 64 + 37 lanes, 4197 = 65 * 64 + 37,
4284 = 66 * 64 + 60; 37 alone).

The limit: this pins the functions as hipcc compiles them STAND-ALONE for gfx950 with the library's flags.  It does not pin the instances
inlined into msm_accumulate_kernel or ntt_pass_kernel (other register pressure, other scheduling); those are covered from outside by
test_gpu_msm.py and test_gpu_ntt.py."""
import ctypes as C
import os
import sys

import pytest

import limb_vectors as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4133          # random vectors per operation and curve: 16 full workgroups of 256 and a ragged one of 37 lanes
EDGE_PAIRS = 64   # the edge grid that leads the operand lists of the Fr multipliers and of the Fq products
EDGE_CANON = 151  # the edge values that lead canon_lazy's list
SMALL = 37


@pytest.fixture(scope="module")
def lib():
    """liblimb_dev.so as `build()` left it.  A missing library is a failure, not a skip."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tests.device_cpp import build as limb_build
    assert os.path.exists(limb_build.OUT), f"{limb_build.OUT} is missing: build it with `{limb_build.COMMAND}` (or __graft_entry__.build())"
    return V.DeviceLib(C.CDLL(limb_build.OUT))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [EDGE_PAIRS + N, SMALL])
def test_shoup_multiplier_against_integers(lib, curve, n):
    V.check_shoup_multiplier_against_integers(lib, curve, n, mont_stride=1)          # every Montgomery product, not one in seven


@pytest.mark.parametrize("curve", [0, 1])
def test_canon_lazy_up_to_48p(lib, curve):
    V.check_canon_lazy_up_to_48p(lib, curve, EDGE_CANON + N)


@pytest.mark.parametrize("curve", [0, 1])
def test_limb_parameters(lib, curve):
    V.check_limb_parameters(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [EDGE_PAIRS + N, SMALL])
def test_field_products_up_to_the_lazy_bounds(lib, curve, n):
    V.check_field_products_up_to_the_lazy_bounds(lib, curve, n)           # the first 64 operand pairs are the edge grid


@pytest.mark.parametrize("curve", [0, 1])
def test_standard_form_round_trip(lib, curve):
    V.check_standard_form_round_trip(lib, curve, N)


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


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("op", range(8))
def test_random_curve_ops_in_batches(lib, curve, op):
    """every curve operation, one operand set per lane: what the sequential chains above cannot give the device — many lanes at once"""
    V.check_random_curve_ops_in_batches(lib, curve, op, N)
    V.check_random_curve_ops_in_batches(lib, curve, op, SMALL)
