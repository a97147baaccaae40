"""The device harness of the limb arithmetic (tests/device_cpp/limb_dev.hip) on the emulated HIP runtime — no GPU.  The arithmetic itself
is checked where no GPU exists by test_fp29_host.py and test_ec_lazy_host.py; what runs here is the HARNESS that test_gpu_limb_arith.py
relies on: kernel indexing over more than one workgroup, the tail guard of a ragged last workgroup, the flag plumbing of the fast paths,
the buffer layouts of every entry point — the exceptional cases plus 1 003 random vectors per operation and curve behind the edge
vectors, every result checked (and one batch of fewer than 64)."""
import ctypes as C
import os
import sys

import pytest

import limb_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1003          # random vectors per operation: 3 full workgroups of 256 and a ragged one of 235 lanes (not a multiple of 64)
EDGE_PAIRS = 64   # the edge grid that leads the operand lists of the Fr multipliers and of the Fq products
EDGE_CANON = 151  # the edge values that lead canon_lazy's list
SMALL = 37


@pytest.fixture(scope="module")
def lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tests.device_cpp import build as limb_build
    return V.DeviceLib(C.CDLL(limb_build.build_emu(verbose=False)))


@pytest.mark.parametrize("curve", [0, 1])
def test_exceptional_cases(lib, curve):
    V.check_exceptional_cases(lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_fr_multipliers_and_canonicalisation(lib, curve):
    V.check_shoup_multiplier_against_integers(lib, curve, EDGE_PAIRS + N, mont_stride=1)       # 1 067 = 16 * 64 + 43 lanes
    V.check_shoup_multiplier_against_integers(lib, curve, SMALL, mont_stride=1)
    V.check_canon_lazy_up_to_48p(lib, curve, EDGE_CANON + N)                                   # 1 154 = 18 * 64 + 2 lanes


@pytest.mark.parametrize("curve", [0, 1])
def test_fq_parameters_products_and_standard_form(lib, curve):
    V.check_limb_parameters(lib, curve)
    V.check_field_products_up_to_the_lazy_bounds(lib, curve, EDGE_PAIRS + N)
    V.check_field_products_up_to_the_lazy_bounds(lib, curve, SMALL)
    V.check_standard_form_round_trip(lib, curve, N)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("op", range(8))
def test_random_curve_ops_in_batches(lib, curve, op):
    V.check_random_curve_ops_in_batches(lib, curve, op, N)
    V.check_random_curve_ops_in_batches(lib, curve, op, SMALL)


def test_a_bad_device_ordinal_is_a_status_not_a_crash(lib):
    out = (C.c_uint32 * 9)()
    assert lib.lib.get_pbar(99, 0, out) != 0
