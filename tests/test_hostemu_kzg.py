"""The KZG kernels (csrc/kzg_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as tests/test_hostemu_verify.py does
for the batch verifier: a selection of tests/test_gpu_kzg_open.py — every length up to 2 T + 1 on both curves, 65 points, values only, bad
arguments, the proofs of open_many —, of tests/test_gpu_kzg_verify.py — one defect sweep at K = 8, the pairs against the integers, the
status words, the edge cases — and of tests/test_gpu_kzg_ownership.py, bit for bit where no GPU exists.  The length that gives the top
scan two tiles per lane, performance, LDS capacity and register pressure stay with `pytest -m gpu` on an MI355X."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_env():
    sys.path.insert(0, ROOT)
    from tests.hostemu import build as emu_build
    lib = emu_build.build(verbose=False)
    env = dict(os.environ)
    env.update(PLONK_HIP_LIB=lib, PLONK_ALLOW_HOSTEMU="1", HIPEMU_DEVICES="1", HIPEMU_THREADS=str(min(8, os.cpu_count() or 1)))
    return env


FILES = ["tests/test_gpu_kzg_open.py", "tests/test_gpu_kzg_verify.py", "tests/test_gpu_kzg_ownership.py"]     # the test names below are unique across the three


@pytest.mark.parametrize("k", ["test_values_and_quotient_rows_match_the_reference and not 5Tp7",
                               "test_point_counts_across_the_table_kernels_workgroup_seam and 65",
                               "test_values_only_mode_equals_the_full_mode or test_bad_arguments",
                               "test_open_many_proofs_are_the_trapdoor_expression or test_reference_points_are_the_oracles_commitments",
                               "test_defects_are_found_where_they_are and 8 and y_plus_1 and bn254",
                               "test_pairs_against_the_integers",
                               "test_status_words",
                               "test_edge_cases and bls12_381",
                               "test_kzg_functions_leave_no_buffer_behind and open_many and bn254"])
def test_kzg_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", *FILES, "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
