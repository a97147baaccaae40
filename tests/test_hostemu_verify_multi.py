"""The multi-key verifier kernels and the sum tree (verify_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_verify.py does for the one-key kernels: a selection of tests/test_gpu_batch_verify_multi.py — a mixed batch of 65 against
the reference on BN254, the verdicts on BLS12-381, the sum tree at 65 and 129 leaves, the status words with their far-away offsets (a read
through a bad span would leave the emulation's address space), the argument errors — bit for bit where no GPU exists.  Divergence cost and
register pressure stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_mixed_batch_matches_the_reference and bn254 and 65",
                               "test_honest_proofs_of_both_circuits_in_one_pairing and bls12_381",
                               "test_a_wrong_proof_is_rejected_alone and bls12_381 and (other_circuit or evaluation)",
                               "test_one_key_equals_the_single_key_entry_point and bn254",
                               "test_sum_tree_equals_the_integer_sums and bn254 and 65",
                               "test_sum_tree_equals_the_integer_sums and bls12_381 and 129",
                               "test_sum_tree_of_nothing_writes_nothing",
                               "test_bad_index_and_bad_span_are_verdicts_that_read_nothing",
                               "test_argument_errors_name_the_key and bn254"])
def test_multi_key_verifier_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_batch_verify_multi.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
