"""The batched verifier's kernels (verify_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu.py does for the rest of the library: a selection of tests/test_gpu_batch_verify.py — device challenges, PI(zeta),
r(zeta), E and the points against oracle/verifier_ref.py, honest proofs accepted, bisection, malformed input — and of
tests/test_gpu_batch_verify_edges.py — the degenerate and coinciding points of the sweep, a batch of 65, the status words — and the one-key
route from bytes of tests/test_gpu_codec_verify.py, bit-for-bit where no GPU exists.  Performance, LDS capacity and register pressure stay with `pytest -m gpu` on an MI355X."""
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


FILES = ["tests/test_gpu_batch_verify.py", "tests/test_gpu_batch_verify_edges.py",
         "tests/test_gpu_codec_verify.py"]                                             # the test names below are unique across the three


@pytest.mark.parametrize("k", ["test_device_challenges_scalars_and_points_match_the_reference and bn254",
                               "test_batch_verify_bisects_to_the_bad_proofs and bls12_381",
                               "test_malformed_input_gives_a_status",
                               "test_sweep_matches_the_integer_statement and degenerate and bn254",
                               "test_sweep_matches_the_integer_statement and coincide and bls12_381",
                               "test_batch_shapes and bls12_381 and 65",
                               "test_status_words and bls12_381",
                               "test_batch_verify_bytes and bn254"])
def test_batch_verify_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", *FILES, "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
