"""The witness solver's kernels (solve_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_verify.py does for the verifier: a selection of tests/test_gpu_solve.py — random layered circuits on both curves
against the big-integer reference, the scheduling shapes (the emulation is quick enough for the 2^12-level chain and the 2^20
independent gates at full size), cycles and validation errors, determinism, and the membership circuit built, solved, proved and
verified at 2^8 gates — bit-for-bit where no GPU exists.  Performance and the memory model stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_random_layered and (log3 or log5 or log8 or log12)",
                               "test_chain_takes or test_independent or test_definitions_after or test_one_variable_on_two",
                               "test_a_cycle or test_invalid_definitions or test_two_runs",
                               "test_membership and log8"])
def test_solve_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_solve.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
