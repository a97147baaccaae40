"""The hint kernels of the witness solver (solve_hints.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_solve.py does for the hint-free solver: a selection of tests/test_gpu_hints.py — random layered circuits with every
hinted operation on both curves against the big-integer reference, the frontier shapes of the per-class lists, BIT at its edge arguments,
cycles and validation errors, hint_op = NULL, determinism, and the hinted circuit built, solved, proved and verified at 2^8 gates —
bit-for-bit where no GPU exists.  Performance, register use and the memory model stay with `pytest -m gpu` on an MI355X."""
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
                               "test_frontier or test_bit_at",
                               "test_a_cycle or test_invalid_hints or test_null_hint_op or test_two_runs",
                               "test_hinted_circuit and log8"])
def test_hint_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_hints.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
