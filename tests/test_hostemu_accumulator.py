"""The accumulator kernels (rescue_acc_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_rescue.py does for the permutation: a selection of tests/test_gpu_accumulator.py — the trees (1, 2), (3, 10), (5, 65) and
(32, 4) at every node on both curves, the paths and the solver-input layout, the input scatter, the argument errors, and a solve from device
inputs against the same solve from host inputs.  Register use, scratch and performance stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_tree_matches and (h1c2 or h3c10 or h5c65 or h32c4)",
                               "test_paths_and_solver_inputs",
                               "test_scatter or test_argument_errors",
                               "test_solving_from_device_inputs"])
def test_accumulator_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_accumulator.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
