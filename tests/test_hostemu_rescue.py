"""The Rescue kernels (rescue_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as tests/test_hostemu_hints.py
does for the hint kernels: a selection of tests/test_gpu_rescue.py — plonk_rescue_permute_dev at counts 1, 3 and 65 on both curves and the
fixtures' edge states against the pure-Python reference, a tree of 8 leaves at every node (and the trees of 1 and 2 leaves), the level
kernel against the permutation kernel, count 0, and the argument errors.  Register use, scratch and performance stay with `pytest -m gpu`
on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_permutation_matches and (count1 or count3 or count65)",
                               "test_fixture_edge_states or test_count_zero or test_injected_parameters",
                               "test_merkle_tree_matches and (log0 or log1 or log3)",
                               "test_level_kernel or test_argument_errors"])
def test_rescue_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_rescue.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
