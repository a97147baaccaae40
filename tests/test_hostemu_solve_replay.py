"""The schedule recorder and the replay kernels (solve_replay.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_solve.py does for the solver: a selection of tests/test_gpu_solve_replay.py — the recorded order against the
reference's levels on both curves, replayed witnesses against solve_dev limb for limb for every fuse width and for K = 1, one Rescue hash
and a chain of two (a fused run of 75 levels with a barrier per level, which the emulation runs as fibers), the wide segment of 3000
gates, a dependency cycle, and device inputs.  The memory model of the fused form stays with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_schedule_matches or test_two_recordings or test_a_cycle",
                               "test_replay_equals_solve",
                               "test_replay_of_one_rescue or test_replay_fuses or test_replay_of_a_segment",
                               "test_device_inputs"])
def test_replay_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_solve_replay.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
