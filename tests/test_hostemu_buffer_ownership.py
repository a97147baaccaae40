"""tests/test_gpu_buffer_ownership.py EXECUTED on the CPU through the host emulation of tests/hostemu, all of it: the ownership of device
buffers is the Python layer's, and every path of it is the same where no GPU exists."""
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


# the groups partition the table: every id holds exactly one of these words
@pytest.mark.parametrize("k", ["codec or rescue", "edwards or elgamal", "circuit or BuiltCircuit or synthetic", "verifier"])
def test_buffer_ownership_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", "tests/test_gpu_buffer_ownership.py", "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout and "deselected" in r.stdout, tail
