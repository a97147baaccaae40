"""The sponge, stream and shared-key kernels (elgamal_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as
tests/test_hostemu_edwards.py does for the Edwards kernels: a selection of tests/test_gpu_elgamal.py — the three kernels at counts 1 and 3 on
both curves against the pure-Python reference, the three enqueued launches under alternating Rescue tables, count 0 and the argument errors —
and of tests/test_gpu_elgamal_circuit.py: the encryption gadget of three instances solved by the emulated solver against the sequential
big-integer solve.  Register use, scratch and performance stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("file,k", [("test_gpu_elgamal.py", "(test_sponge_matches or test_stream_there or test_dh_key_matches) and (count1 or count3)"),
                                    ("test_gpu_elgamal.py", "test_three_dh_key_launches"),
                                    ("test_gpu_elgamal.py", "test_count_zero_and_argument_errors"),
                                    ("test_gpu_elgamal_circuit.py", "test_gadget_circuits_solve and elgamal_L4 and bn254")])
def test_elgamal_kernels_under_emulation(emu_env, file, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", os.path.join("tests", file), "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
