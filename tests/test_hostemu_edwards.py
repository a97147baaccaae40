"""The Edwards kernels (edwards_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as tests/test_hostemu_rescue.py
does for the Rescue kernels: a selection of tests/test_gpu_edwards.py — the four kernels at counts 1 and 3 on both curves against the
pure-Python reference, fixed_mul against mul with G (which builds the generator's table), the injected generator, count 0 and the argument
errors, sign then verify, the four kernels on a scaled curve at count 3, mul and add over an input, the table rebuilt between three enqueued
fixed_mul launches, fixed_mul after plonk_trim and after a round under a new commit key — and of tests/test_gpu_edwards_circuit.py: the signature circuit of three signatures solved by the emulated solver
against the sequential big-integer solve.  Register use, scratch and performance stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("file,k", [("test_gpu_edwards.py", "(test_mul_matches or test_fixed_mul_matches or test_add_matches or test_check_flags) and (count1 or count3)"),
                                    ("test_gpu_edwards.py", "test_injected_generator or test_count_zero_and_argument_errors"),
                                    ("test_gpu_edwards.py", "test_sign_then_verify"),
                                    ("test_gpu_edwards.py", "(test_the_four_kernels_on_a_scaled_curve and count3) or test_mul_over_its_points or test_three_fixed_mul_launches"
                                                            " or test_fixed_mul_after_trim"),
                                    ("test_gpu_edwards_circuit.py", "test_gadget_circuits_solve and schnorr and bn254")])
def test_edwards_kernels_under_emulation(emu_env, file, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", os.path.join("tests", file), "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
