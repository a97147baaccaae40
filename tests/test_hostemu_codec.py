"""The codec kernels (codec_kernels.hpp) EXECUTED on the CPU through the host emulation of tests/hostemu, as tests/test_hostemu_elgamal.py
does for the sponge and stream kernels: a selection of tests/test_gpu_codec.py — the round trips at counts 1 and 3 in both forms on both
curves, the named values, the scalars, the strided decode with its shared status word, count 0 and the argument errors, a batch of three
proofs with each bad element in turn, and an SRS loaded from bytes in both encodings with point 517 spoiled — against the pure-Python
reference.  Register use, scratch and performance stay with `pytest -m gpu` on an MI355X."""
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


@pytest.mark.parametrize("k", ["test_round_trip_of_srs_points and (count1 or count3)",
                               "test_named_values or test_fr_values or test_infinity_round_trip",
                               "test_strides_gaps and bn254 or test_count_zero_and_argument_errors",
                               "test_proofs_from_bytes and K3",
                               "test_init_bytes_commits_like_init"])
def test_codec_kernels_under_emulation(emu_env, k):
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_codec.py"), "-k", k]
    r = subprocess.run(cmd, cwd=ROOT, env=emu_env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail
