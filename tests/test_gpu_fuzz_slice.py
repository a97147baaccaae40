"""Fixed-seed slices of the differential ABI fuzzer (tools/fuzz_abi.py) against the REAL library on an MI355X, every result compared with a
CPU reference bit for bit.  The oracle and the pure-Python references are the checkers; the product path is the C ABI.

  * `--ops core`: 300 random operations of the nineteen kinds of the MSM / NTT / prover side (single kernels, plonk_trim between operations,
    the gate-range grand product, the residue-class iFFT, refused SRSs, distributed transforms, batched commitments, fixed-base tables, whole
    proofs handed to the verifier) with random shapes, flags and options.  Round 3 could only run the fuzzer against the host emulation
    (tests/test_hostemu.py); its first run on the device (round 4: 1651 operations in 100 s, no mismatch — profiles/
    r04_opening_measurements.txt) is pinned here as a test.
  * `--ops circuit,...`: the six operations on circuits, witnesses, Rescue trees and the verifier (circuit preprocessing, the level-by-level
    solver and its hinted variant, the Rescue permutation and Merkle kernels, the ternary accumulator and its path gather, the batched
    verifier, the whole membership chain) in arbitrary order on one long-lived context, with round1 (a new commit key), msm (workspace
    growth, forced windows), trim (the scratch dropped), ntt and poly drawn between them."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_differential_fuzz_slice_on_the_device():
    r = subprocess.run([sys.executable, "tools/fuzz_abi.py", "--seconds", "240", "--max-ops", "300", "--seed", "2026", "--max-log", "13", "--ops", "core"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fuzz ok: 300 operations" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("seed", [3101, 3102, 3103, 3104])
def test_circuit_operations_fuzz_slice_on_the_device(seed):
    """25 operations per seed, the two curves in turn.  Most of the wall time is the Python references (capped per operation in the tool),
    the device's share is a few seconds; the timeout is a hang guard.  Wall time per run on the MI355X, interpreter start included: 9.7 s
    (seed 3101), 7.1 s (3102), 8.2 s (3103), 11.0 s (3104); every one of the six circuit operations is drawn at least six times over the four."""
    r = subprocess.run([sys.executable, "tools/fuzz_abi.py", "--seconds", "500", "--max-ops", "25", "--seed", str(seed), "--max-log", "10",
                        "--ops", "circuit,trim,ntt,msm,poly,round1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "fuzz ok: 25 operations" in r.stdout, (r.stdout + r.stderr)[-3000:]
