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
    growth, forced windows), trim (the scratch dropped), ntt and poly drawn between them.
  * `--ops curve,...`: the four operations on the embedded Edwards curve, Schnorr signatures, the builder's point gadgets and the solve-schedule
    replay, with round1 (a new commit key), msm, trim and ntt between them; the draw counts and the branch counters that the tool prints are
    asserted, so that a change to the draw logic cannot silently empty a branch."""
import ast
import os
import re
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


CURVE_SEEDS = [3212, 3228, 3233, 3237]
CURVE_BRANCHES = (["edwards.kernel." + x for x in ("mul", "fixed_mul", "add", "check")]
                  + ["edwards.params." + x for x in ("default", "generator", "scaled")]
                  + ["edwards.alias." + x for x in ("none", "out=points", "out=p", "out=q")]
                  + ["edwards.table rebuilt without sync"]
                  + ["schnorr.defect." + x for x in ("none", "s+1", "s+l", "message", "pk", "R off curve", "pk off curve", "pk outside subgroup")]
                  + ["gadget." + x for x in ("point_add", "point_double", "point_neg", "point_select", "enforce_on_curve", "scalar_mul", "fixed_base_mul",
                                             "spoil.off curve", "spoil.select bit")]
                  + ["replay." + x for x in ("wide", "fused", "fused run starting at class != 0", "segment == fuse_width", "cycle")])
_curve_runs = {}


def curve_run(seed):
    """one run of the slice per seed and session -> (the finished process, its per-op counts, its branch counters)"""
    if seed not in _curve_runs:
        r = subprocess.run([sys.executable, "tools/fuzz_abi.py", "--seconds", "500", "--max-ops", "25", "--seed", str(seed), "--max-log", "10",
                            "--ops", "curve,trim,ntt,msm,round1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
        m = re.search(r"per op (\{.*?\}); branches (\{.*\})", r.stdout)
        _curve_runs[seed] = (r, ast.literal_eval(m.group(1)) if m else {}, ast.literal_eval(m.group(2)) if m else {})
    return _curve_runs[seed]


@pytest.mark.parametrize("seed", CURVE_SEEDS)
def test_curve_operations_fuzz_slice_on_the_device(seed):
    """25 operations per seed, the two curves in turn; most of the wall time is the Python references (capped per operation in the tool), the
    timeout is a hang guard.  Wall time per run on the MI355X, interpreter start included: 4.4 s
    (seed 3212), 4.5 s (3228), 4.3 s (3233), 4.4 s (3237).
    The draws and the branch counters depend on the seed alone.  Over the four seeds every one of the four curve operations is drawn at
    least five times and every branch of CURVE_BRANCHES is taken — each kernel, parameter set and aliasing, the table rebuilt between
    enqueued launches, each Schnorr defect, each gadget and spoiled input, the replay's launch forms and the planted cycle: asserted with the
    last seed over all four runs (a seed that has not run in this session yet runs then), from the counters the tool prints."""
    r, _, _ = curve_run(seed)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fuzz ok: 25 operations" in r.stdout and "; branches {" in r.stdout, (r.stdout + r.stderr)[-3000:]
    if seed == CURVE_SEEDS[-1]:
        runs = [curve_run(x) for x in CURVE_SEEDS]
        drawn = {name: sum(per_op.get(name, 0) for _, per_op, _ in runs) for name in ("edwards", "schnorr", "edwards_gadgets", "replay")}
        taken = {name: sum(branches.get(name, 0) for _, _, branches in runs) for name in CURVE_BRANCHES}
        print(drawn, taken)
        assert min(drawn.values()) >= 5, drawn
        assert min(taken.values()) >= 1, {k: v for k, v in taken.items() if not v}
