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
    asserted, so that a change to the draw logic cannot silently empty a branch.
  * `--ops wire,...`: the five operations on the Rescue sponge and stream, ElGamal on device pointers, the sponge / stream / encryption
    gadgets, the byte codec under drawn offsets and strides (or a commit key loaded from bytes) and batches of serialized proofs with drawn
    defects, with round1 (a new commit key), msm, trim (which frees the shared-key buffer) and ntt between them; draw counts and branch
    counters asserted as for the curve slice, the branches that only BLS12-381 can take from that curve's own counters."""
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


WIRE_SEEDS = [3302, 3305, 3321, 3322]
WIRE_OPS = ("sponge_stream", "elgamal", "wire_gadgets", "codec", "proof_bytes")
WIRE_BRANCHES = (["sponge." + x for x in ("L%3==0", "L%3!=0", "n_out.1", "n_out.2", "n_out.3")]
                 + ["stream." + x for x in ("encrypt", "decrypt", "in place", "straddles a workgroup")]
                 + ["rescue table switched between enqueued launches"]
                 + ["elgamal.params." + x for x in ("default", "generator", "scaled")]
                 + ["elgamal.defect." + x for x in ("none", "small order", "outside subgroup", "off curve")]
                 + ["elgamal." + x for x in ("ct shifted", "in place", "r>=l refused", "key buffer grown between enqueued launches")]
                 + ["wire_gadget." + x for x in ("sponge", "stream", "elgamal_circuit", "spoil.message", "spoil.r", "spoil.ct", "spoil.E")]
                 + ["codec.g1." + x for x in ("compressed", "uncompressed")]
                 + ["codec.subgroup." + x for x in ("checked", "unchecked")]
                 + ["codec.status stride." + x for x in ("0", "1", "2")]
                 + ["codec.odd input address", "codec.fr", "codec.srs from bytes.accepted", "codec.srs from bytes.refused"]
                 + ["codec.kind." + x for x in ("valid", "infinity", "random x", "x >= q", "both flags", "infinity with non-zero bytes", "sign bit on a pair",
                                                "off-curve pair")]
                 + ["proof_bytes.defect." + x for x in ("none", "flipped sign", "no point", "scalar >= r", "non-canonical infinity", "length prefix",
                                                        "two bad elements")]
                 + ["proof_bytes." + x for x in ("K.1", "K.>1", "all good", "mixed batch")])
WIRE_BRANCHES_BLS12_381 = ["codec.kind.outside subgroup", "proof_bytes.defect.outside subgroup"]       # BN254's cofactor is 1: its context never takes them
_wire_runs = {}


def wire_run(seed):
    """one run of the slice per seed and session -> (the finished process, its per-op counts, its branch counters, those of the BLS12-381 context)"""
    if seed not in _wire_runs:
        r = subprocess.run([sys.executable, "tools/fuzz_abi.py", "--seconds", "500", "--max-ops", "25", "--seed", str(seed), "--max-log", "10",
                            "--ops", "wire,trim,ntt,msm,round1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
        m = re.search(r"per op (\{.*?\}); branches (\{.*\})", r.stdout)
        bls = re.search(r"^branches on bls12_381 (\{.*\})$", r.stdout, re.M)
        _wire_runs[seed] = (r, ast.literal_eval(m.group(1)) if m else {}, ast.literal_eval(m.group(2)) if m else {}, ast.literal_eval(bls.group(1)) if bls else {})
    return _wire_runs[seed]


@pytest.mark.parametrize("seed", WIRE_SEEDS)
def test_wire_operations_fuzz_slice_on_the_device(seed):
    """25 operations per seed, the two curves in turn; most of the wall time is the Python references (capped per operation in the tool), the
    timeout is a hang guard.  Wall time per run on the MI355X, interpreter start included: 8.3 s
    (seed 3302), 7.7 s (3305), 8.7 s (3321), 6.8 s (3322).
    The draws and the branch counters depend on the seed alone; the seeds were chosen on the host emulation, where both are the same.  Over the
    four seeds every one of the five wire operations is drawn at least five times and every branch of WIRE_BRANCHES is taken — each sponge
    and stream form, the Rescue table switched and the key buffer replaced between enqueued launches, each spoiled E, each gadget and spoil,
    each encoding, status stride and element kind of the codec, a commit key from bytes accepted and refused, each defect of a serialized
    proof —, and the BLS12-381 context takes the two branches that need a cofactor (WIRE_BRANCHES_BLS12_381): asserted with the last seed
    over all four runs (a seed that has not run in this session yet runs then), from the counters the tool prints."""
    r, _, _, _ = wire_run(seed)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "fuzz ok: 25 operations" in r.stdout and "; branches {" in r.stdout, (r.stdout + r.stderr)[-3000:]
    if seed == WIRE_SEEDS[-1]:
        runs = [wire_run(x) for x in WIRE_SEEDS]
        drawn = {name: sum(per_op.get(name, 0) for _, per_op, _, _ in runs) for name in WIRE_OPS}
        taken = {name: sum(branches.get(name, 0) for _, _, branches, _ in runs) for name in WIRE_BRANCHES}
        taken.update({name + " (bls12_381)": sum(bls.get(name, 0) for _, _, _, bls in runs) for name in WIRE_BRANCHES_BLS12_381})
        print(drawn, taken)
        assert min(drawn.values()) >= 5, drawn
        assert min(taken.values()) >= 1, {k: v for k, v in taken.items() if not v}
