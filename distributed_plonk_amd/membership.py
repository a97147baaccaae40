"""The circuit the reference's end-to-end test proves (generate_circuit, dispatcher2.rs:1226-1271), for any height and proof count: m
memberships in one ternary Rescue accumulator (rescue.Accumulator; the reference has TREE_HEIGHT = 32 and NUM_MEMBERSHIP_PROOFS = 50)
against its public root.

    built = membership_circuit("bn254", 32, 50)                     # n = 2^18
    acc = rescue.Accumulator(worker, rescue.RescueParams.default("bn254"), elems, 32)
    d_in = acc.witness_inputs_dev(range(50))                        # gathered on the device
    inst = built.preprocess(worker, d_inputs=d_in.ptr, public_inputs=acc.root.reshape(1, 4))

The inputs are created in the order in which plonk_rescue_acc_paths_dev writes its rows, each row m values: uid, elem, then per level
sib1_j, sib2_j, is_left_j, is_right_j — (2 + 4 height) x m, row-major."""
from __future__ import annotations

from .builder import BuiltCircuit, CircuitBuilder


def num_input_rows(height: int) -> int:
    return 2 + 4 * height


def membership_circuit(curve: str, height: int, m: int, params=None) -> BuiltCircuit:
    """One public root; m x (uid, elem, height x (sib1, sib2, is_left, is_right)) inputs; enforce_equal(accumulator_root(..), root) per
    membership."""
    from .rescue import MAX_HEIGHT
    if not 1 <= height <= MAX_HEIGHT:
        raise ValueError(f"height = {height}: 1 .. {MAX_HEIGHT}")
    if m < 1:
        raise ValueError(f"m = {m}: at least one membership")
    b = CircuitBuilder(curve)
    root = b.public_input()
    as_ids = lambda v: [v] if m == 1 else v               # input(1) gives a scalar id
    uid, elem = as_ids(b.input(m)), as_ids(b.input(m))
    sib1s, sib2s, is_lefts, is_rights = [], [], [], []
    for _ in range(height):
        for rows in (sib1s, sib2s, is_lefts, is_rights):
            rows.append(as_ids(b.input(m)))
    b.enforce_equal(b.accumulator_root(uid, elem, sib1s, sib2s, is_lefts, is_rights, params), root)
    return b.build()
