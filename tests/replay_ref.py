"""The solve schedule and the replay's launch plan restated from a reference solve (a helper of tests/test_gpu_solve_replay.py and of
tools/fuzz_abi.py, not a test): the level of def_gate[v] is lvl[v] of tests/hint_ref.py, the class comes from the opcode, ties break by gate;
the plan is read off seg and fuse_width by the rule that csrc/solve_replay.hpp states for circuit_replay_run."""
import numpy as np

from distributed_plonk_amd import builder as BD
from tests.hint_ref import GIVEN


def class_of(opcode: int) -> int:
    return 1 if opcode in (BD.HINT_INV, BD.HINT_DIV) else 2 if opcode == BD.HINT_ROOT5 else 0


def ref_schedule(built, ref):
    """-> (order, seg, levels, evaluations) from the reference's levels: gates sorted by (level, class, gate).  ref: a solved HintRefSolver"""
    keyed = sorted((3 * ref.lvl[v] + class_of(ref.opcode(int(g))), int(g)) for v, g in enumerate(built.def_gate) if g != GIVEN)
    levels = ref.depth()
    keys = np.array([k for k, _ in keyed], dtype=np.int64)
    seg = np.searchsorted(keys, np.arange(3 * levels + 1), side="left").astype(np.uint32)
    return np.array([g for _, g in keyed], dtype=np.uint32), seg, levels, len(keyed)


def replay_plan(seg, fuse_width: int) -> list:
    """The launches of one replay, in order: ("wide", s, s + 1) for a non-empty segment launched on its own, ("fused", s, end) for a maximal
    run of segments of at most fuse_width gates each that holds more than one non-empty segment.  seg: the 3 levels + 1 segment starts."""
    seg = [int(x) for x in seg]
    segments = len(seg) - 1
    length = lambda s: seg[s + 1] - seg[s]
    plan, s = [], 0
    while s < segments:
        end = s
        while fuse_width and end < segments and length(end) <= fuse_width:
            end += 1
        if sum(1 for t in range(s, end) if length(t)) > 1:
            plan.append(("fused", s, end))
            s = end
        else:
            for t in range(s, max(end, s + 1)):
                if length(t):
                    plan.append(("wide", t, t + 1))
            s = max(end, s + 1)
    return plan


def plan_branches(seg, fuse_width: int, K: int, threads: int = 256) -> set:
    """Which forms a replay of (seg, fuse_width, K) takes, as names: "wide", "fused", "fused run starting at class != 0", "fused run ending
    inside a level", "empty segment inside a fused run", "wide launch after a fused run of its level", "segment == fuse_width",
    "segment == fuse_width + 1", "wide launch of more than one workgroup", "wide launch of one workgroup"."""
    seg = [int(x) for x in seg]
    lens = [seg[s + 1] - seg[s] for s in range(len(seg) - 1)]
    out = set()
    plan = replay_plan(seg, fuse_width)
    for i, (form, s, end) in enumerate(plan):
        out.add(form)
        if form == "fused":
            if s % 3:
                out.add("fused run starting at class != 0")
            if end % 3:
                out.add("fused run ending inside a level")
            if any(lens[t] == 0 for t in range(s + 1, end - 1)):
                out.add("empty segment inside a fused run")
        else:
            out.add("wide launch of more than one workgroup" if lens[s] * K > threads else "wide launch of one workgroup")
            if i and plan[i - 1][0] == "fused" and (plan[i - 1][2] - 1) // 3 == s // 3:
                out.add("wide launch after a fused run of its level")
    if fuse_width and fuse_width in lens:
        out.add("segment == fuse_width")
    if fuse_width and fuse_width + 1 in lens:
        out.add("segment == fuse_width + 1")
    return out
