"""Host-side refusals of the replay path: plonk_circuit_replay_dev checks its arguments before it touches the context, and
BuiltCircuit.solve_many_dev its shapes before it touches the worker — none of it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from distributed_plonk_amd import _ffi
from distributed_plonk_amd import builder as BD
from distributed_plonk_amd.worker import REPLAY_FUSE_DEFAULT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000                                                # stands for a device pointer: never followed on the host


def replay(seg, levels, *, wire_vars=PTR, sel=PTR, hint_op=None, order=PTR, pub=None, num_inputs=0, witness=PTR, K=2, n=8, fuse=0):
    """the raw entry without a context -> (return code, error text)"""
    lib = _ffi.lib()
    s = None if seg is None else np.ascontiguousarray(seg, dtype=np.uint32)
    rc = lib.plonk_circuit_replay_dev(None, wire_vars, n, 20, sel, hint_op, order, None if s is None else s.ctypes.data_as(C.c_void_p), levels, pub, num_inputs,
                                      witness, K, fuse)
    return rc, lib.plonk_last_error().decode()


GOOD_SEG = [0, 2, 2, 2, 5, 5, 6]                            # two levels


def test_replay_entry_names_the_refused_argument():
    for kw, name in ((dict(wire_vars=None), "d_wire_vars"), (dict(sel=None), "d_selector_evals"), (dict(order=None), "d_order"),
                     (dict(witness=None), "d_witness")):
        rc, err = replay(GOOD_SEG, 2, **kw)
        assert rc == -1 and "plonk_circuit_replay_dev" in err and name + " is null" in err, err
    rc, err = replay(None, 2)
    assert rc == -1 and "seg is null" in err, err
    rc, err = replay(GOOD_SEG, 2, K=0)
    assert rc == -1 and "K is 0" in err, err
    # public inputs: a pointer iff there are any, and no more than gates
    rc, err = replay(GOOD_SEG, 2, pub=PTR, num_inputs=0)
    assert rc == -1 and "d_pub_inputs" in err, err
    rc, err = replay(GOOD_SEG, 2, pub=None, num_inputs=1)
    assert rc == -1 and "d_pub_inputs" in err, err
    rc, err = replay(GOOD_SEG, 2, pub=PTR, num_inputs=9)
    assert rc == -1 and "num_inputs = 9" in err, err


def test_replay_entry_refuses_a_schedule_that_is_not_one():
    rc, err = replay([0, 2, 1, 2, 5, 5, 6], 2)
    assert rc == -1 and "seg decreases" in err and "at 1" in err, err
    rc, err = replay([0, 2, 2, 2, 5, 5, 4], 2)
    assert rc == -1 and "seg decreases" in err and "at 5" in err, err
    rc, err = replay([0, 2, 2, 2, 5, 5, 9], 2)              # n = 8
    assert rc == -1 and "seg ends at 9" in err, err
    rc, err = replay(np.zeros(28, dtype=np.uint32), 9)
    assert rc == -1 and "levels = 9" in err, err
    # a good argument list gets as far as the context
    for fuse in (0, REPLAY_FUSE_DEFAULT):
        rc, err = replay(GOOD_SEG, 2, fuse=fuse)
        assert rc == -1 and "null context" in err, err
    rc, err = replay([0], 0)
    assert rc == -1 and "null context" in err, err


def test_the_default_fuse_width_is_the_header_macro():
    text = open(os.path.join(ROOT, "include", "plonk_hip.h")).read()
    m = re.search(r"#define\s+PLONK_REPLAY_FUSE_DEFAULT\s+(\d+)", text)
    assert m and int(m.group(1)) == REPLAY_FUSE_DEFAULT
    rust = open(os.path.join(ROOT, "ffi", "plonk_hip.rs")).read()
    assert f"PLONK_REPLAY_FUSE_DEFAULT: c_uint = {REPLAY_FUSE_DEFAULT};" in rust


class NoDevice:
    """a worker that refuses every use: the shape checks come first"""
    curve_name = "bn254"

    def __getattr__(self, name):
        raise AssertionError(f"the worker was used ({name}) before the arguments were checked")


def small_circuit():
    b = BD.CircuitBuilder("bn254")
    out = b.public_input()
    x = b.input(3)
    b.enforce_equal(b.add(b.mul(x, x), out), x)
    return b.build()


def test_solve_many_dev_checks_its_shapes_before_the_device():
    built = small_circuit()
    w = NoDevice()
    z = lambda *shape: np.zeros(shape, dtype=np.uint64)
    for kw in (dict(inputs=z(2, 3, 4)),                                 # no public inputs for one public input
               dict(inputs=z(2, 3, 4), public_inputs=z(3, 1, 4)),       # two witnesses or three
               dict(inputs=z(3, 4), public_inputs=z(1, 4)),             # solve_dev's shapes: no K axis
               dict(inputs=z(2, 4, 4), public_inputs=z(2, 1, 4)),       # four values for three inputs
               dict(inputs=z(2, 3, 4), public_inputs=z(2, 2, 4)),
               dict(inputs=z(2, 3, 3), public_inputs=z(2, 1, 4)),       # not limbs
               dict(inputs=z(0, 3, 4), public_inputs=z(0, 1, 4)),       # K = 0
               dict(public_inputs=z(2, 1, 4)),                          # no inputs at all
               dict(inputs=z(2, 3, 4), public_inputs=z(2, 1, 4), K=3),
               dict(inputs=z(2, 3, 4), public_inputs=z(2, 1, 4), d_inputs=PTR),
               dict(inputs=z(2, 3, 4), public_inputs=z(2, 1, 4), fuse_width=-1)):
        with pytest.raises(ValueError):
            built.solve_many_dev(w, **kw)
    with pytest.raises(ValueError):
        built.solve_many_dev(type("Other", (), {"curve_name": "bls12_381"})(), z(2, 3, 4), z(2, 1, 4))
    # good shapes reach the worker
    with pytest.raises(AssertionError, match="the worker was used"):
        built.solve_many_dev(w, z(2, 3, 4), z(2, 1, 4))
