"""distributed_plonk_amd.circuit.Circuit on the host: shape checks and pad() (no device involved)."""
import numpy as np
import pytest

from distributed_plonk_amd.circuit import Circuit


def _circuit(gates=5, num_vars=7, num_inputs=1):
    rs = np.random.RandomState(gates)
    wv = rs.randint(1, num_vars, size=(5, gates))
    wit = rs.randint(1, 1 << 60, size=(num_vars, 4)).astype(np.uint64)
    wit[0] = 0
    sel = rs.randint(1, 1 << 60, size=(13, gates, 4)).astype(np.uint64)
    pub = rs.randint(1, 1 << 60, size=(num_inputs, 4)).astype(np.uint64)
    return Circuit(wv, wit, sel, pub)


def test_shapes_are_checked():
    c = _circuit()
    assert c.num_gates == 5 and c.num_vars == 7 and c.wire_vars.dtype == np.uint32
    with pytest.raises(ValueError, match="wire_vars"):
        Circuit(np.zeros((4, 5)), c.witness, c.selector_evals)
    with pytest.raises(ValueError, match="ids"):
        Circuit(np.full((5, 5), 7), c.witness, c.selector_evals)
    with pytest.raises(ValueError, match="selector_evals"):
        Circuit(c.wire_vars, c.witness, c.selector_evals[:12])
    with pytest.raises(ValueError, match="witness"):
        Circuit(c.wire_vars, c.witness[:, :3], c.selector_evals)
    with pytest.raises(ValueError, match="public inputs"):
        Circuit(c.wire_vars, c.witness, c.selector_evals, np.zeros((6, 4), dtype=np.uint64))
    with pytest.raises(ValueError, match="k"):
        Circuit(c.wire_vars, c.witness, c.selector_evals, k=np.zeros((4, 4), dtype=np.uint64))


@pytest.mark.parametrize("gates,want", [(1, 2), (2, 2), (5, 8), (8, 8), (1000, 1024)])
def test_pad_to_a_power_of_two(gates, want):
    c = _circuit(gates=gates)
    p = c.pad(0)
    assert p.num_gates == want and p.num_vars == c.num_vars
    assert np.array_equal(p.wire_vars[:, :gates], c.wire_vars)
    assert (p.wire_vars[:, gates:] == 0).all()
    assert np.array_equal(p.selector_evals[:, :gates], c.selector_evals)
    assert not p.selector_evals[:, gates:].any()
    assert np.array_equal(p.public_inputs, c.public_inputs) and np.array_equal(p.witness, c.witness)
    assert c.num_gates == gates                        # the original is unchanged


def test_pad_needs_a_zero_variable():
    c = _circuit()
    with pytest.raises(ValueError, match="nonzero"):
        c.pad(3)
    with pytest.raises(ValueError, match="not a variable"):
        c.pad(7)
