"""User circuits: from jellyfish's arithmetised form to a proving instance in HBM.

A circuit is what jellyfish's `preprocess` consumes: for each of the 5 wire columns and each gate the variable the wire reads,
a witness value per variable, the 13 selector columns and the public inputs.  `preprocess` turns it into what `Prover.load_key_dev`,
`Prover.verifying_key` and `Prover.prove_dev` take — the same attribute names as `synthetic.SyntheticInstance`:

    inst = preprocess(worker, Circuit(wire_vars, witness, selector_evals, public_inputs).pad(zero_var))
    pv = Prover(worker, inst.log_n)
    pv.load_key_dev(inst.sel_ptrs, inst.sig_ptrs, inst.k)
    proof = pv.prove_dev(inst.wev, inst.d_id.ptr, inst.d_idx.ptr, inst.d_pi.ptr, blinders, pv.fiat_shamir(inst.public_inputs()))

The work runs on the device: the copy-constraint permutation (plonk_circuit_permutation_dev), witness placement
(plonk_circuit_witness_dev), the satisfiability check (plonk_circuit_check_dev) and the 13 + 5 inverse NTTs into coefficient form.
For many witnesses of one circuit `setup_dev` does the witness-independent half once (a `CircuitKey`: permutation, proving key) and
`CircuitKey.instance` the rest per witness (placement, check); an instance has the attribute names above and borrows the key's buffers.
Selector order: q_lc 0-3, q_mul 4-5, q_hash 6-9, q_o 10, q_c 11, q_ecc 12.  Field elements are (.., 4) u64 Montgomery limbs.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import fr as _fr
from .synthetic import NUM_SELECTORS, NUM_WIRE_TYPES, wire_subset_separators
from .worker import DeviceScope, PlonkWorker, closing_on_error


class UnsatisfiedCircuit(ValueError):
    """The witness does not satisfy the circuit: `gate` is the first failing gate (or -1), `position` the first wire position
    p = i * n + j whose value differs from the next position of its copy cycle (or -1)."""

    def __init__(self, gate: int, position: int, n: int):
        parts = []
        if gate >= 0:
            parts.append(f"gate {gate} does not satisfy its gate equation")
        if position >= 0:
            parts.append(f"copy constraint broken at position {position} (wire {position // n} of gate {position % n})")
        super().__init__("; ".join(parts))
        self.gate, self.position = gate, position


class UnsolvableCircuit(ValueError):
    """The witness solver could not reach every defined variable: `variable` is the smallest one left, on a dependency cycle of
    defining gates or downstream of one."""

    def __init__(self, variable: int):
        super().__init__(f"variable {variable} cannot be solved: its defining gate waits for a variable on a dependency cycle")
        self.variable = variable


def _fr_array(a, shape_tail, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.shape[-len(shape_tail):] != shape_tail:
        raise ValueError(f"{what}: shape {a.shape}, expected (..., {', '.join(map(str, shape_tail))})")
    return a


class Circuit:
    """Host arrays of one circuit.

    wire_vars: (5, gates) variable ids; witness: (num_vars, 4); selector_evals: (13, gates, 4) evaluations per gate;
    public_inputs: (num_inputs, 4), the values that sit at gates 0 .. num_inputs (the IO-gate convention: such a gate reads
    its variable on wire 4 with q_o = 1, so PI - e = 0); k: (5, 4) coset representatives, default
    `synthetic.wire_subset_separators(field, 1)` of the worker's curve."""

    def __init__(self, wire_vars, witness, selector_evals, public_inputs=None, k: Optional[np.ndarray] = None):
        wv = np.asarray(wire_vars)
        if wv.ndim != 2 or wv.shape[0] != NUM_WIRE_TYPES:
            raise ValueError(f"wire_vars: shape {wv.shape}, expected ({NUM_WIRE_TYPES}, gates)")
        gates = wv.shape[1]
        if gates == 0:
            raise ValueError("a circuit needs at least one gate")
        witness = _fr_array(witness, (4,), "witness")
        if witness.ndim != 2 or witness.shape[0] == 0:
            raise ValueError(f"witness: shape {witness.shape}, expected (num_vars >= 1, 4)")
        num_vars = witness.shape[0]
        if wv.size and (wv.min() < 0 or wv.max() >= num_vars):
            raise ValueError(f"wire_vars: ids must lie in [0, {num_vars})")
        sel = _fr_array(selector_evals, (4,), "selector_evals")
        if sel.shape != (NUM_SELECTORS, gates, 4):
            raise ValueError(f"selector_evals: shape {sel.shape}, expected ({NUM_SELECTORS}, {gates}, 4)")
        pub = np.zeros((0, 4), dtype=np.uint64) if public_inputs is None else _fr_array(public_inputs, (4,), "public_inputs").reshape(-1, 4)
        if pub.shape[0] > gates:
            raise ValueError(f"{pub.shape[0]} public inputs for {gates} gates")
        if k is not None:
            k = np.ascontiguousarray(k, dtype=np.uint64)
            if k.shape != (NUM_WIRE_TYPES, 4):
                raise ValueError(f"k: shape {k.shape}, expected ({NUM_WIRE_TYPES}, 4)")
        self.wire_vars = np.ascontiguousarray(wv, dtype=np.uint32)
        self.witness, self.selector_evals, self.public_inputs, self.k = witness, sel, pub, k

    @property
    def num_gates(self) -> int:
        return self.wire_vars.shape[1]

    @property
    def num_vars(self) -> int:
        return self.witness.shape[0]

    def pad(self, zero_var: int) -> "Circuit":
        """A copy with the gate count raised to the next power of two (>= 2), as jellyfish's padding does: the new gates have zero
        selectors and all five wires read `zero_var`, whose witness value must be zero."""
        if not 0 <= zero_var < self.num_vars:
            raise ValueError(f"zero_var {zero_var} is not a variable of this circuit")
        if self.witness[zero_var].any():
            raise ValueError(f"zero_var {zero_var} has a nonzero witness value")
        g = self.num_gates
        n = max(2, 1 << (g - 1).bit_length())
        wv = np.full((NUM_WIRE_TYPES, n), zero_var, dtype=np.uint32)
        wv[:, :g] = self.wire_vars
        sel = np.zeros((NUM_SELECTORS, n, 4), dtype=np.uint64)
        sel[:, :g] = self.selector_evals
        return Circuit(wv, self.witness.copy(), sel, self.public_inputs.copy(), None if self.k is None else self.k.copy())


class PreprocessedCircuit:
    """Device buffers of one preprocessed circuit; `close()` frees them.  Attribute names follow synthetic.SyntheticInstance, so
    Prover.load_key_dev / verifying_key / prove_dev take it unchanged."""

    def __init__(self, worker: PlonkWorker, n: int, num_inputs: int, k: np.ndarray):
        self.w, self.n, self.num_inputs = worker, n, num_inputs
        self.log_n = n.bit_length() - 1
        self.k = np.ascontiguousarray(k, dtype=np.uint64)
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            alloc = lambda n_fr: self._scope.alloc(n_fr * 32)
            self.d_wires = alloc(NUM_WIRE_TYPES * n)
            self.d_id = alloc(NUM_WIRE_TYPES * n)
            self.d_idx = self._scope.alloc(NUM_WIRE_TYPES * n * 8)
            self.d_sig_ev = alloc(NUM_WIRE_TYPES * n)
            self.d_sel = alloc(NUM_SELECTORS * n)
            self.d_sig = alloc(NUM_WIRE_TYPES * n)
            self.d_pi = alloc(n)
        self.wev = [self.d_wires.ptr + i * n * 32 for i in range(NUM_WIRE_TYPES)]
        self.sel_ptrs = [self.d_sel.ptr + t * n * 32 for t in range(NUM_SELECTORS)]
        self.sig_ptrs = [self.d_sig.ptr + t * n * 32 for t in range(NUM_WIRE_TYPES)]

    def public_inputs(self) -> np.ndarray:
        """`circuit.public_input()`: the num_inputs values (not padded) -> (num_inputs, 4)."""
        return self.d_pi.download((self.num_inputs, 4))

    def download(self) -> dict:
        """Everything as host arrays (small sizes only)."""
        n = self.n
        return dict(wires=self.d_wires.download((NUM_WIRE_TYPES, n, 4)), selectors=self.d_sel.download((NUM_SELECTORS, n, 4)),
                    sigmas=self.d_sig.download((NUM_WIRE_TYPES, n, 4)), id_perm=self.d_id.download((NUM_WIRE_TYPES * n, 4)),
                    perm_idx=self.d_idx.download((NUM_WIRE_TYPES * n,)), pub_input=self.d_pi.download((n, 4)), k=self.k.copy(),
                    sigma_evals=self.d_sig_ev.download((NUM_WIRE_TYPES, n, 4)))

    def close(self):
        self._scope.close()


def default_k(curve_name: str) -> np.ndarray:
    return wire_subset_separators(_fr.FIELDS[curve_name], 1)


def preprocess_dev(worker: PlonkWorker, d_wire_vars: int, n: int, num_vars: int, d_witness: int, d_selector_evals: int, d_pub_input: int,
                   num_inputs: int, k: Optional[np.ndarray] = None, check: bool = True) -> PreprocessedCircuit:
    """`preprocess` for a circuit already in HBM: d_wire_vars u32 [5][n], d_witness num_vars Fr, d_selector_evals [13][n] Fr,
    d_pub_input n Fr (public inputs at gates 0 .. num_inputs, zero elsewhere).  The caller's buffers are read, not modified or kept.
    check: run the satisfiability check and raise UnsatisfiedCircuit naming the first failing gate / copy position."""
    if n < 2 or n & (n - 1):
        raise ValueError(f"gate count {n} is not a power of two >= 2: pad the circuit first (Circuit.pad)")
    if not 0 <= num_inputs <= n:
        raise ValueError(f"{num_inputs} public inputs for {n} gates")
    w = worker
    k = default_k(w.curve_name) if k is None else k
    inst = PreprocessedCircuit(w, n, num_inputs, k)
    with closing_on_error(inst):
        w.memcpy_d2d(inst.d_pi.ptr, d_pub_input, n * 32)
        w.circuit_permutation_dev(d_wire_vars, n, num_vars, inst.k, inst.d_id.ptr, inst.d_idx.ptr, inst.d_sig_ev.ptr)
        w.circuit_witness_dev(d_wire_vars, n, d_witness, num_vars, inst.d_wires.ptr)
        if check:
            gate, pos = w.circuit_check_dev(inst.d_wires.ptr, d_selector_evals, inst.d_pi.ptr, inst.d_idx.ptr, n)
            if gate >= 0 or pos >= 0:
                raise UnsatisfiedCircuit(gate, pos, n)
        _proving_key_polys(w, n, d_selector_evals, inst.d_sig_ev.ptr, inst.d_sel.ptr, inst.d_sig.ptr)
    return inst


def _proving_key_polys(w: PlonkWorker, n: int, d_selector_evals: int, d_sigma_evals: int, d_sel: int, d_sig: int):
    """proving key: selector and sigma polynomials in coefficient form (n-point iNTTs; ntt_dev consumes its input, so a copy goes in)"""
    with DeviceScope(w) as s:
        tmp = s.alloc(n * 32)
        for src, dst, cnt in ((d_selector_evals, d_sel, NUM_SELECTORS), (d_sigma_evals, d_sig, NUM_WIRE_TYPES)):
            for t in range(cnt):
                w.memcpy_d2d_async(tmp.ptr, src + t * n * 32, n * 32)
                w.ntt_dev(tmp.ptr, dst + t * n * 32, n, True, False)
        w.sync()


class CircuitInstance:
    """One witness of a CircuitKey's circuit, placed on the wires: what Prover.prove_dev takes, under PreprocessedCircuit's attribute names.  It
    owns its wires and d_pi alone; d_id, d_idx, sel_ptrs and sig_ptrs are the key's, which has to outlive it."""

    def __init__(self, key: "CircuitKey"):
        self.key, self.w, self.n, self.log_n, self.num_inputs, self.k = key, key.w, key.n, key.log_n, key.num_inputs, key.k
        self.d_id, self.d_idx, self.sel_ptrs, self.sig_ptrs = key.d_id, key.d_idx, key.sel_ptrs, key.sig_ptrs
        n = self.n
        self._scope = DeviceScope(self.w)
        with closing_on_error(self._scope):
            self.d_wires = self._scope.alloc(NUM_WIRE_TYPES * n * 32)
            self.d_pi = self._scope.alloc(n * 32)
        self.wev = [self.d_wires.ptr + i * n * 32 for i in range(NUM_WIRE_TYPES)]

    def public_inputs(self) -> np.ndarray:
        """`circuit.public_input()`: the num_inputs values (not padded) -> (num_inputs, 4)."""
        return self.d_pi.download((self.num_inputs, 4))

    def close(self):
        self._scope.close()


class CircuitKey:
    """What does not depend on the witness, computed once (setup_dev): the copy-constraint permutation (d_id, d_idx, d_sig_ev) and the proving
    key (d_sel, d_sig in coefficient form; sel_ptrs / sig_ptrs for Prover.load_key_dev).  d_wire_vars and d_selector_evals stay the caller's
    and are read again by every instance().  `close()` frees the key's buffers; its instances are closed on their own."""

    def __init__(self, worker: PlonkWorker, d_wire_vars: int, n: int, num_vars: int, d_selector_evals: int, num_inputs: int, k: np.ndarray):
        self.w, self.n, self.num_vars, self.num_inputs = worker, n, num_vars, num_inputs
        self.d_wire_vars, self.d_selector_evals = d_wire_vars, d_selector_evals
        self.log_n = n.bit_length() - 1
        self.k = np.ascontiguousarray(k, dtype=np.uint64)
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            alloc = self._scope.alloc
            self.d_id = alloc(NUM_WIRE_TYPES * n * 32)
            self.d_idx = alloc(NUM_WIRE_TYPES * n * 8)
            self.d_sig_ev = alloc(NUM_WIRE_TYPES * n * 32)
            self.d_sel = alloc(NUM_SELECTORS * n * 32)
            self.d_sig = alloc(NUM_WIRE_TYPES * n * 32)
        self.sel_ptrs = [self.d_sel.ptr + t * n * 32 for t in range(NUM_SELECTORS)]
        self.sig_ptrs = [self.d_sig.ptr + t * n * 32 for t in range(NUM_WIRE_TYPES)]

    def instance(self, d_witness: int, public_inputs=None, check: bool = True) -> CircuitInstance:
        """The witness at d_witness (num_vars Fr) placed on the wires.  public_inputs: a device pointer to the num_inputs values (a row of
        SolvedBatch.d_pub), or the values themselves as (num_inputs, 4) host limbs; None without public inputs.  check: run the
        satisfiability check and raise UnsatisfiedCircuit naming the first failing gate / copy position, as preprocess_dev does."""
        n, w = self.n, self.w
        if self.num_inputs and public_inputs is None:
            raise ValueError(f"no public input values for {self.num_inputs} public inputs")
        pub = None
        if self.num_inputs and not isinstance(public_inputs, (int, np.integer)):
            pub = _fr_array(public_inputs, (4,), "public_inputs").reshape(-1, 4)
            if pub.shape[0] != self.num_inputs:
                raise ValueError(f"{pub.shape[0]} public input values for {self.num_inputs} public inputs")
        inst = CircuitInstance(self)
        with closing_on_error(inst):
            w.memset_dev(inst.d_pi.ptr, 0, n * 32)
            if pub is not None:
                inst.d_pi.upload(pub)
            elif self.num_inputs:
                w.memcpy_d2d_async(inst.d_pi.ptr, int(public_inputs), self.num_inputs * 32)
            w.circuit_witness_dev(self.d_wire_vars, n, d_witness, self.num_vars, inst.d_wires.ptr)
            if check:
                gate, pos = w.circuit_check_dev(inst.d_wires.ptr, self.d_selector_evals, inst.d_pi.ptr, self.d_idx.ptr, n)
                if gate >= 0 or pos >= 0:
                    raise UnsatisfiedCircuit(gate, pos, n)
        return inst

    def instances(self, batch, check: bool = True):
        """One instance per witness of a builder.SolvedBatch, in order (a generator: close each instance when its proof is done)."""
        for b in range(batch.K):
            yield self.instance(batch.d_witness.ptr + b * self.num_vars * 32, batch.d_pub.ptr + b * self.num_inputs * 32 if self.num_inputs else None, check)

    def close(self):
        self._scope.close()


def setup_dev(worker: PlonkWorker, d_wire_vars: int, n: int, num_vars: int, d_selector_evals: int, num_inputs: int, k: Optional[np.ndarray] = None) -> CircuitKey:
    """The witness-independent half of preprocess_dev, once per circuit: the copy-constraint permutation and the 13 + 5 inverse NTTs of the
    proving key.  d_wire_vars u32 [5][n], d_selector_evals [13][n] Fr: read now and by every CircuitKey.instance, not modified or owned."""
    if n < 2 or n & (n - 1):
        raise ValueError(f"gate count {n} is not a power of two >= 2: pad the circuit first (Circuit.pad)")
    if not 0 <= num_inputs <= n:
        raise ValueError(f"{num_inputs} public inputs for {n} gates")
    w = worker
    key = CircuitKey(w, d_wire_vars, n, num_vars, d_selector_evals, num_inputs, default_k(w.curve_name) if k is None else k)
    with closing_on_error(key):
        w.circuit_permutation_dev(d_wire_vars, n, num_vars, key.k, key.d_id.ptr, key.d_idx.ptr, key.d_sig_ev.ptr)
        _proving_key_polys(w, n, d_selector_evals, key.d_sig_ev.ptr, key.d_sel.ptr, key.d_sig.ptr)
    return key


def preprocess(worker: PlonkWorker, circuit: Circuit, check: bool = True) -> PreprocessedCircuit:
    """Upload a Circuit (gate count a power of two: Circuit.pad) and run preprocess_dev on it."""
    n = circuit.num_gates
    if n < 2 or n & (n - 1):
        raise ValueError(f"gate count {n} is not a power of two >= 2: pad the circuit first (Circuit.pad)")
    pub = np.zeros((n, 4), dtype=np.uint64)
    pub[:circuit.public_inputs.shape[0]] = circuit.public_inputs
    w = worker
    with DeviceScope(w) as s:
        up = lambda a: s.alloc(max(a.nbytes, 8)).upload(a).ptr
        d_vars, d_wit, d_sel, d_pub = up(circuit.wire_vars), up(circuit.witness), up(circuit.selector_evals), up(pub)
        return preprocess_dev(w, d_vars, n, circuit.num_vars, d_wit, d_sel, d_pub, circuit.public_inputs.shape[0], circuit.k, check)
