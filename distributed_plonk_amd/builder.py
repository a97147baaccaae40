"""Building a circuit from operations, and solving its witness on the device.

The reference's end-to-end test does not write selector tables: it builds its circuit with jellyfish's constraint builder
(`PlonkCircuit::new`, `create_variable`, the arithmetic gates; generate_circuit, dispatcher2.rs:1226-1271) and the builder knows the
witness.  `CircuitBuilder` is the array-oriented counterpart on the host: every operation takes variable ids as scalars or 1-D integer
arrays broadcast against each other, emits one gate per element in one numpy step and returns the ids of the new variables, so a
2^22-gate circuit is a few hundred calls.  `build()` gives a `BuiltCircuit`: exactly the arrays `circuit.Circuit` takes, padded to a
power of two, plus `def_gate` — which gate defines each variable.  From the values of the inputs and public inputs alone
`BuiltCircuit.solve_dev` has the device evaluate every defining gate in dependency order (plonk_circuit_solve_dev), and
`BuiltCircuit.preprocess` continues into `circuit.preprocess_dev` without the witness leaving HBM:

    b = CircuitBuilder("bn254")
    x, y = b.input(2)
    out = b.public_input()
    t = b.pow5_lc([x, y], [1, 3], const=7)            # x^5 + 3 y^5 + 7
    b.enforce_equal(b.mul(t, y), out)
    inst = b.build().preprocess(worker, inputs, public_inputs)      # a circuit.PreprocessedCircuit

Values that no gate equation yields — an inverse, a quotient, a fifth root, a bit — are HINTED: `inv`, `inv_or_zero`, `div`, `root5` and `bit`
emit one gate whose selectors check the value and whose `hint_op` entry tells the device solver how to compute it from the gate's source
wires (plonk_circuit_solve_hints_dev); `to_bits`, `range_check`, `is_zero`, `is_equal`, `select` and `less_than` are composed from them.

Hashing: `rescue_permutation`, `rescue_hash2` and `merkle_root` emit the Rescue permutation of rescue.py (148 gates per instance, from `lc`,
`root5` and `pow5_lc`), so a path of a rescue.MerkleTree built on the device is proved against its root; `rescue_hash3` and `accumulator_root`
do the same for the ternary rescue.Accumulator (membership.py builds the reference's generate_circuit shape from them).  Inputs that are
already on the device — a rescue.Accumulator's witness_inputs_dev — go into a solve as `d_inputs=` and never visit the host.

Curve points: a point is a pair (x_ids, y_ids) on the twisted Edwards curve embedded in Fr (edwards.py: Baby Jubjub, Jubjub), whose complete
addition law needs no case distinction and hence no selector of its own — `point_add` (9 gates), `point_double`, `point_select`, `point_neg`,
`enforce_on_curve`, `to_bits_strict` (every bit of the canonical residue), `scalar_mul`, `fixed_base_mul` and `schnorr_verify` are composed
from `mul`, `mul_add`, `lc` and `div`; edwards.py computes the same group on the device and `edwards.schnorr_circuit` builds the circuit.

Vectors and encryption: `rescue_sponge` hashes a list of variables (the sponge of rescue.py: the length sits in the capacity),
`rescue_stream` gives the counter-mode keystream under a key variable, and `elgamal_encrypt` proves a ciphertext of elgamal.py —
E = [r] G, the key from [r] ek, the stream added to the message — from `fixed_base_mul`, `scalar_mul` and the two; `elgamal.elgamal_circuit`
builds the circuit.

Same circuit, next witness: `BuiltCircuit.schedule` records the solver's order of evaluation once (plonk_circuit_schedule_dev),
`solve_many_dev` replays it for K witnesses in one go (plonk_circuit_replay_dev; each witness bit-identical to solve_dev's), and `setup`
gives a `circuit.CircuitKey` — permutation and proving key, once — whose `instances(batch)` are what `Prover.prove_dev` takes per witness.

Field constants are Python ints (or sequences of them, one per gate), reduced mod r.  Gate equation and selector order: circuit.py.
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence

import numpy as np

from . import circuit as _circuit
from . import fr as _fr
from .synthetic import NUM_SELECTORS, NUM_WIRE_TYPES
from .worker import REPLAY_FUSE_DEFAULT, DeviceScope, PlonkWorker, closing_on_error

SELECTOR_INDEX = {**{f"q_lc{i}": i for i in range(4)}, "q_mul0": 4, "q_mul1": 5, **{f"q_hash{i}": 6 + i for i in range(4)}, "q_o": 10, "q_c": 11}
GIVEN = 0xFFFFFFFF                                    # def_gate of a variable no gate defines
HINT_INV, HINT_DIV, HINT_ROOT5, HINT_BIT = 1, 2, 3, 4 # hint_op opcodes (bits 0-7; bits 8-31: the argument, BIT's bit index)
HINT_BIT_ARGS = 256                                   # BIT indices lie in [0, 256)
_SCALARS = (int, np.integer)


class BuiltCircuit:
    """What CircuitBuilder.build() returns.  wire_vars (5, n) u32, selector_evals (13, n, 4) Montgomery limbs, n a power of two (jellyfish's
    padding gates at the end); def_gate (num_vars,) u32: the gate that defines the variable, GIVEN for an input; input_vars / public_vars:
    the ids whose values `inputs` / `public_inputs` carry, in that order; the IO gate of public_vars[i] is gate i.  hint_op (n,) u32 or None:
    opcode | argument << 8 per gate, 0 for an ordinary gate (see HINT_*); None stands for all zero."""

    def __init__(self, curve: str, wire_vars, selector_evals, num_vars: int, def_gate, input_vars, public_vars, zero_var: int, num_gates: int, *,
                 hint_op=None):
        self.curve, self.wire_vars, self.selector_evals, self.num_vars, self.def_gate = curve, wire_vars, selector_evals, num_vars, def_gate
        self.input_vars, self.public_vars, self.zero_var = input_vars, public_vars, zero_var
        self.num_public = len(public_vars)
        self.num_gates_unpadded = num_gates
        if hint_op is None:
            hint_op = np.zeros(wire_vars.shape[1], dtype=np.uint32)
        self.hint_op = np.ascontiguousarray(hint_op, dtype=np.uint32)
        if self.hint_op.shape != (wire_vars.shape[1],):
            raise ValueError(f"hint_op of shape {self.hint_op.shape} for {wire_vars.shape[1]} gates")
        self._dev = None                              # (worker, [wire_vars, selector_evals, def_gate(, hint_op)] device buffers)
        self._dev_input_vars = None                   # input_vars as u32 on the same worker, once a solve took d_inputs
        self._schedule = None                         # the SolveSchedule of the upload, once schedule() recorded it

    @property
    def n(self) -> int:
        return self.wire_vars.shape[1]

    @property
    def log_n(self) -> int:
        return self.n.bit_length() - 1

    @property
    def has_hints(self) -> bool:
        """whether solve_dev goes through plonk_circuit_solve_hints_dev (some hint_op entry is non-zero) or plonk_circuit_solve_dev"""
        return bool(self.hint_op.any())

    def _upload(self, worker: PlonkWorker):
        if self._dev is not None and self._dev[0] is not worker:
            self.close()
        if self._dev is None:
            with DeviceScope(worker) as s:
                bufs = [s.upload(a) for a in (self.wire_vars, self.selector_evals, self.def_gate) + ((self.hint_op,) if self.has_hints else ())]
                self._dev = (worker, [s.release(b) for b in bufs])
        return self._dev[1]

    def close(self):
        """Free the device copy of the circuit that solve_dev keeps between calls.  _upload, _input_vars_dev and schedule each released theirs to
        this object when they had filled them, so they are freed one by one here."""
        if self._dev is not None:
            for b in self._dev[1]:
                b.free()
            self._dev = None
        if self._dev_input_vars is not None:
            self._dev_input_vars.free()
            self._dev_input_vars = None
        if self._schedule is not None:
            self._schedule.d_order.free()
            self._schedule = None

    def _input_vars_dev(self, worker: PlonkWorker):
        if self._dev_input_vars is None:
            ids = np.ascontiguousarray(self.input_vars, dtype=np.uint32)
            with DeviceScope(worker) as s:
                self._dev_input_vars = s.release(s.alloc(max(4, ids.nbytes)).upload(ids))
        return self._dev_input_vars

    def schedule(self, worker: PlonkWorker) -> "SolveSchedule":
        """The order in which the solver evaluates this circuit's defining gates (plonk_circuit_schedule_dev): a function of the circuit alone,
        recorded once per upload and kept until close().  Raises circuit.UnsolvableCircuit as solve_dev does."""
        if worker.curve_name != self.curve:
            raise ValueError(f"circuit over {self.curve}, worker over {worker.curve_name}")
        d_vars, d_sel, d_def, *d_hint = self._upload(worker)
        if self._schedule is None:
            with DeviceScope(worker) as s:
                d_order = s.alloc(self.n * 4)
                unsolved, levels, evaluations, seg = worker.circuit_schedule_dev(d_vars.ptr, self.n, self.num_vars, d_sel.ptr, d_def.ptr,
                                                                                 d_hint[0].ptr if d_hint else 0, d_order.ptr)
                if unsolved >= 0:
                    raise _circuit.UnsolvableCircuit(unsolved)
                self._schedule = SolveSchedule(s.release(d_order), seg, levels, evaluations)
        return self._schedule

    def solve_many_dev(self, worker: PlonkWorker, inputs=None, public_inputs=None, *, d_inputs: Optional[int] = None, fuse_width: Optional[int] = None,
                       K: Optional[int] = None) -> "SolvedBatch":
        """solve_dev for K witnesses of this circuit at once, by replaying its schedule() (plonk_circuit_replay_dev): witness b is bit-identical
        to what solve_dev gives for inputs[b], public_inputs[b].  inputs: (K, len(input_vars), 4), public_inputs: (K, num_public, 4) Montgomery
        limbs; d_inputs, instead of `inputs`: a device pointer to the same K x len(input_vars) values, scattered on the device.  K: only needed
        where neither array tells it.  fuse_width: see PlonkWorker.circuit_replay_dev; the result does not depend on it.  The work is enqueued;
        SolvedBatch.witness, or any synchronising call, waits for it.  Shape errors are ValueError.  -> SolvedBatch (close() it)."""
        if worker.curve_name != self.curve:
            raise ValueError(f"circuit over {self.curve}, worker over {worker.curve_name}")
        if d_inputs is not None and inputs is not None:
            raise ValueError("inputs and d_inputs: one of them")
        num_in = len(self.input_vars)
        inp = None if inputs is None else np.ascontiguousarray(inputs, dtype=np.uint64)
        pub = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if inp is not None and (inp.ndim != 3 or inp.shape[1:] != (num_in, 4)):
            raise ValueError(f"inputs: shape {inp.shape}, expected (K, {num_in}, 4)")
        if pub is not None and (pub.ndim != 3 or pub.shape[1:] != (self.num_public, 4)):
            raise ValueError(f"public_inputs: shape {pub.shape}, expected (K, {self.num_public}, 4)")
        counts = {int(x) for x in (K, None if inp is None else inp.shape[0], None if pub is None else pub.shape[0]) if x is not None}
        if len(counts) != 1:
            raise ValueError(f"the number of witnesses: {sorted(counts) or 'not given (inputs, public_inputs or K)'}")
        K = counts.pop()
        if K < 1:
            raise ValueError(f"{K} witnesses")
        if inp is None and d_inputs is None and num_in:
            raise ValueError(f"no input values for {num_in} inputs")
        if pub is None and self.num_public:
            raise ValueError(f"no public input values for {self.num_public} public inputs")
        if fuse_width is None:
            fuse_width = REPLAY_FUSE_DEFAULT
        if not 0 <= fuse_width < 1 << 32:
            raise ValueError(f"fuse_width {fuse_width}")
        sched = self.schedule(worker)
        d_vars, d_sel, _, *d_hint = self._upload(worker)
        out = SolvedBatch(worker, self, K, d_vars.ptr, d_sel.ptr)
        with closing_on_error(out):
            if d_inputs is None:
                witness = np.zeros((K, self.num_vars, 4), dtype=np.uint64)
                if num_in:
                    witness[:, self.input_vars] = inp
                out.d_witness.upload(witness)
                del witness
            else:
                worker.memset_dev(out.d_witness.ptr, 0, K * self.num_vars * 32)
                ids = self._input_vars_dev(worker)
                for b in range(K):
                    worker.circuit_scatter_inputs_dev(ids.ptr, num_in, d_inputs + b * num_in * 32, out.d_witness.ptr + b * self.num_vars * 32, self.num_vars)
            if self.num_public:
                out.d_pub.upload(pub)
            worker.circuit_replay_dev(d_vars.ptr, self.n, self.num_vars, d_sel.ptr, d_hint[0].ptr if d_hint else 0, sched.d_order.ptr, sched.seg, sched.levels,
                                      out.d_pub.ptr if self.num_public else 0, self.num_public, out.d_witness.ptr, K, fuse_width)
        return out

    def setup(self, worker: PlonkWorker, k: Optional[np.ndarray] = None) -> _circuit.CircuitKey:
        """circuit.setup_dev on this circuit's upload: the permutation and the proving key, once for every witness.  The key reads the upload
        (wire_vars, selector_evals) whenever it makes an instance: close() the key before the circuit."""
        if worker.curve_name != self.curve:
            raise ValueError(f"circuit over {self.curve}, worker over {worker.curve_name}")
        d_vars, d_sel, *_ = self._upload(worker)
        return _circuit.setup_dev(worker, d_vars.ptr, self.n, self.num_vars, d_sel.ptr, self.num_public, k)

    def solve_dev(self, worker: PlonkWorker, inputs=None, public_inputs=None, *, d_inputs: Optional[int] = None) -> "SolvedWitness":
        """inputs: (len(input_vars), 4), public_inputs: (num_public, 4) Montgomery limbs.  The circuit is uploaded once per worker and kept
        (close() frees it); the witness buffer gets the inputs and zero, the device fills in every defined variable.  d_inputs, instead of
        `inputs`: a device pointer to the same (len(input_vars), 4) values, scattered into the witness buffer on the device
        (plonk_circuit_scatter_inputs_dev).  Raises circuit.UnsolvableCircuit naming the smallest variable on a dependency cycle.
        -> SolvedWitness (device buffers; close() it)."""
        if worker.curve_name != self.curve:
            raise ValueError(f"circuit over {self.curve}, worker over {worker.curve_name}")
        if d_inputs is not None and inputs is not None:
            raise ValueError("inputs and d_inputs: one of them")
        inp = np.ascontiguousarray(np.zeros((0, 4)) if inputs is None else inputs, dtype=np.uint64).reshape(-1, 4)
        pub = np.ascontiguousarray(np.zeros((0, 4)) if public_inputs is None else public_inputs, dtype=np.uint64).reshape(-1, 4)
        if d_inputs is None and inp.shape[0] != len(self.input_vars):
            raise ValueError(f"{inp.shape[0]} input values for {len(self.input_vars)} inputs")
        if pub.shape[0] != self.num_public:
            raise ValueError(f"{pub.shape[0]} public input values for {self.num_public} public inputs")
        d_vars, d_sel, d_def, *d_hint = self._upload(worker)
        n = self.n
        out = SolvedWitness(worker, self, d_vars.ptr, d_sel.ptr)
        with closing_on_error(out):
            if d_inputs is None:
                witness = np.zeros((self.num_vars, 4), dtype=np.uint64)
                witness[self.input_vars] = inp
                out.d_witness.upload(witness)
                del witness
            else:
                worker.memset_dev(out.d_witness.ptr, 0, self.num_vars * 32)
                worker.circuit_scatter_inputs_dev(self._input_vars_dev(worker).ptr, len(self.input_vars), d_inputs, out.d_witness.ptr, self.num_vars)
            worker.memset_dev(out.d_pub.ptr, 0, n * 32)
            if self.num_public:
                out.d_pub.upload(pub)
            if d_hint:
                unsolved, out.levels, out.evaluations = worker.circuit_solve_hints_dev(d_vars.ptr, n, self.num_vars, d_sel.ptr, out.d_pub.ptr, d_def.ptr,
                                                                                       d_hint[0].ptr, out.d_witness.ptr)
            else:
                unsolved, out.levels, out.evaluations = worker.circuit_solve_dev(d_vars.ptr, n, self.num_vars, d_sel.ptr, out.d_pub.ptr, d_def.ptr,
                                                                                 out.d_witness.ptr)
            if unsolved >= 0:
                raise _circuit.UnsolvableCircuit(unsolved)
        return out

    def preprocess(self, worker: PlonkWorker, inputs=None, public_inputs=None, check: bool = True, k: Optional[np.ndarray] = None, *,
                   d_inputs: Optional[int] = None) -> _circuit.PreprocessedCircuit:
        """solve_dev, then circuit.preprocess_dev on the same device buffers.  check: the satisfiability kernel validates every gate, the
        constraints included, so a wrong input raises circuit.UnsatisfiedCircuit."""
        s = self.solve_dev(worker, inputs, public_inputs, d_inputs=d_inputs)
        try:
            return _circuit.preprocess_dev(worker, s.d_wire_vars, self.n, self.num_vars, s.d_witness.ptr, s.d_selector_evals, s.d_pub.ptr, self.num_public,
                                           k, check)
        finally:
            s.close()

    def circuit(self, worker: PlonkWorker, inputs, public_inputs=None) -> _circuit.Circuit:
        """The same circuit as host arrays with the solved witness downloaded (small sizes, tests)."""
        s = self.solve_dev(worker, inputs, public_inputs)
        try:
            return _circuit.Circuit(self.wire_vars, s.witness(), self.selector_evals, s.d_pub.download((self.num_public, 4)))
        finally:
            s.close()


class SolvedWitness:
    """Device buffers of one solve: d_witness (num_vars Fr) and d_pub (n Fr, public inputs at the IO gates), beside the pointers of the
    circuit's own upload (owned by the BuiltCircuit).  levels / evaluations: what the solver reports."""

    def __init__(self, worker: PlonkWorker, built: BuiltCircuit, d_wire_vars: int, d_selector_evals: int):
        self.built, self.d_wire_vars, self.d_selector_evals = built, d_wire_vars, d_selector_evals
        self.levels = self.evaluations = 0
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            self.d_witness, self.d_pub = self._scope.alloc(built.num_vars * 32), self._scope.alloc(built.n * 32)

    def witness(self) -> np.ndarray:
        return self.d_witness.download((self.built.num_vars, 4))

    def close(self):
        self._scope.close()


class SolveSchedule:
    """What BuiltCircuit.schedule() records, owned by the BuiltCircuit: d_order (device, u32 [n]) holds the `evaluations` defining gates sorted by
    (level, cost class, gate); seg (3 levels + 1,) u32: seg[3 L + c] is where class c of level L starts (0 gates and BIT hints, 1 INV / DIV,
    2 ROOT5), the last word = evaluations.  levels / evaluations: what solve_dev reports for the same circuit."""

    def __init__(self, d_order, seg: np.ndarray, levels: int, evaluations: int):
        self.d_order, self.seg, self.levels, self.evaluations = d_order, seg, levels, evaluations

    def order(self) -> np.ndarray:
        """the evaluated gates in replay order -> (evaluations,) u32"""
        return self.d_order.download((self.evaluations,), dtype=np.uint32)


class SolvedBatch:
    """Device buffers of one solve_many_dev: d_witness (K x num_vars Fr, witness b at byte b * num_vars * 32) and d_pub (K x num_public Fr, the
    public inputs as given — not padded to the gates), beside the pointers of the circuit's own upload (owned by the BuiltCircuit)."""

    def __init__(self, worker: PlonkWorker, built: BuiltCircuit, K: int, d_wire_vars: int, d_selector_evals: int):
        self.built, self.K, self.d_wire_vars, self.d_selector_evals = built, K, d_wire_vars, d_selector_evals
        self._scope = DeviceScope(worker)
        with closing_on_error(self._scope):
            self.d_witness, self.d_pub = self._scope.alloc(K * built.num_vars * 32), self._scope.alloc(max(8, K * built.num_public * 32))

    def witness(self, b: int) -> np.ndarray:
        """witness b -> (num_vars, 4); waits for the solve"""
        if not 0 <= b < self.K:
            raise IndexError(f"witness {b} of {self.K}")
        return self.d_witness.download((self.built.num_vars, 4), byte_offset=b * self.built.num_vars * 32)

    def close(self):
        self._scope.close()


class CircuitBuilder:
    """Collects gates; see the module docstring.  Variable 0 is `zero`, variable 1 is `one` (each pinned by a constant gate, as jellyfish's
    PlonkCircuit::new does); unused wires read `zero`.  A refused call (unknown id, mismatched lengths, ...) raises ValueError and emits
    nothing."""

    def __init__(self, curve: str):
        self.curve = curve
        self.field = _fr.FIELDS[curve]
        self.num_vars = 0
        self._chunks = []                             # (wires (5, k) int64, {selector index: int | list of k ints}, defines, is_io[, hint_op (k,) u32])
        self._inputs = []
        self._publics = []
        self._constants = {}
        self.zero = None
        self.zero = self.constant(0)
        self.one = self.constant(1)

    @property
    def num_gates(self) -> int:
        return sum(c[0].shape[1] for c in self._chunks)

    # ------------------------------------------------------------------ arguments
    def _new_vars(self, count: int) -> np.ndarray:
        ids = np.arange(self.num_vars, self.num_vars + count, dtype=np.int64)
        self.num_vars += count
        if self.num_vars > GIVEN - 1:
            raise ValueError("more than 2^32 - 2 variables")
        return ids

    def _var(self, a) -> np.ndarray:
        v = np.asarray(a)
        if v.dtype.kind not in "iu" or v.ndim > 1:
            raise ValueError(f"variable ids must be integers, scalar or 1-D (got dtype {v.dtype}, shape {v.shape})")
        if v.size and (int(v.min()) < 0 or int(v.max()) >= self.num_vars):
            raise ValueError(f"unknown variable id (ids lie in [0, {self.num_vars}))")
        return v.astype(np.int64)

    def _coef(self, c):
        p = self.field.p
        if isinstance(c, _SCALARS):
            return int(c) % p
        vals = [int(x) % p for x in (c.tolist() if isinstance(c, np.ndarray) else list(c))]
        return vals

    def _emit(self, wires4: Sequence, selectors: Mapping[str, object], out=None, is_io: bool = False):
        """One gate per element of the broadcast arguments.  out None: wire 4 is a fresh variable that the gate defines."""
        if len(wires4) != 4:
            raise ValueError(f"{len(wires4)} input wires, a gate has 4")
        wires = [self._var(w) for w in wires4] + ([] if out is None else [self._var(out)])
        sel = {}
        for name, val in selectors.items():
            if name not in SELECTOR_INDEX:
                raise ValueError(f"unknown selector {name!r} (one of {', '.join(SELECTOR_INDEX)})")
            sel[SELECTOR_INDEX[name]] = self._coef(val)
        sel.setdefault(SELECTOR_INDEX["q_o"], 1)
        lens = [w.shape[0] for w in wires if w.ndim] + [len(v) for v in sel.values() if isinstance(v, list)]
        k = max(lens, default=1)
        if any(l not in (1, k) for l in lens):
            raise ValueError(f"mismatched lengths {sorted(set(lens))}: array arguments must have one length (or length 1)")
        scalar = not lens
        for t, v in sel.items():
            if isinstance(v, list):
                sel[t] = v[0] if len(v) == 1 else v
        if out is None:
            q_o = sel[SELECTOR_INDEX["q_o"]]
            if (q_o == 0) if isinstance(q_o, int) else (0 in q_o):
                raise ValueError("a gate that defines its output needs q_o != 0")
        wv = np.empty((NUM_WIRE_TYPES, k), dtype=np.int64)
        for i, w in enumerate(wires):
            wv[i] = w
        new = None
        if out is None:
            new = self._new_vars(k)
            wv[4] = new
        self._chunks.append((wv, {t: v for t, v in sel.items() if isinstance(v, list) or v != 0}, out is None, is_io))
        if new is None:
            return None
        return int(new[0]) if scalar else new

    # ------------------------------------------------------------------ variables
    def input(self, count: int = 1):
        """`count` given variables (their values come with solve_dev's `inputs`, in order of creation) -> id, or ids for count > 1."""
        ids = self._new_vars(count)
        self._inputs.append(ids)
        return int(ids[0]) if count == 1 else ids

    def public_input(self, count: int = 1):
        """`count` variables each defined by an IO gate (wire 4, q_o = 1, PI - e = 0); build() puts those gates first."""
        z = np.full(count, self.zero, dtype=np.int64)
        ids = self._emit([z, z, z, z], {}, is_io=True)
        self._publics.append(ids)
        return int(ids[0]) if count == 1 else ids

    def constant(self, c: int) -> int:
        """The variable of a gate q_c = c, q_o = 1; equal constants share one."""
        c = int(c) % self.field.p
        if c not in self._constants:
            if self.zero is None:                     # the zero variable's own gate: its dead wires read itself
                v = int(self._new_vars(1)[0])
                self._chunks.append((np.full((NUM_WIRE_TYPES, 1), v, dtype=np.int64), {SELECTOR_INDEX["q_o"]: 1}, True, False))
                self._constants[c] = v
            else:
                z = self.zero
                self._constants[c] = self._emit([z, z, z, z], {"q_c": c})
        return self._constants[c]

    # ------------------------------------------------------------------ gates that define a variable
    def gate(self, wires4: Sequence, selectors: Mapping[str, object], out=None):
        """The general form: wires 0-3 and any of q_lc0..3, q_mul0..1, q_hash0..3, q_o (default 1), q_c.  Without `out` the gate defines a fresh
        variable on wire 4, (q_c + sum q_lc w + q_mul0 ab + q_mul1 cd + sum q_hash w^5) / q_o, and returns it; with `out` (existing ids) it is a
        constraint on them and returns None."""
        return self._emit(wires4, selectors, out=out)

    def _terms(self, vars_, coeffs, prefix: str) -> tuple:
        vars_, coeffs = list(vars_), list(coeffs)
        if len(vars_) > 4:
            raise ValueError(f"{len(vars_)} terms: a gate takes at most 4")
        if len(vars_) != len(coeffs):
            raise ValueError(f"mismatched lengths: {len(vars_)} variables, {len(coeffs)} coefficients")
        wires = vars_ + [self.zero] * (4 - len(vars_))
        return wires, {f"{prefix}{i}": c for i, c in enumerate(coeffs)}

    def lc(self, vars_, coeffs, const=0):
        """sum coeff_i * w_i + const, up to 4 terms."""
        wires, sel = self._terms(vars_, coeffs, "q_lc")
        return self._emit(wires, {**sel, "q_c": const})

    def pow5_lc(self, vars_, coeffs, const=0):
        """sum coeff_i * w_i^5 + const, up to 4 terms: the Rescue-style q_hash gate."""
        wires, sel = self._terms(vars_, coeffs, "q_hash")
        return self._emit(wires, {**sel, "q_c": const})

    def add(self, a, b):
        return self._emit([a, b, self.zero, self.zero], {"q_lc0": 1, "q_lc1": 1})

    def sub(self, a, b):
        return self._emit([a, b, self.zero, self.zero], {"q_lc0": 1, "q_lc1": -1})

    def mul(self, a, b):
        return self._emit([a, b, self.zero, self.zero], {"q_mul0": 1})

    def mul_add(self, a, b, c, d, q0=1, q1=1):
        """q0 * a b + q1 * c d"""
        return self._emit([a, b, c, d], {"q_mul0": q0, "q_mul1": q1})

    # ------------------------------------------------------------------ hinted variables
    def _hint(self, wires4, selectors, op: int, arg=0):
        """One hint gate per element: [w0, w1, s0, s1 | y] with q_o = 0, y fresh and computed by the solver from s0, s1 (hint_op = op | arg << 8).
        None among wires 0-1 stands for y itself."""
        ws = [None if w is None else self._var(w) for w in wires4]
        a = np.asarray(arg)
        if a.dtype.kind not in "iu" or a.ndim > 1:
            raise ValueError("a bit index must be an integer, scalar or 1-D")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= HINT_BIT_ARGS):
            raise ValueError(f"bit index outside [0, {HINT_BIT_ARGS})")
        lens = [w.shape[0] for w in ws if w is not None and w.ndim] + ([a.shape[0]] if a.ndim else [])
        k = max(lens, default=1)
        if any(l not in (1, k) for l in lens):
            raise ValueError(f"mismatched lengths {sorted(set(lens))}: array arguments must have one length (or length 1)")
        sel = {SELECTOR_INDEX[name]: self._coef(val) for name, val in selectors.items()}
        new = self._new_vars(k)
        wv = np.empty((NUM_WIRE_TYPES, k), dtype=np.int64)
        for i, w in enumerate(ws):
            wv[i] = new if w is None else w
        wv[4] = new
        hint = (np.uint32(op) | (np.broadcast_to(a, (k,)).astype(np.uint32) << np.uint32(8))).astype(np.uint32)
        self._chunks.append((wv, {t: v for t, v in sel.items() if v != 0}, True, False, hint))
        return new if lens else int(new[0])

    def inv(self, x):
        """y = 1 / x, checked by x * y = 1: x = 0 leaves the circuit unsatisfied (the solver then writes y = 0)."""
        return self._hint([x, None, x, self.zero], {"q_mul0": 1, "q_c": -1}, HINT_INV)

    def inv_or_zero(self, x):
        """y = 1 / x, or 0 for x = 0, with NO constraint of its own: the caller constrains y (is_zero does)."""
        return self._hint([self.zero, self.zero, x, self.zero], {}, HINT_INV)

    def div(self, a, b):
        """y = a / b, checked by y * b = a.  b = 0: y = 0, satisfied only for a = 0."""
        return self._hint([None, b, a, b], {"q_mul0": 1, "q_lc2": -1}, HINT_DIV)

    def root5(self, x):
        """y = x^(1/5), checked by y^5 = x: the inverse S-box of a Rescue round in one gate (x -> x^5 is a bijection of the field)."""
        return self._hint([None, self.zero, x, self.zero], {"q_hash0": 1, "q_lc2": -1}, HINT_ROOT5)

    def bit(self, x, k):
        """y = bit k (scalar or per element, < 256) of the canonical residue of x, checked by y * y = y.  That y is THE bit of x is up to the
        caller's recomposition (to_bits)."""
        return self._hint([None, None, x, self.zero], {"q_mul0": 1, "q_lc0": -1}, HINT_BIT, k)

    def _nbits(self, nbits, most: int) -> int:
        if not isinstance(nbits, _SCALARS) or not 1 <= int(nbits) <= most:
            raise ValueError(f"nbits = {nbits!r}: an integer in 1 .. {most} (the field has {self.field.p.bit_length()} bits)")
        return int(nbits)

    def to_bits(self, x, nbits: int):
        """The nbits low bits of x, LSB first, as a list of id arrays, with x = sum 2^i bit_i enforced: nbits bit gates and a chain of 4-term
        lc gates from the top bits down, the last one a constraint on x — at most nbits + ceil(nbits / 3) + 1 gates per element.
        nbits in 1 .. bit_length(r) - 1 (beyond that the decomposition is not unique).  Unsatisfied for x >= 2^nbits."""
        nbits = self._nbits(nbits, self.field.p.bit_length() - 1)
        x = self._var(x)
        bits = [self.bit(x, k) for k in range(nbits)]
        return self._recompose(bits, x)

    def _recompose(self, bits: list, x):
        """x = sum 2^i bits[i] (mod r) enforced; -> bits"""
        nbits = len(bits)
        # Horner from the top: acc <- 2^j acc + (the next j bits), 3 bits per gate; the last gate has x on wire 4
        acc, at = None, nbits
        while True:
            take = min(3 if acc is not None else 4, at)
            final = at - take == 0
            terms = bits[at - take:at]
            wires = ([acc] if acc is not None else []) + terms
            coeffs = ([1 << take] if acc is not None else []) + [1 << i for i in range(take)]
            at -= take
            if final:
                w, sel = self._terms(wires, coeffs, "q_lc")
                self._emit(w, sel, out=x)
                return bits
            acc = self.lc(wires, coeffs)

    def range_check(self, x, nbits: int):
        """x < 2^nbits (nbits as in to_bits)"""
        self.to_bits(x, nbits)

    def is_zero(self, x):
        """b = 1 if x = 0 else 0: y = inv_or_zero(x), b = 1 - x y, and x b = 0 enforced (3 gates)."""
        x = self._var(x)
        y = self.inv_or_zero(x)
        b = self._emit([x, y, self.zero, self.zero], {"q_mul0": -1, "q_c": 1})
        self._emit([x, b, self.zero, self.zero], {"q_mul0": 1}, out=self.zero)
        return b

    def is_equal(self, a, b):
        """1 if a = b else 0"""
        return self.is_zero(self.sub(a, b))

    def select(self, c, a, b):
        """b + c (a - b): a where c = 1, b where c = 0.  The caller makes c boolean."""
        c, a, b = self._var(c), self._var(a), self._var(b)
        return self._emit([c, a, c, b], {"q_mul0": 1, "q_mul1": -1, "q_lc3": 1})

    def less_than(self, a, b, nbits: int):
        """1 if a < b else 0, for a, b < 2^nbits (both range-checked here), nbits in 1 .. bit_length(r) - 2: a - b + 2^nbits lies in
        (0, 2^(nbits+1)), and its bit `nbits` is set exactly when a >= b."""
        nbits = self._nbits(nbits, self.field.p.bit_length() - 2)
        a, b = self._var(a), self._var(b)
        lens = {w.shape[0] for w in (a, b) if w.ndim}
        if len(lens - {1}) > 1:
            raise ValueError(f"mismatched lengths {sorted(lens)}: array arguments must have one length (or length 1)")
        self.range_check(a, nbits)
        self.range_check(b, nbits)
        d = self.lc([a, b], [1, -1], const=1 << nbits)
        top = self.to_bits(d, nbits + 1)[nbits]
        return self.lc([top], [-1], const=1)

    # ------------------------------------------------------------------ Rescue (rescue.py: the same function on the device)
    def _rescue_params(self, params):
        from .rescue import RescueParams
        if params is None:
            return RescueParams.default(self.curve)
        if not isinstance(params, RescueParams) or params.curve != self.curve:
            raise ValueError(f"params: a rescue.RescueParams over {self.curve}")
        return params

    def _same_length(self, ids) -> list:
        """ids checked and, if any of them is an array, all broadcast to that length (so that each emits one gate per instance)"""
        vs = [self._var(v) for v in ids]
        lens = sorted({v.shape[0] for v in vs if v.ndim})
        k = max(lens, default=1)
        if any(l not in (1, k) for l in lens):
            raise ValueError(f"mismatched lengths {lens}: array arguments must have one length (or length 1)")
        return [np.broadcast_to(v, (k,)) for v in vs] if lens else vs

    def rescue_permutation(self, state4, params=None):
        """The Rescue permutation of the state (s0, s1, s2, s3) -> its four output variables.  Per instance 4 lc gates for s + K[0], then per
        round 4 root5 (the inverse S-boxes, hinted), 4 lc gates M y + K[2i+1] and 4 pow5_lc gates M (.)^5 + K[2i+2]: 148 gates, 37 levels."""
        state4 = list(state4)
        if len(state4) != 4:
            raise ValueError(f"a state of {len(state4)} elements: Rescue's width is 4")
        prm = self._rescue_params(params)
        M, K = prm.mds, prm.round_keys
        s = self._same_length(state4)
        s = [self.lc([s[i]], [1], const=K[0][i]) for i in range(4)]
        for rnd in range(len(K) // 2):
            y = [self.root5(x) for x in s]
            s = [self.lc(y, M[i], const=K[2 * rnd + 1][i]) for i in range(4)]
            s = [self.pow5_lc(s, M[i], const=K[2 * rnd + 2][i]) for i in range(4)]
        return s

    def rescue_hash2(self, l, r, params=None):
        """hash2(l, r) = rescue_permutation((l, r, 0, 0))[0]"""
        return self.rescue_permutation([l, r, self.zero, self.zero], params)[0]

    def merkle_root(self, leaf, index_bits, siblings, params=None):
        """The root of the Merkle path from `leaf` up: siblings[j] is the other child at depth j (from the leaf), index_bits[j] = 1 where the
        node on the path is the RIGHT child — rescue.MerkleTree.path's order.  Per depth: enforce_bool(bit), left = select(bit, sib, cur),
        right = select(bit, cur, sib), cur = rescue_hash2(left, right).  -> the root variable(s); the caller equates it with the public root."""
        index_bits, siblings = list(index_bits), list(siblings)
        if len(index_bits) != len(siblings):
            raise ValueError(f"mismatched lengths: {len(index_bits)} index bits, {len(siblings)} siblings")
        prm = self._rescue_params(params)
        self._same_length([leaf] + index_bits + siblings)
        cur = leaf
        for bit, sib in zip(index_bits, siblings):
            self.enforce_bool(bit)
            left, right = self.select(bit, sib, cur), self.select(bit, cur, sib)
            cur = self.rescue_hash2(left, right, prm)
        return cur

    def rescue_hash3(self, a, b, c, params=None):
        """hash3(a, b, c) = rescue_permutation((a, b, c, 0))[0]"""
        return self.rescue_permutation([a, b, c, self.zero], params)[0]

    def accumulator_root(self, uid, elem, sib1s, sib2s, is_lefts, is_rights, params=None):
        """The root of the path of leaf (uid, elem) through a ternary accumulator (rescue.Accumulator; jellyfish's compute_merkle_root):
        cur = rescue_hash3(zero, uid, elem), then per level j, from the leaves up, with the two other members sib1s[j], sib2s[j] of the group
        in ascending position and the flags is_lefts[j], is_rights[j] (cur is the left / the right member; neither: the middle one):
            enforce_bool(is_left), enforce_bool(is_right), enforce_bool(is_left + is_right)
            l = select(is_left, cur, sib1),  r = select(is_right, cur, sib2),  mid = cur + sib1 + sib2 - l - r,  cur = rescue_hash3(l, mid, r)
        — 148 + 8 gates per level after the 148 of the leaf.  The flags are NOT tied to uid, exactly as in jellyfish: the circuit proves that
        SOME position sequence leads from the leaf hash, which contains uid, to the root.  -> the root variable(s); the caller equates it
        with the public root."""
        lists = [list(x) for x in (sib1s, sib2s, is_lefts, is_rights)]
        if len({len(x) for x in lists}) != 1:
            raise ValueError(f"mismatched lengths: {', '.join(str(len(x)) for x in lists)} sib1s, sib2s, is_lefts, is_rights")
        prm = self._rescue_params(params)
        self._same_length([uid, elem] + [v for x in lists for v in x])
        cur = self.rescue_hash3(self.zero, uid, elem, prm)
        for sib1, sib2, is_left, is_right in zip(*lists):
            self.enforce_bool(is_left)
            self.enforce_bool(is_right)
            self.enforce_bool(self.add(is_left, is_right))
            l, r = self.select(is_left, cur, sib1), self.select(is_right, cur, sib2)
            mid = self.sub(self.lc([cur, sib1, sib2, l], [1, 1, 1, -1]), r)
            cur = self.rescue_hash3(l, mid, r, prm)
        return cur

    def rescue_sponge(self, inputs, n_out: int = 1, params=None):
        """sponge(x_0 .. x_{L-1}; n_out) of rescue.py, the variable-length hash: s = (0, 0, 0, L), then per block of three s[j] += x[3b + j]
        and s = rescue_permutation(s); -> the LIST of the n_out first state variables after the last block, n_out in (1, 2, 3).  The first
        block goes straight into rescue_permutation([x0, x1, x2, constant(L)]) with zero for absent elements; each later block is up to three
        add gates and one permutation: 148 ceil(L / 3) + max(L - 3, 0) gates per instance (and at most one for the constant L), in
        37 + 38 (ceil(L / 3) - 1) levels.  The length in the capacity separates (a) from (a, 0); rescue_sponge([a, b, c])[0] is
        permute((a, b, c, 3))[0] and NOT rescue_hash3(a, b, c) = permute((a, b, c, 0))[0], by design."""
        inputs = list(inputs)
        L = len(inputs)
        if not 1 <= L < 1 << 32:
            raise ValueError(f"rescue_sponge: L = {L} inputs (1 .. 2^32 - 1)")
        if n_out not in (1, 2, 3):
            raise ValueError(f"rescue_sponge: n_out = {n_out!r} (1, 2 or 3)")
        prm = self._rescue_params(params)
        x = self._same_length(inputs)
        s = self.rescue_permutation([x[j] if j < L else self.zero for j in range(3)] + [self.constant(L)], prm)
        for b in range(1, (L + 2) // 3):
            s = [self.add(s[j], x[3 * b + j]) if 3 * b + j < L else s[j] for j in range(3)] + [s[3]]
            s = self.rescue_permutation(s, prm)
        return s[:n_out]

    def rescue_stream(self, key, nblocks: int, params=None):
        """The keystream of rescue.py's counter mode under the variable `key`: -> a list of nblocks triples, block j being the three first
        variables of rescue_permutation([key, constant(j), zero, constant(-1)]).  148 gates per block and instance (and the constants), every
        block at the same depth: 37 levels.  Element i of a text takes block i div 3, position i mod 3."""
        if not isinstance(nblocks, _SCALARS) or not 1 <= int(nblocks) < 1 << 32:
            raise ValueError(f"rescue_stream: nblocks = {nblocks!r} (1 .. 2^32 - 1)")
        prm = self._rescue_params(params)
        key = self._var(key)
        minus_one = self.constant(-1)
        return [tuple(self.rescue_permutation([key, self.constant(j), self.zero, minus_one], prm)[:3]) for j in range(int(nblocks))]

    # ------------------------------------------------------------------ the embedded Edwards curve (edwards.py: the same group on the device)
    # A point is a pair (x_ids, y_ids).  E: a x^2 + y^2 = 1 + d x^2 y^2 with a a square and d a non-square, so for points ON E no denominator
    # below is zero and one formula serves P + Q, P + P, P - P, the identity (0, 1) and the points of small order.  The gadgets are gates the
    # builder already has (mul, mul_add, lc, div): no selector of their own.  The quotients are div gates, checked by y * b = a: a zero
    # denominator — possible only for a point off E — leaves the circuit unsatisfied unless the numerator vanishes too, so a gadget's
    # points must be on E: a constant, enforce_on_curve'd, checked outside the circuit (a public key), or the output of a gadget.
    def _edwards_params(self, prm):
        from .edwards import EdwardsParams
        if prm is None:
            return EdwardsParams.default(self.curve)
        if not isinstance(prm, EdwardsParams) or prm.curve != self.curve:
            raise ValueError(f"prm: an edwards.EdwardsParams over {self.curve}")
        return prm

    def _points(self, points, others=()):
        """pairs checked, and every id of `points` and `others` broadcast to one length -> (list of (x, y), list of the others)"""
        flat = []
        for p in points:
            if not isinstance(p, (tuple, list)) or len(p) != 2:
                raise ValueError("a point is a pair (x_ids, y_ids)")
            flat += [p[0], p[1]]
        vs = self._same_length(flat + list(others))
        k = len(points)
        return [(vs[2 * i], vs[2 * i + 1]) for i in range(k)], vs[2 * k:]

    def point_constant(self, x: int, y: int, prm=None):
        """The constant point (x, y) of E as a pair of constant variables (at most 2 gates, shared with equal constants)."""
        prm = self._edwards_params(prm)
        p = self.field.p
        x, y = int(x) % p, int(y) % p
        if (prm.a * x * x + y * y - 1 - prm.d * x * x * y * y) % p:
            raise ValueError("point_constant: not on the curve")
        return self.constant(x), self.constant(y)

    def point_add(self, p, q, prm=None):
        """p + q by the complete law: x3 = (x1 y2 + y1 x2) / (1 + d t), y3 = (y1 y2 - a x1 x2) / (1 - d t), t = x1 x2 y1 y2.  Per instance
        9 gates (mul_add, three mul, three lc, two div) in 4 levels."""
        prm = self._edwards_params(prm)
        ((x1, y1), (x2, y2)), _ = self._points([p, q])
        nx = self.mul_add(x1, y2, y1, x2)
        xx, yy = self.mul(x1, x2), self.mul(y1, y2)
        t = self.mul(xx, yy)
        ny = self.lc([yy, xx], [1, -prm.a])
        dx, dy = self.lc([t], [prm.d], const=1), self.lc([t], [-prm.d], const=1)
        return self.div(nx, dx), self.div(ny, dy)

    def point_double(self, p, prm=None):
        """2 p for p ON E, where t = x^2 y^2 need not be formed: x3 = 2 x y / (a x^2 + y^2), y3 = (y^2 - a x^2) / (2 - a x^2 - y^2).  Per
        instance 8 gates (three mul, three lc, two div) in 3 levels.  (point_add(p, p) is the law itself and asks nothing of p.)"""
        prm = self._edwards_params(prm)
        ((x, y),), _ = self._points([p])
        xy2 = self._emit([x, y, self.zero, self.zero], {"q_mul0": 2})
        xx, yy = self.mul(x, x), self.mul(y, y)
        dx, ny = self.lc([xx, yy], [prm.a, 1]), self.lc([yy, xx], [1, -prm.a])
        dy = self.lc([xx, yy], [-prm.a, -1], const=2)
        return self.div(xy2, dx), self.div(ny, dy)

    def point_neg(self, p):
        """-(x, y) = (-x, y): one lc gate."""
        ((x, y),), _ = self._points([p])
        return self.lc([x], [-1]), y

    def point_select(self, bit, p, q):
        """p where bit = 1, q where bit = 0: two select gates, 1 level.  The caller makes bit boolean."""
        ((px, py), (qx, qy)), (bit,) = self._points([p, q], [bit])
        return self.select(bit, px, qx), self.select(bit, py, qy)

    def enforce_on_curve(self, p, prm=None):
        """a x^2 + y^2 = 1 + d x^2 y^2: two mul gates and one constraint gate."""
        prm = self._edwards_params(prm)
        ((x, y),), _ = self._points([p])
        xx, yy = self.mul(x, x), self.mul(y, y)
        self._emit([xx, yy, self.zero, self.zero], {"q_lc0": prm.a, "q_lc1": 1, "q_mul0": -prm.d, "q_c": -1, "q_o": 0}, out=self.zero)

    def enforce_point_equal(self, p, q):
        """two enforce_equal gates"""
        ((px, py), (qx, qy)), _ = self._points([p, q])
        self.enforce_equal(px, qx)
        self.enforce_equal(py, qy)

    def to_bits_strict(self, x):
        """ALL bit_length(r) bits of the canonical residue of x, LSB first: the bit gates and the recomposition of to_bits, which at this
        width holds for x and for x + r alike, and the comparison that excludes the latter — the bits read as an integer are <= r - 1.
        From the top bit down `run` = [every bit so far that is set in r - 1 is set]: run <- run * bit at a set bit of r - 1 (a mul gate),
        run * bit = 0 enforced at a clear one.  Per element L + 1 + ceil((L - 4) / 3) + (L - 1) gates for L = bit_length(r) (r - 1 ends in
        zeros on both fields): 592 on bn254, 594 on bls12_381; the run is a chain of popcount(r - 1) levels."""
        p = self.field.p
        L = p.bit_length()
        x = self._var(x)
        bits = self._recompose([self.bit(x, k) for k in range(L)], x)
        c = p - 1
        lowest_clear = next(i for i in range(L) if not (c >> i) & 1)
        run = bits[L - 1]
        for i in range(L - 2, lowest_clear - 1, -1):
            if (c >> i) & 1:
                run = self.mul(run, bits[i])
            else:
                self._emit([run, bits[i], self.zero, self.zero], {"q_mul0": 1, "q_o": 0}, out=self.zero)
        return bits

    def _point_or_identity(self, bit, p):
        """p where bit = 1, (0, 1) where bit = 0: (bit x, 1 + bit (y - 1)), 2 gates"""
        x, y = p
        return self.mul(bit, x), self._emit([bit, y, self.zero, self.zero], {"q_mul0": 1, "q_lc0": -1, "q_c": 1})

    def scalar_mul(self, bits, p, prm=None):
        """[sum 2^i bits[i]] p for p ON E; bits: a list of boolean variables, LSB first, as to_bits and to_bits_strict return them.  Per
        bit the addend (p_i where the bit is set, else the identity: 2 gates), its addition to the sum (point_add: 9) and p_{i+1} = 2 p_i
        (point_double: 8); the first bit needs no addition and the last no doubling: 19 nbits - 17 gates per instance.  The doublings do
        not wait for the sum, so the depth is that of the additions: 4 nbits levels."""
        prm = self._edwards_params(prm)
        bits = list(bits)
        if not bits:
            raise ValueError("scalar_mul: no bits")
        (base,), bits = self._points([p], bits)
        acc = None
        for i, bit in enumerate(bits):
            q = self._point_or_identity(bit, base)
            acc = q if acc is None else self.point_add(acc, q, prm)
            if i + 1 < len(bits):
                base = self.point_double(base, prm)
        return acc

    def fixed_base_mul(self, bits, prm=None):
        """[sum 2^i bits[i]] G for the generator of prm; bits as in scalar_mul.  The multiples C_i = 2^i G are constants, and adding
        (C_i where the bit is set, else the identity) = (cx b, 1 + (cy - 1) b) to (x, y) has, with b^2 = b, numerators and denominators of
        degree two: x + (cy - 1) b x + cx b y,  y + (cy - 1) b y - a cx b x,  1 +- d cx cy b (x y) — 7 gates per bit (two numerators, x y,
        two denominators, two div) in 3 levels, no select; the first bit is two lc gates: 7 nbits - 5 gates per instance."""
        prm = self._edwards_params(prm)
        bits = list(bits)
        if not bits:
            raise ValueError("fixed_base_mul: no bits")
        bits = self._same_length(bits)
        z, a, d = self.zero, prm.a, prm.d
        cx, cy = prm.generator
        x, y = self.lc([bits[0]], [cx]), self.lc([bits[0]], [cy - 1], const=1)
        for bit in bits[1:]:
            cx, cy = prm.add_int((cx, cy), (cx, cy))
            nx = self._emit([bit, x, bit, y], {"q_mul0": cy - 1, "q_mul1": cx, "q_lc1": 1})
            ny = self._emit([bit, y, bit, x], {"q_mul0": cy - 1, "q_mul1": -a * cx, "q_lc1": 1})
            xy = self.mul(x, y)
            dx = self._emit([bit, xy, z, z], {"q_mul0": d * cx * cy, "q_c": 1})
            dy = self._emit([bit, xy, z, z], {"q_mul0": -d * cx * cy, "q_c": 1})
            x, y = self.div(nx, dx), self.div(ny, dy)
        return x, y

    def schnorr_verify(self, pk, message, R, s, prm=None, rescue=None):
        """The signature (R, s) of edwards.schnorr_sign on `message` under pk:  [s] G = R + [c] pk  with  c = hash3(hash3(R.x, R.y, pk.x),
        pk.y, message).  s: a variable (decomposed here with to_bits to bit_length(l) bits), or a LIST of that many bit variables, LSB
        first (made boolean here).  enforce_on_curve(R), the two rescue_hash3, to_bits_strict(c) — c multiplies pk as the integer in
        [0, r) that the device's kernel takes it for —, fixed_base_mul, scalar_mul, point_add, enforce_point_equal: 7798 gates per
        signature on bn254, 7827 on bls12_381 with the default parameters (n = 2^13 for one signature).
        NOT proved: that pk is on E and in the subgroup of order l — pk is public, check it outside with edwards.in_subgroup, as the
        doublings of scalar_mul assume pk on E; that R lies in that subgroup (the cofactor is 8: R may carry a component of small order,
        which the equation then forces onto [c] pk — impossible for pk in the subgroup, so R is in it whenever pk is); that s < l (any
        s < 2^bit_length(l) with the same residue mod l is accepted: edwards.schnorr_verify refuses s >= l)."""
        prm, rp = self._edwards_params(prm), self._rescue_params(rescue)
        lbits = prm.order.bit_length()
        s_is_bits = isinstance(s, (list, tuple))
        if s_is_bits and len(s) != lbits:
            raise ValueError(f"s: {len(s)} bits, the order has {lbits}")
        self._nbits(lbits, self.field.p.bit_length() - 1)
        (pk, R), rest = self._points([pk, R], [message] + (list(s) if s_is_bits else [s]))
        message, s = rest[0], rest[1:]
        self.enforce_on_curve(R, prm)
        if s_is_bits:
            s_bits = list(s)
            for b in s_bits:
                self.enforce_bool(b)
        else:
            s_bits = self.to_bits(s[0], lbits)
        c = self.rescue_hash3(self.rescue_hash3(R[0], R[1], pk[0], rp), pk[1], message, rp)
        c_bits = self.to_bits_strict(c)
        lhs = self.fixed_base_mul(s_bits, prm)
        rhs = self.point_add(R, self.scalar_mul(c_bits, pk, prm), prm)
        self.enforce_point_equal(lhs, rhs)

    def elgamal_encrypt(self, ek, msg, r, prm=None, rescue=None):
        """The ciphertext of elgamal.encrypt on the message variables `msg` (a list of L >= 1) under the key point ek with the randomness r:
        E = [r] G, S = [r] ek, k = hash3(S.x, S.y, 0), ct_i = msg_i + ks_{i div 3}[i mod 3] with the keystream of rescue_stream under k.
        -> (E, ct): the point E and the list of the L ciphertext variables; the caller equates them with the public ciphertext.  r: a
        variable (decomposed here with to_bits to bit_length(l) bits), or a LIST of that many bit variables, LSB first (made boolean here),
        as schnorr_verify takes s.  to_bits, fixed_base_mul, scalar_mul, rescue_hash3, rescue_stream over ceil(L / 3) blocks and L add
        gates: 6987 + 148 ceil(L / 3) + L gates per instance on bn254, 7014 + ... on bls12_381 with the default parameters (and the
        constants of the stream), in 4 bit_length(l) + 75 levels.
        NOT proved: that ek is on E and in the subgroup of order l — ek is public, check it outside with edwards.in_subgroup, as the
        doublings of scalar_mul assume ek on E; that r < l — any r below 2^bit_length(l) is accepted (elgamal.encrypt refuses r >= l).
        The SAME bits of r serve both multiplications, which is the point: E and the key belong to one r."""
        prm, rp = self._edwards_params(prm), self._rescue_params(rescue)
        msg = list(msg)
        L = len(msg)
        if not 1 <= L < 1 << 32:
            raise ValueError(f"elgamal_encrypt: a message of {L} elements (at least 1)")
        lbits = prm.order.bit_length()
        r_is_bits = isinstance(r, (list, tuple))
        if r_is_bits and len(r) != lbits:
            raise ValueError(f"r: {len(r)} bits, the order has {lbits}")
        self._nbits(lbits, self.field.p.bit_length() - 1)
        (ek,), rest = self._points([ek], msg + (list(r) if r_is_bits else [r]))
        msg, r = rest[:L], rest[L:]
        if r_is_bits:
            bits = list(r)
            for b in bits:
                self.enforce_bool(b)
        else:
            bits = self.to_bits(r[0], lbits)
        E = self.fixed_base_mul(bits, prm)
        S = self.scalar_mul(bits, ek, prm)
        k = self.rescue_hash3(S[0], S[1], self.zero, rp)
        ks = self.rescue_stream(k, (L + 2) // 3, rp)
        return E, [self.add(msg[i], ks[i // 3][i % 3]) for i in range(L)]

    # ------------------------------------------------------------------ constraints
    def enforce_equal(self, a, b):
        self._emit([a, b, self.zero, self.zero], {"q_lc0": 1, "q_lc1": -1, "q_o": 0}, out=self.zero)

    def enforce_constant(self, a, c):
        z = self.zero
        self._emit([z, z, z, z], {"q_c": c}, out=a)

    def enforce_bool(self, a):
        self._emit([a, a, self.zero, self.zero], {"q_mul0": 1}, out=a)

    def enforce_mul(self, a, b, c):
        self._emit([a, b, self.zero, self.zero], {"q_mul0": 1}, out=c)

    # ------------------------------------------------------------------ build
    def _limbs(self, values) -> np.ndarray:
        p, R = self.field.p, self.field.R
        raw = b"".join((v * R % p).to_bytes(32, "little") for v in values)
        return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4)

    def build(self) -> BuiltCircuit:
        chunks = [c for c in self._chunks if c[3]] + [c for c in self._chunks if not c[3]]
        g = sum(c[0].shape[1] for c in chunks)
        n = max(2, 1 << (g - 1).bit_length())
        wire_vars = np.full((NUM_WIRE_TYPES, n), self.zero, dtype=np.uint32)
        sel = np.zeros((NUM_SELECTORS, n, 4), dtype=np.uint64)
        def_gate = np.full(self.num_vars, GIVEN, dtype=np.uint32)
        hint_op = np.zeros(n, dtype=np.uint32)
        scalar_limbs = {}
        at = 0
        for wv, s, defines, _, *hint in chunks:
            k = wv.shape[1]
            if hint:
                hint_op[at:at + k] = hint[0]
            wire_vars[:, at:at + k] = wv
            for t, v in s.items():
                if isinstance(v, list):
                    sel[t, at:at + k] = self._limbs(v)
                else:
                    if v not in scalar_limbs:
                        scalar_limbs[v] = self.field.to_limbs(v)
                    sel[t, at:at + k] = scalar_limbs[v]
            if defines:
                def_gate[wv[4]] = np.arange(at, at + k, dtype=np.uint32)
            at += k
        cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
        pub = cat([np.atleast_1d(np.asarray(p)) for p in self._publics])
        return BuiltCircuit(self.curve, wire_vars, sel, self.num_vars, def_gate, cat(self._inputs), pub, int(self.zero), g, hint_op=hint_op)
