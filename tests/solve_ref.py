"""A sequential big-integer witness solver over the arrays of a builder.BuiltCircuit (a helper of the solver tests, not a test).

Written from the TurboPlonk gate equation
    q_c + PI + sum q_lc_i w_i + q_mul0 w0 w1 + q_mul1 w2 w3 + sum q_hash_i w_i^5 + q_ecc w0 w1 w2 w3 w4 - q_o w4 = 0
on Python ints mod r, demand-driven: the value of a variable is its defining gate's equation solved for wire 4, evaluated once the
variables on that gate's live wires (q_lc, q_hash or the wire's q_mul non-zero) are known — a depth-first walk with an explicit
stack, so one variable can be evaluated along its own chain without touching the rest of a 2^22-gate circuit.  The level of a
variable: -1 if given, else 1 + the largest level among the variables on its gate's live wires."""
import numpy as np

from distributed_plonk_amd import fr as _fr

GIVEN = 0xFFFFFFFF


class Cycle(Exception):
    def __init__(self, variable):
        super().__init__(f"variable {variable} depends on itself")
        self.variable = variable


class RefSolver:
    def __init__(self, built, inputs=None, public_inputs=(), given=None):
        """inputs / public_inputs: plain residues (Python ints), in the order of built.input_vars / built.public_vars; or, instead of
        `inputs`, given: {variable: residue} for the inputs that the variables to be evaluated depend on."""
        self.b = built
        self.f = _fr.FIELDS[built.curve]
        self.n = built.wire_vars.shape[1]
        self.pub = [int(x) % self.f.p for x in public_inputs]
        assert len(self.pub) == built.num_public
        if given is None:
            assert len(inputs) == len(built.input_vars)
            given = dict(zip(built.input_vars, inputs))
        self.partial = inputs is None
        self.val = {int(v): int(x) % self.f.p for v, x in given.items()}
        self.lvl = {v: -1 for v in self.val}
        self._sel = {}

    def selectors(self, g: int):
        """the 13 selectors of gate g as plain residues"""
        if g not in self._sel:
            f = self.f
            self._sel[g] = [int.from_bytes(self.b.selector_evals[t, g].tobytes(), "little") * f.R_inv % f.p for t in range(13)]
        return self._sel[g]

    def live_wires(self, g: int):
        q = self.selectors(g)
        return [i for i in range(4) if q[i] or q[6 + i] or q[4 + i // 2]]

    def pub_at(self, g: int) -> int:
        return self.pub[g] if g < len(self.pub) else 0

    def inputs_value(self, g: int, w) -> int:
        """q_c + PI + sum q_lc w + q_mul0 ab + q_mul1 cd + sum q_hash w^5 at gate g for the four input values w"""
        q, p = self.selectors(g), self.f.p
        acc = q[11] + self.pub_at(g) + q[4] * w[0] * w[1] + q[5] * w[2] * w[3]
        for i in range(4):
            acc += q[i] * w[i] + q[6 + i] * pow(w[i], 5, p)
        return acc % p

    def residual(self, g: int, w5) -> int:
        """the gate equation's left-hand side at gate g for its five wire values"""
        q, p = self.selectors(g), self.f.p
        return (self.inputs_value(g, w5[:4]) + q[12] * w5[0] * w5[1] * w5[2] * w5[3] * w5[4] - q[10] * w5[4]) % p

    def value(self, v: int) -> int:
        """the value of variable v, evaluating whatever it depends on first"""
        wv, dg, p = self.b.wire_vars, self.b.def_gate, self.f.p
        stack, expanded = [int(v)], set()
        while stack:
            u = stack[-1]
            if u in self.val:
                stack.pop()
                continue
            g = int(dg[u])
            if g == GIVEN:                              # a given variable without a value (none of the builder's): zero
                assert not self.partial, f"variable {u} is given, but `given` has no value for it"
                self.val[u], self.lvl[u] = 0, -1
                stack.pop()
                continue
            assert g < self.n and int(wv[4, g]) == u, f"def_gate[{u}] = {g} does not name a gate whose wire 4 reads it"
            live = self.live_wires(g)
            missing = [int(wv[i, g]) for i in live if int(wv[i, g]) not in self.val]
            if missing:
                if u in expanded or any(m in expanded for m in missing):
                    raise Cycle(min([u] + [m for m in missing if m in expanded]))
                expanded.add(u)
                stack.extend(missing)
                continue
            q = self.selectors(g)
            assert q[10] != 0 and q[12] == 0
            w = [self.val[int(wv[i, g])] if i in live else 0 for i in range(4)]
            self.val[u] = self.inputs_value(g, w) * pow(q[10], -1, p) % p
            self.lvl[u] = 1 + max([self.lvl[int(wv[i, g])] for i in live], default=-1)
            expanded.discard(u)
            stack.pop()
        return self.val[int(v)]

    def solve(self):
        """-> (witness as a list of plain residues, level per variable as a list)"""
        for v in range(self.b.num_vars):
            self.value(v)
        return [self.val[v] for v in range(self.b.num_vars)], [self.lvl[v] for v in range(self.b.num_vars)]

    def depth(self) -> int:
        """the number of dependency levels among the solved variables"""
        return 1 + max(self.lvl.values(), default=-1)

    def unsatisfied_gates(self, witness):
        """the gates whose equation does not hold under `witness` (plain residues per variable)"""
        wv = self.b.wire_vars
        return [g for g in range(self.n) if self.residual(g, [witness[int(wv[i, g])] for i in range(5)])]

    def limbs(self, values) -> np.ndarray:
        """plain residues -> (len, 4) Montgomery limbs"""
        f = self.f
        raw = b"".join((int(x) % f.p * f.R % f.p).to_bytes(32, "little") for x in values)
        return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()
