"""tests/solve_ref.py's sequential big-integer solver extended with hinted definitions (a helper of the hint tests, not a test).

A gate g with a non-zero opcode in built.hint_op[g] (bits 0-7; bits 8-31 an argument) defines the variable on its wire 4 from the values
s0 on wire 2 and s1 on wire 3, evaluated here with Python's pow and bit operations on canonical residues:
    1 INV    s0^-1, 0 for s0 = 0            2 DIV    s0 * s1^-1, 0 for s1 = 0
    3 ROOT5  s0^d, d = 5^-1 mod (r - 1)     4 BIT    bit `arg` of s0
Its live wires are its sources alone (wire 2; wire 3 too for DIV), whatever its selectors say, and its level follows from them as for
any other gate.  No selector of a hint gate is read for its value; unsatisfied_gates (inherited) checks every gate's equation."""
from tests.solve_ref import GIVEN, Cycle, RefSolver  # noqa: F401  (re-exported for the tests)

INV, DIV, ROOT5, BIT = 1, 2, 3, 4


class HintRefSolver(RefSolver):
    def __init__(self, built, inputs=None, public_inputs=(), given=None):
        super().__init__(built, inputs, public_inputs, given)
        self.hint_op = [int(h) for h in built.hint_op]
        self.root5_exp = pow(5, -1, self.f.p - 1)

    def opcode(self, g: int) -> int:
        return self.hint_op[g] & 0xFF

    def live_wires(self, g: int):
        op = self.opcode(g)
        if op == 0:
            return super().live_wires(g)
        return [2, 3] if op == DIV else [2]

    def hint_value(self, g: int, s0: int, s1: int) -> int:
        op, arg, p = self.opcode(g), self.hint_op[g] >> 8, self.f.p
        if op == INV:
            return pow(s0, -1, p) if s0 else 0
        if op == DIV:
            return s0 * pow(s1, -1, p) % p if s1 else 0
        if op == ROOT5:
            return pow(s0, self.root5_exp, p)
        assert op == BIT and arg < 256, f"gate {g}: hint_op {self.hint_op[g]:#x}"
        return (s0 >> arg) & 1

    def value(self, v: int) -> int:
        """RefSolver.value with hint gates: the same explicit-stack walk over live_wires"""
        wv, dg, p = self.b.wire_vars, self.b.def_gate, self.f.p
        stack, expanded = [int(v)], set()
        while stack:
            u = stack[-1]
            if u in self.val:
                stack.pop()
                continue
            g = int(dg[u])
            if g == GIVEN:
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
            if self.opcode(g):
                self.val[u] = self.hint_value(g, self.val[int(wv[2, g])], self.val[int(wv[3, g])] if 3 in live else 0)
            else:
                q = self.selectors(g)
                assert q[10] != 0 and q[12] == 0
                w = [self.val[int(wv[i, g])] if i in live else 0 for i in range(4)]
                self.val[u] = self.inputs_value(g, w) * pow(q[10], -1, p) % p
            self.lvl[u] = 1 + max([self.lvl[int(wv[i, g])] for i in live], default=-1)
            expanded.discard(u)
            stack.pop()
        return self.val[int(v)]
