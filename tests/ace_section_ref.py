"""The rule of the ACE chiplet's trace section (include/midenhip.h mh_ace_section_build; processor/src/trace/chiplets/ace/{mod,trace,
instruction}.rs, processor/src/execution/operations/eval_circuit.rs:54-118), restated on Python integers: 16 columns, per evaluation
n_read READ rows and num_eval EVAL rows, wire ids descending from nw - 1 in insertion order, every wire's fan-out as a multiplicity,
products in F_p[x]/(x^2 - 7), the last wire zero.  Also the device schedule's round count (n_rounds), which is a function of the
circuits alone, and helpers that build circuits which evaluate to zero."""
import numpy as np

P = 0xFFFFFFFF00000001
DT = np.dtype([("ctx", "<u4"), ("ptr", "<u4"), ("clk", "<u4"), ("num_vars", "<u4"), ("num_eval", "<u4"), ("reserved", "<u4"), ("payload", "<u8")])
WIDTH = 16
SUB, MUL, ADD = 0, 1, 2
MAX_WIRES = (1 << 30) - 1
WINDOW = 64


class Defect(Exception):
    def __init__(self, kind, index, gate=0):
        super().__init__(f"defect {kind} at evaluation {index}, gate {gate}")
        self.kind, self.index, self.gate = kind, index, gate


def min_log_n(rows):
    return max(6, (rows - 1).bit_length()) if rows else 6


def qmul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def apply(op, x, y):
    if op == SUB:
        return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
    if op == MUL:
        return qmul(x, y)
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def encode(id_l, id_r, op):
    return id_l | (id_r << 30) | (op << 60)


def decode(felt):
    ins = int(felt) % P
    return ins & MAX_WIRES, (ins >> 30) & MAX_WIRES, ins >> 60


def header_defect(evals, e, n_felts):
    """The first of kinds 1, 2, 3 that evaluation e carries, or 0."""
    h = evals[e]
    nv, ne = int(h["num_vars"]), int(h["num_eval"])
    if nv == 0 or nv % 2 or ne == 0 or ne % 4 or nv + ne > MAX_WIRES:
        return 1
    if e and int(h["clk"]) <= int(evals[e - 1]["clk"]):
        return 2
    need = 2 * nv + ne
    if int(h["payload"]) > n_felts or need > n_felts - int(h["payload"]) or int(h["ptr"]) + need > 1 << 32:
        return 3
    return 0


def gate_defect(h, felts):
    """The lowest gate of a well-formed evaluation whose opcode is above 2 or that names a wire not yet inserted, or None."""
    nv, ne = int(h["num_vars"]), int(h["num_eval"])
    nw, base = nv + ne, int(h["payload"]) + 2 * nv
    for k in range(ne):
        id_l, id_r, op = decode(felts[base + k])
        if op > 2 or id_l >= nw or id_r >= nw or nw - 1 - id_l >= nv + k or nw - 1 - id_r >= nv + k:
            return k
    return None


def rounds(positions, n_read2):
    """The rounds of the window schedule for gates whose operand positions are `positions` [(pos_l, pos_r)]: 64 gates a window; in a
    round every pending gate computes whose operands lie before the window or belong to a gate of the window finished in an EARLIER
    round."""
    total = 0
    for base in range(0, len(positions), WINDOW):
        first = n_read2 + base
        done_round = {}
        for j, (pl, pr) in enumerate(positions[base:base + WINDOW]):
            need = [done_round[p - first] for p in (pl, pr) if p >= first]
            done_round[j] = 1 + max(need, default=0)
        total += max(done_round.values())
    return total


def evaluate(h, felts):
    """One well-formed evaluation -> (rows [n_read + num_eval, 16], last wire value, rounds)."""
    ctx, ptr, clk, nv, ne = (int(h[f]) for f in ("ctx", "ptr", "clk", "num_vars", "num_eval"))
    n_read, nw, at = nv // 2, nv + ne, int(h["payload"])
    values, mult = [], [0] * nw
    for i in range(nv):
        values.append((int(felts[at + 2 * i]) % P, int(felts[at + 2 * i + 1]) % P))
    gates = []
    for k in range(ne):
        id_l, id_r, op = decode(felts[at + 2 * nv + k])
        pl, pr = nw - 1 - id_l, nw - 1 - id_r
        mult[pl] += 1
        mult[pr] += 1
        values.append(apply(op, values[pl], values[pr]))
        gates.append((op, pl, pr))
    rows = np.zeros((n_read + ne, WIDTH), dtype=np.uint64)
    for i in range(n_read):
        v0, v1 = values[2 * i], values[2 * i + 1]
        rows[i] = [1 if i == 0 else 0, 0, ctx, ptr + 4 * i, clk, 0, nw - 1 - 2 * i, v0[0], v0[1], nw - 2 - 2 * i, v1[0], v1[1], ne - 1, 0,
                   mult[2 * i + 1], mult[2 * i]]
    for k, (op, pl, pr) in enumerate(gates):
        v0, vl, vr = values[nv + k], values[pl], values[pr]
        rows[n_read + k] = [0, 1, ctx, ptr + 4 * n_read + k, clk, {SUB: P - 1, MUL: 0, ADD: 1}[op], ne - 1 - k, v0[0], v0[1], nw - 1 - pl, vl[0],
                            vl[1], nw - 1 - pr, vr[0], vr[1], mult[nv + k]]
    return rows, values[-1], rounds([(pl, pr) for _, pl, pr in gates], nv)


def section(evals, felts, cap_rows=None):
    """-> (rows uint64 [n_rows, 16], info dict n_rows, n_wires, n_gates, n_rounds).  Defects: the lowest evaluation that carries one of
    kinds 1..4 (each evaluation carries the first it has), then kind 5 (index = the first evaluation without its rows), then kind 6 for
    the lowest evaluation whose last wire is not zero."""
    evals = np.asarray(evals, dtype=DT).reshape(-1) if len(evals) else np.zeros(0, dtype=DT)
    felts = np.asarray(felts, dtype=np.uint64).reshape(-1)
    for e in range(len(evals)):
        kind = header_defect(evals, e, len(felts))
        if kind:
            raise Defect(kind, e)
        gate = gate_defect(evals[e], felts)
        if gate is not None:
            raise Defect(4, e, gate)
    at = 0
    for e, h in enumerate(evals):
        at += int(h["num_vars"]) // 2 + int(h["num_eval"])
        if cap_rows is not None and at > cap_rows:
            raise Defect(5, e)
    out, n_rounds, nonzero = [], 0, None
    for e, h in enumerate(evals):
        rows, last, r = evaluate(h, felts)
        out.append(rows)
        n_rounds += r
        if last != (0, 0) and nonzero is None:
            nonzero = e
    if nonzero is not None:
        raise Defect(6, nonzero)
    rows = np.concatenate(out) if out else np.zeros((0, WIDTH), dtype=np.uint64)
    n_wires = sum(int(h["num_vars"]) + int(h["num_eval"]) for h in evals)
    n_gates = sum(int(h["num_eval"]) for h in evals)
    return rows, dict(n_rows=rows.shape[0], n_wires=n_wires, n_gates=n_gates, n_rounds=n_rounds)


# ---- building lists ----
class Circuit:
    """One evaluation under construction.  `inputs`: the quadratic-extension values of the READ wires (an even number after close());
    gates name wires by POSITION (insertion order: inputs first, then gates), which encode() turns into descending ids at the end."""

    def __init__(self, inputs):
        self.inputs = [(int(a), int(b)) for a, b in inputs]
        self.gates = []   # (op, pos_l, pos_r) with gate positions counted from 0 = the first gate, as ('g', k), or inputs as ('i', k)

    def gate(self, op, left, right):
        self.gates.append((op, left, right))
        return ("g", len(self.gates) - 1)

    def _values(self, inputs):
        vals = []
        for op, l, r in self.gates:
            x = inputs[l[1]] if l[0] == "i" else vals[l[1]]
            y = inputs[r[1]] if r[0] == "i" else vals[r[1]]
            vals.append(apply(op, (x[0] % P, x[1] % P), (y[0] % P, y[1] % P)))
        return vals

    def close(self, zero=True):
        """Pad the gates to a multiple of 4 minus 1 with copies (x + 0 needs a zero input: appended), then end with `last - c` where the
        input c is the value the circuit has reached (zero=True) or that value minus 1 (zero=False: the output is 1).  The inputs are
        padded to an even number.  -> self"""
        ins = list(self.inputs)
        zero_at = len(ins)
        ins.append((0, 0))
        c_at = len(ins)
        ins.append((0, 0))   # placeholder
        if len(ins) % 2:
            ins.append((0, 0))
        if not self.gates:
            self.gate(ADD, ("i", 0), ("i", zero_at))
        while (len(self.gates) + 1) % 4:
            self.gate(ADD, ("g", len(self.gates) - 1), ("i", zero_at))
        last = self._values(ins)[-1]
        ins[c_at] = last if zero else ((last[0] - 1) % P, last[1])
        self.gate(SUB, ("g", len(self.gates) - 1), ("i", c_at))
        self.inputs = ins
        return self

    def close_exact(self, zero=True):
        """End with `last - c` without changing the sizes: the LAST input becomes c (no gate may have read it), the gate count must be
        3 mod 4 and the input count even.  -> self"""
        assert len(self.inputs) % 2 == 0 and (len(self.gates) + 1) % 4 == 0 and self.gates
        c_at = len(self.inputs) - 1
        assert all(w != ("i", c_at) for _, l, r in self.gates for w in (l, r))
        last = self._values(self.inputs)[-1]
        self.inputs[c_at] = last if zero else ((last[0] - 1) % P, last[1])
        self.gate(SUB, ("g", len(self.gates) - 1), ("i", c_at))
        return self

    def emit(self):
        """-> (num_vars, num_eval, felts): 2 num_vars input felts, then the instructions."""
        nv, ne = len(self.inputs), len(self.gates)
        assert nv % 2 == 0 and ne % 4 == 0 and nv and ne
        nw = nv + ne
        pos = lambda w: w[1] if w[0] == "i" else nv + w[1]   # noqa: E731
        felts = [x for v in self.inputs for x in v]
        felts += [encode(nw - 1 - pos(l), nw - 1 - pos(r), op) for op, l, r in self.gates]
        return nv, ne, felts


def make_list(circuits, ctx=0, ptr=1 << 10, clk0=5):
    """Closed circuits -> (evals, felts): consecutive clocks, every evaluation at `ptr`."""
    evals, felts = np.zeros(len(circuits), dtype=DT), []
    for i, c in enumerate(circuits):
        nv, ne, f = c.emit()
        evals[i] = (ctx, ptr, clk0 + i, nv, ne, 0, len(felts))
        felts += f
    return evals, np.array(felts, dtype=np.uint64)


def random_circuit(rng, n_inputs, n_gates, zero=True, local=0.5):
    """A random circuit of about n_gates gates: operands are recent wires with probability `local`, any earlier wire otherwise."""
    inputs = [(int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(n_inputs)]
    c = Circuit(inputs)

    def pick(k):
        if k and rng.random() < local:
            return ("g", int(rng.integers(max(0, k - 4), k)))
        j = int(rng.integers(0, n_inputs + k))
        return ("i", j) if j < n_inputs else ("g", j - n_inputs)

    for k in range(n_gates):
        c.gate(int(rng.integers(0, 3)), pick(k), pick(k))
    return c.close(zero)


def sized_circuit(rng, num_vars, num_eval, zero=True, local=0.5, inputs=None):
    """A random circuit of exactly num_vars inputs and num_eval gates (the last input is the closing constant)."""
    if inputs is None:
        inputs = [(int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 64, dtype=np.uint64))) for _ in range(num_vars)]
    c = Circuit(inputs)
    free = max(1, num_vars - 1)   # inputs the gates may read

    def pick(k):
        if k and rng.random() < local:
            return ("g", int(rng.integers(max(0, k - 4), k)))
        j = int(rng.integers(0, free + k))
        return ("i", j) if j < free else ("g", j - free)

    for k in range(num_eval - 1):
        c.gate(int(rng.integers(0, 3)), pick(k), pick(k))
    return c.close_exact(zero)


def chain_circuit(rng, num_eval, num_vars=2):
    """Gate k reads gate k - 1 (and the first READ wire): num_eval rounds."""
    c = Circuit([(int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(num_vars)])
    c.gate(MUL, ("i", 0), ("i", 0))
    for k in range(1, num_eval - 1):
        c.gate((MUL, ADD, SUB)[k % 3], ("g", k - 1), ("i", 0) if k % 2 else ("g", k - 1))
    return c.close_exact()


def flat_circuit(rng, num_eval, num_vars=4):
    """Every gate reads READ wires only, the last one the same wire twice (x - x = 0): ceil(num_eval / 64) rounds."""
    c = Circuit([(int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(num_vars)])
    for k in range(num_eval - 1):
        c.gate(k % 3, ("i", int(rng.integers(0, num_vars))), ("i", int(rng.integers(0, num_vars))))
    c.gate(SUB, ("i", 1), ("i", 1))
    return c
