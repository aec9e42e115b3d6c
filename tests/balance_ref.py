"""The reference of the bus-balance tests: an independent evaluation of an "MHLKP001" lookup program over Python integers (one numpy
object array per node, so the walk is per node and not per cell), followed by the reference's HashMap walk
(air/src/lookup/debug/trace/mod.rs check_trace_balance): a dict from encoded denominator to net multiplicity plus the push list.
Nothing here calls the library."""
import numpy as np

P = 0xFFFFFFFF00000001
OP_CONST, OP_MAIN, OP_PERIODIC, OP_RANDOMNESS, OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_PREPROCESSED = 0, 1, 4, 8, 10, 11, 12, 13, 14


def parse_lookup(blob):
    w = [int(x) for x in blob]
    assert w[0] == 0x4d484c4b50303031, "not a lookup blob"
    k, periodic = 12, []
    for _ in range(w[6]):
        periodic.append(w[k + 1:k + 1 + w[k]])
        k += 1 + w[k]
    nodes = []
    for _ in range(w[8]):
        nodes.append((w[k] & 0xFF, (w[k] >> 8) & ((1 << 28) - 1), w[k] >> 36, w[k + 1]))
        k += 2
    cols = []
    for _ in range(w[2]):
        cnt = w[k]
        cols.append([(w[k + 1 + 2 * j], w[k + 2 + 2 * j]) for j in range(cnt)])
        k += 1 + 2 * cnt
    return periodic, nodes, cols


def fractions(blob, main, rnd, prep=None):
    """-> [(column, fraction, m0, m1, d0, d1)] in program order; m*, d*: object arrays [n] of canonical Python ints."""
    periodic, nodes, cols = parse_lookup(blob)
    n = main.shape[0]
    obj = lambda a: np.array([int(x) % P for x in a], dtype=object)   # noqa: E731
    zero = np.array([0] * n, dtype=object)
    rows = np.arange(n)
    val = []
    for op, a, b, c in nodes:
        if op == OP_CONST: v = (zero + c % P, zero)
        elif op == OP_MAIN: v = (np.roll(obj(main[:, a]), -b), zero)
        elif op == OP_PREPROCESSED: v = (np.roll(obj(prep[:, a]), -b), zero)
        elif op == OP_PERIODIC: v = (obj([periodic[a][r % len(periodic[a])] for r in rows]), zero)
        elif op == OP_RANDOMNESS: v = (zero + int(rnd[a][0]) % P, zero + int(rnd[a][1]) % P)
        elif op == OP_ADD: v = ((val[a][0] + val[b][0]) % P, (val[a][1] + val[b][1]) % P)
        elif op == OP_SUB: v = ((val[a][0] - val[b][0]) % P, (val[a][1] - val[b][1]) % P)
        elif op == OP_MUL: v = ((val[a][0] * val[b][0] + 7 * val[a][1] * val[b][1]) % P, (val[a][0] * val[b][1] + val[a][1] * val[b][0]) % P)
        elif op == OP_NEG: v = ((-val[a][0]) % P, (-val[a][1]) % P)
        else: raise AssertionError(op)
        val.append(v)
    return [(c, j, val[m][0], val[m][1], val[d][0], val[d][1]) for c, col in enumerate(cols) for j, (m, d) in enumerate(col)]


def main_reads(blob):
    """The main columns (current row) the program reads."""
    return sorted({a for op, a, b, _ in parse_lookup(blob)[1] if op == OP_MAIN and b == 0})


def balance(instances, boundary=()):
    """instances: per instance the `fractions` list (or None: no buses); boundary: [((d0, d1), +1 | -1)].
    -> [(denom, net, [push])] ascending by denominator, for every denominator whose net multiplicity is not zero;
    push = (instance, row, column, fraction, (m0, m1)) in (instance, row, column, fraction) order, boundary pushes (instance -1) last."""
    table = {}

    def push(d, m, rec):
        if d == (0, 0):
            raise ZeroDivisionError("a live push with a zero denominator")
        e = table.setdefault(d, [0, 0, []])
        e[0] = (e[0] + m[0]) % P
        e[1] = (e[1] + m[1]) % P
        e[2].append(rec)

    for i, fr in enumerate(instances):
        if not fr:
            continue
        n = len(fr[0][2])
        for r in range(n):
            for c, j, m0, m1, d0, d1 in fr:
                m = (m0[r], m1[r])
                if m != (0, 0):
                    push((d0[r], d1[r]), m, (i, r, c, j, m))
    for k, (d, s) in enumerate(boundary):
        m = (s % P, 0)
        push((int(d[0]) % P, int(d[1]) % P), m, (-1, 0, 0, k, m))
    return [(d, (e[0], e[1]), e[2]) for d, e in sorted(table.items()) if (e[0], e[1]) != (0, 0)]


def e_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_inv(a):
    ni = pow((a[0] * a[0] - 7 * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * ni % P, (P - a[1]) * ni % P)


def residue_sum(report):
    """sum of net / denom over a report: what the buses' accumulator finals (plus the boundary terms) add up to."""
    s = (0, 0)
    for d, net, _ in report:
        t = e_mul(net, e_inv(d))
        s = ((s[0] + t[0]) % P, (s[1] + t[1]) % P)
    return s


def as_report(entries):
    """[BalanceEntry] of the library -> the shape of `balance`."""
    return [((e.denom[0], e.denom[1]), (e.net[0], e.net[1]),
             [(p.instance, p.row, p.column, p.fraction, (p.multiplicity[0], p.multiplicity[1])) for p in e.push_list]) for e in entries]
