"""The reference of the multiplicity-fill tests: the semantics of mh_fill_multiplicities (include/midenhip.h) over Python integers and
dicts, on top of balance_ref.fractions.  Nothing here calls the library.

  probe    per instance with declared columns: the program on a copy of the trace with every declared column 0 (P0), then 1 (P1);
           for a slot a = m_P0, b = m_P1 - m_P0, key = d.  Refused: a slot's d differs, a slot's b has c1 != 0, another fraction's m
           or d differs, a slot out of range, two slots on one fraction, a live push with a zero denominator.
  net      per key the sum of a over the pushes with a != 0 (and the boundary pushes); owner = the lowest push id (instance base +
           row * K + fraction) among the slot pushes with b != 0.
  resolve  per (instance, declared column, row) the first slot of the column in declaration order with b != 0: the cell becomes
           -net_c0 / b if that push owns its key, 0 otherwise; no such slot: untouched.
  verify   balance_ref.balance over the filled traces."""
import numpy as np
import balance_ref as BR

P = BR.P


class Refused(Exception):
    """The declaration (or the statement) is refused: MH_ERR_INVALID in the library.  `reason` is one of "range", "duplicate", "key",
    "ef", "reader", "zero"."""
    def __init__(self, reason, where=None):
        super().__init__(f"{reason}: {where}")
        self.reason, self.where = reason, where


def fill(blobs, mains, rnd, slots, boundary=(), preps=None):
    """blobs / mains / preps: per instance the lookup blob, the main trace [n, w] (np.uint64, NOT modified) and the preprocessed matrix
    or None; slots: [(instance, lookup_column, fraction, main_column)].
    -> (cells written, the filled copies of `mains`, the report of balance_ref.balance over them)."""
    n_in = len(blobs)
    preps = list(preps) if preps is not None else [None] * n_in
    cols = [BR.parse_lookup(b)[2] for b in blobs]
    seen = set()
    for s in slots:
        i, c, j, mc = (int(x) for x in s)
        if not (0 <= i < n_in and 0 <= c < len(cols[i]) and 0 <= j < len(cols[i][c]) and 0 <= mc < mains[i].shape[1]):
            raise Refused("range", s)
    for s in slots:
        if tuple(s[:3]) in seen:
            raise Refused("duplicate", s)
        seen.add(tuple(s[:3]))
    if not slots:
        frs = [BR.fractions(b, m, rnd, prep=p) for b, m, p in zip(blobs, mains, preps)]
        return 0, [m.copy() for m in mains], _balance(frs, boundary)

    def flat(i, c, j):
        return sum(len(x) for x in cols[i][:c]) + j

    declared = [[] for _ in range(n_in)]              # per instance its declared columns, first appearance first
    slot_of = [dict() for _ in range(n_in)]           # per instance: flat fraction index -> main column
    for i, c, j, mc in slots:
        slot_of[i][flat(i, c, j)] = mc
        if mc not in declared[i]:
            declared[i].append(mc)
    f0, f1 = [], []
    for i in range(n_in):
        if declared[i]:
            t = mains[i].copy()
            t[:, declared[i]] = 0
            f0.append(BR.fractions(blobs[i], t, rnd, prep=preps[i]))
            t[:, declared[i]] = 1
            f1.append(BR.fractions(blobs[i], t, rnd, prep=preps[i]))
        else:
            f0.append(BR.fractions(blobs[i], mains[i], rnd, prep=preps[i]))
            f1.append(None)
    # the declaration, numerically: the first offending (instance, fraction)
    for i in range(n_in):
        if f1[i] is None:
            continue
        for k, (x, y) in enumerate(zip(f0[i], f1[i])):
            c, j = x[0], x[1]
            same_d = (x[4] == y[4]).all() and (x[5] == y[5]).all()
            if k in slot_of[i]:
                if not same_d:
                    raise Refused("key", (i, c, j))
                if ((y[3] - x[3]) % P != 0).any():
                    raise Refused("ef", (i, c, j))
            elif not (same_d and (x[2] == y[2]).all() and (x[3] == y[3]).all()):
                raise Refused("reader", (i, c, j))
    # net
    table = {}  # key -> [net0, net1, owner id | None]
    base, bases = 0, []
    for i in range(n_in):
        bases.append(base)
        n, K = mains[i].shape[0], len(f0[i])
        for r in range(n):
            for k, x in enumerate(f0[i]):
                a = (x[2][r], x[3][r])
                b = (f1[i][k][2][r] - x[2][r]) % P if k in slot_of[i] else 0
                if a == (0, 0) and b == 0:
                    continue
                d = (x[4][r], x[5][r])
                if d == (0, 0):
                    raise Refused("zero", (i, x[0], x[1], r))
                e = table.setdefault(d, [0, 0, None])
                e[0], e[1] = (e[0] + a[0]) % P, (e[1] + a[1]) % P
                if b:
                    pid = base + r * K + k
                    e[2] = pid if e[2] is None else min(e[2], pid)
        base += n * K
    for d, s in boundary:
        e = table.setdefault((int(d[0]) % P, int(d[1]) % P), [0, 0, None])
        e[0] = (e[0] + s) % P
    # resolve
    out = [m.copy() for m in mains]
    written = 0
    for i in range(n_in):
        K = len(f0[i])
        for mc in declared[i]:
            ks = [flat(si, c, j) for si, c, j, smc in slots if si == i and smc == mc]
            for r in range(mains[i].shape[0]):
                for k in ks:
                    b = (f1[i][k][2][r] - f0[i][k][2][r]) % P
                    if not b:
                        continue
                    e = table[(f0[i][k][4][r], f0[i][k][5][r])]
                    out[i][r, mc] = (-e[0] * pow(b, P - 2, P)) % P if e[2] == bases[i] + r * K + k else 0
                    written += 1
                    break
    frs = [BR.fractions(b, m, rnd, prep=p) for b, m, p in zip(blobs, out, preps)]
    return written, out, _balance(frs, boundary)


def _balance(frs, boundary):
    try:
        return BR.balance(frs, boundary)
    except ZeroDivisionError as e:
        raise Refused("zero", str(e))
