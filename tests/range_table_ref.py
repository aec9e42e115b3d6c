"""The reference of the range-table tests: the semantics of mh_fill_range_table (include/midenhip.h) over Python integers, on top of
balance_ref.fractions and multiplicity_ref.fill.  Nothing here calls the library.

  probe    the declaring instance's program on a copy of its trace with the value column 0 (P0), then 1 (P1).  Refused: the provider's
           multiplicity differs ("mult"); its denominator is not d0 + g * cell with d0, g the same on every row and g != 0 ("denom");
           another fraction differs ("reader").  The first offending fraction in program order is named.
  mark     every push with a non-zero multiplicity except the provider's, boundary pushes included: t = (d - d0) / g; t in the base
           field and below 2^16 -> the value t is present.  0 and 65535 always are.
  rows     per present value 1 + bridge_rows(gap to the value before), plus the trailing row.  Refused: more rows than the trace ("rows").
  emit     zeros in rows [0, n - rows_needed) of both columns, then the table: bridge rows by the strides 3^7 .. 3^0, the value row;
           the last row is 65535.
  fill     multiplicity_ref.fill with the provider as the one slot; the count of value 0 is moved from row 0 to the table's first row."""
import balance_ref as BR
import multiplicity_ref as MR

P = BR.P
MAX_STRIDE = 3 ** 7
Refused = MR.Refused


def bridge_rows(gap):
    """get_num_bridge_rows (processor/src/trace/range/mod.rs:167-180)."""
    rows, stride = 0, MAX_STRIDE
    while gap != stride:
        if gap > stride:
            rows += 1
            gap -= stride
        else:
            stride //= 3
    return rows


def table_values(present):
    """write_rows over the ascending present values, then the trailing row (range/mod.rs:106-119, 184-204) -> the value column of the table."""
    out, prev = [], 0
    for v in sorted(present):
        gap, stride = v - prev, MAX_STRIDE
        while gap != stride:
            if gap > stride:
                gap -= stride
                prev += stride
                out.append(prev)
            else:
                stride //= 3
        out.append(v)
        prev = v
    out.append(65535)
    return out


def rows_needed(present):
    prev, rows = 0, 1
    for v in sorted(present):
        rows += 1 + bridge_rows(v - prev)
        prev = v
    return rows


def _sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def fill(blobs, mains, rnd, slot, boundary=(), preps=None):
    """blobs / mains / preps as multiplicity_ref.fill; slot = (instance, lookup_column, fraction, value_column, mult_column).
    -> (info = dict(n_values, rows_needed, rows_available), the filled copies of `mains`, the report of balance_ref.balance over them).
    Refused carries `info` when the table does not fit."""
    n_in = len(blobs)
    preps = list(preps) if preps is not None else [None] * n_in
    si, c, j, vc, mc = (int(x) for x in slot)
    cols = [BR.parse_lookup(b)[2] for b in blobs]
    if not (0 <= si < n_in and 0 <= c < len(cols[si]) and 0 <= j < len(cols[si][c]) and 0 <= vc < mains[si].shape[1]
            and 0 <= mc < mains[si].shape[1]) or vc == mc:
        raise Refused("range", slot)
    kslot = sum(len(x) for x in cols[si][:c]) + j
    n = mains[si].shape[0]
    # probe
    t = mains[si].copy()
    t[:, vc] = 0
    f0 = BR.fractions(blobs[si], t, rnd, prep=preps[si])
    t[:, vc] = 1
    f1 = BR.fractions(blobs[si], t, rnd, prep=preps[si])
    d0 = g = None
    for k, (x, y) in enumerate(zip(f0, f1)):
        same_m = (x[2] == y[2]).all() and (x[3] == y[3]).all()
        if k == kslot:
            d0 = (x[4][0], x[5][0])
            g = _sub((y[4][0], y[5][0]), d0)
            if not same_m:
                raise Refused("mult", (si, x[0], x[1]))
            uniform = all((x[4][r], x[5][r]) == d0 and _sub((y[4][r], y[5][r]), (x[4][r], x[5][r])) == g for r in range(n))
            if g == (0, 0) or not uniform:
                raise Refused("denom", (si, x[0], x[1]))
        elif not (same_m and (x[4] == y[4]).all() and (x[5] == y[5]).all()):
            raise Refused("reader", (si, x[0], x[1]))
    # mark
    ginv = BR.e_inv(g)
    present = {0, 65535}

    def mark(d):
        v = BR.e_mul(_sub(d, d0), ginv)
        if v[1] == 0 and v[0] < 1 << 16:
            present.add(v[0])

    for i in range(n_in):
        fr = f0 if i == si else BR.fractions(blobs[i], mains[i], rnd, prep=preps[i])
        for k, x in enumerate(fr):
            if i == si and k == kslot:
                continue
            for r in range(mains[i].shape[0]):
                if (x[2][r], x[3][r]) != (0, 0):
                    mark((x[4][r], x[5][r]))
    for d, _ in boundary:
        mark((int(d[0]) % P, int(d[1]) % P))
    # rows
    need = rows_needed(present)
    info = dict(n_values=len(present), rows_needed=need, rows_available=n)
    if need > n:
        e = Refused("rows", info)
        e.info = info
        raise e
    # emit
    out = [m.copy() for m in mains]
    table = table_values(present)
    assert len(table) == need
    pad = n - need
    out[si][:, vc] = [0] * pad + table
    out[si][:, mc] = 0
    # fill
    _, out, report = MR.fill(blobs, out, rnd, [(si, c, j, mc)], boundary=boundary, preps=preps)
    if pad:
        out[si][[0, pad], mc] = out[si][[pad, 0], mc]
    return info, out, report
