"""The rule of the bitwise chiplet's trace section (include/midenhip.h mh_bitwise_section_build; processor/src/trace/chiplets/bitwise/
mod.rs), restated on Python integers: 13 columns, 8 rows per operation, 4 bits per row from the most significant nibble."""
import numpy as np

DT = np.dtype([("op", "<u4"), ("a", "<u4"), ("b", "<u4")])
WIDTH = 13
AND, XOR = 0, 1


class Defect(Exception):
    def __init__(self, kind, index):
        super().__init__(f"defect {kind} at op {index}")
        self.kind, self.index = kind, index


def min_log_n(rows):
    return max(6, (rows - 1).bit_length()) if rows else 6


def section(ops, cap_rows=None):
    """-> (rows uint64 [8 n, 13], results [n]).  Defect 1: op > 1 at the lowest index; defect 2: the rows do not fit `cap_rows`,
    index = the first op without its rows."""
    ops = np.asarray(ops, dtype=DT).reshape(-1) if len(ops) else np.zeros(0, dtype=DT)
    for i, o in enumerate(ops):
        if int(o["op"]) > 1:
            raise Defect(1, i)
    if cap_rows is not None and 8 * len(ops) > cap_rows:
        raise Defect(2, cap_rows // 8)
    out = np.zeros((8 * len(ops), WIDTH), dtype=np.uint64)
    results = np.zeros(len(ops), dtype=np.uint32)
    for k, o in enumerate(ops):
        op, a, b = int(o["op"]), int(o["a"]), int(o["b"])
        result = 0
        for i in range(8):
            off = 28 - 4 * i
            aa, ba = a >> off, b >> off
            prev = result
            nibble = ((aa & ba) if op == AND else (aa ^ ba)) & 0xF
            result = (prev << 4) | nibble
            out[8 * k + i] = [op, aa, ba] + [(aa >> j) & 1 for j in range(4)] + [(ba >> j) & 1 for j in range(4)] + [prev, result]
        results[k] = result
    return out, results
