"""The rule of the kernel ROM's trace section (include/midenhip.h mh_kernel_rom_section_build; processor/src/trace/chiplets/kernel_rom/
mod.rs), restated on Python integers: one row m | h0..h3 per distinct declared digest, sorted by the 32 canonical little-endian bytes."""
import numpy as np

P = 0xFFFFFFFF00000001
WIDTH = 5
MAX_PROCS = 255


class Defect(Exception):
    def __init__(self, kind, index):
        super().__init__(f"defect {kind} at {index}")
        self.kind, self.index = kind, index


def key(digest):
    return b"".join((int(x) % P).to_bytes(8, "little") for x in digest)


def min_log_n(rows):
    return max(6, (rows - 1).bit_length()) if rows else 6


def section(procs, calls, cap_rows=None):
    """-> (rows uint64 [n_rows, 5], digests uint64 [n_rows, 4] in trace order).  Defect 1: a call of an undeclared digest, the lowest
    call; defect 2: the rows do not fit `cap_rows`, index = the first row without room."""
    procs = np.asarray(procs, dtype=np.uint64).reshape(-1, 4)
    calls = np.asarray(calls, dtype=np.uint64).reshape(-1, 4)
    assert len(procs) <= MAX_PROCS
    table = {}
    for d in procs:
        table.setdefault(key(d), [[int(x) % P for x in d], 0])
    for i, d in enumerate(calls):
        if key(d) not in table:
            raise Defect(1, i)
        table[key(d)][1] += 1
    if cap_rows is not None and len(table) > cap_rows:
        raise Defect(2, cap_rows)
    out = np.zeros((len(table), WIDTH), dtype=np.uint64)
    for r, k in enumerate(sorted(table)):
        out[r] = [table[k][1]] + table[k][0]
    return out, out[:, 1:5].copy()
