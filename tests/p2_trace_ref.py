"""The scan rule of mh_miden_poseidon2_trace (csrc/p2_trace.hip), restated with numpy.  A helper module, not a test:
tests/test_p2_trace_cpu.py holds it to the generators' own request ledgers, tests/test_gpu_p2_trace.py holds the kernels to it.

A row of the chiplets trace [N, 22] is a hasher controller INPUT row iff column 0 is 0 (the hasher's chiplet selector) and column 1 is 1
(controller s0).  Its request id is column 20 (perm_id), its state columns 4..15.  The request list has k = max id + 1 entries; entry c
is the state of the LOWEST input row with id c and the number of input rows with id c.  Defects, in the order the library reports
them: (1, row) an id beyond the table of N/2 + 1 entries, (3, row) an input row whose state differs from its id's first row,
(2, id) an id below k nobody requests -- always the lowest row / id of the kind."""
import numpy as np

COL_CHIPLET_SELECTOR, COL_S0, COL_STATE, COL_PERM_ID = 0, 1, 4, 20


class Defect(Exception):
    def __init__(self, kind, row):
        Exception.__init__(self, f"defect {kind} at {row}")
        self.kind, self.row = kind, row


def input_rows(chiplets):
    t = np.asarray(chiplets, dtype=np.uint64)
    return np.nonzero((t[:, COL_CHIPLET_SELECTOR] == 0) & (t[:, COL_S0] == 1))[0]


def scan(chiplets):
    """-> (states uint64 [k, 12], multiplicities uint64 [k], number of input rows); raises Defect."""
    t = np.asarray(chiplets, dtype=np.uint64)
    rows = input_rows(t)
    ids = t[rows, COL_PERM_ID]
    table = t.shape[0] // 2 + 1
    if (ids >= table).any():
        raise Defect(1, int(rows[ids >= table][0]))
    ids = ids.astype(np.int64)
    k = int(ids.max()) + 1 if rows.size else 0
    mult = np.bincount(ids, minlength=k).astype(np.uint64)
    first = np.full(k, t.shape[0], dtype=np.int64)
    np.minimum.at(first, ids, rows)
    if rows.size:
        differs = (t[rows, COL_STATE:COL_STATE + 12] != t[first[ids], COL_STATE:COL_STATE + 12]).any(axis=1)
        if differs.any():
            raise Defect(3, int(rows[differs][0]))
    if (mult == 0).any():
        raise Defect(2, int(np.nonzero(mult == 0)[0][0]))
    return t[first, COL_STATE:COL_STATE + 12].reshape(k, 12), mult, int(rows.size)


def min_log_n(k):
    """the height log_n = -1 asks for: max(6, ceil log2((k + 1) * 16))"""
    return max(6, ((k + 1) * 16 - 1).bit_length())
