"""The frame of the chiplets trace (include/midenhip.h mh_miden_chiplets_build, mh_miden_chiplets_frame; processor/src/trace/chiplets/
mod.rs:58-73, 134-173, 213-310): the five sections stacked behind their selector prefixes, the padding band, chip_clk = row + 1."""
import numpy as np

WIDTH = 22
CHIP_CLK = 21
# section -> (number of selector ones before the zero, first payload column, payload width)
LAYOUT = [(0, 1, 20), (1, 2, 13), (2, 3, 17), (3, 4, 16), (4, 5, 5)]
FRAME_SECTION = 5   # mh_chiplets_info.defect_section of a trace that does not fit


class Defect(Exception):
    def __init__(self, section, kind, index):
        super().__init__(f"section {section}: defect {kind} at {index}")
        self.section, self.kind, self.index = section, kind, index


def min_log_n(trace_len):
    return max(6, (trace_len - 1).bit_length())


def starts(section_rows):
    """-> (start[5], padding_start, trace_len) for the five sections' row counts."""
    at, out = 0, []
    for n in section_rows:
        out.append(at)
        at += n
    return out, at, at + 1


def place(t, section, start, rows):
    """Write `rows` of `section` into the width-22 matrix t at `start`: the selector prefix and the payload columns, nothing else."""
    ones, col0, width = LAYOUT[section]
    n = rows.shape[0]
    assert rows.shape[1] == width
    t[start:start + n, 0:ones] = 1
    t[start:start + n, ones] = 0
    t[start:start + n, col0:col0 + width] = rows
    return t


def frame(t, padding_start):
    """mh_miden_chiplets_frame: chip_clk on every row; from padding_start on selector ones and a zero payload."""
    n = t.shape[0]
    t[:, CHIP_CLK] = np.arange(1, n + 1, dtype=np.uint64)
    t[padding_start:, 0:5] = 1
    t[padding_start:, 5:CHIP_CLK] = 0
    return t


def stack(sections, log_n=None):
    """-> (trace uint64 [2^log_n, 22], start[5], padding_start, trace_len).  A trace_len above 2^log_n is a defect of the frame."""
    st, pad, trace_len = starts([s.shape[0] for s in sections])
    log_n = min_log_n(trace_len) if log_n is None else log_n
    if trace_len > 1 << log_n:
        raise Defect(FRAME_SECTION, 1, trace_len)
    t = np.zeros((1 << log_n, WIDTH), dtype=np.uint64)
    for i, s in enumerate(sections):
        place(t, i, st[i], s)
    return frame(t, pad), st, pad, trace_len
