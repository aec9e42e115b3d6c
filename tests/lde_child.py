"""The child process of tests/test_gpu_lde_plans.py::test_switch (not a test): csrc/ntt.hip reads its MH_NTT_* switches once per process,
so every setting gets a process of its own.  Opens one context, runs lde_cases.SWITCH_CASES through Ctx.coset_lde_batch under whatever
switches its environment carries, compares each case with the CPU oracle and prints one line per case:

    CASE <kind> <log_n> <width> <added_bits> ok
    CASE <kind> <log_n> <width> <added_bits> MISMATCH <differing felts> first at (<row>, <column>) | NON-CANONICAL <felts>

Exit status 0: every case equal; 3: a case differs (the lines say which).  Anything else is a crash.

usage: lde_child.py [EXPECTED_DIR]   -- the oracle's LDEs of the distinct columns are taken from EXPECTED_DIR/<kind>_<log_n>_<width>_<ab>.npy
when the file is there (the parent computes them once for all its children); otherwise computed here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import lde_cases as lc  # noqa: E402
import oracle_binding as ob  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def expected_file(directory, case):
    return os.path.join(directory, "%s_%d_%d_%d.npy" % case)


def oracle_lde(case):
    """the oracle's LDE of the distinct columns of a case, on the canonical shift"""
    kind, log_n, width, ab = case
    cols, _, _ = lc.switch_input(*case)
    return ob.coset_lde_bitrev(cols, ab, ob.lib().orc_canonical_lde_shift(log_n + ab))


def main(argv):
    directory = argv[1] if len(argv) > 1 else None
    pkg = load_package()
    ctx = pkg.Ctx(0)
    bad = 0
    for case in lc.SWITCH_CASES:
        kind, log_n, width, ab = case
        _, m, idx = lc.switch_input(*case)
        path = expected_file(directory, case) if directory else None
        exp = np.load(path) if path and os.path.exists(path) else oracle_lde(case)
        got = ctx.coset_lde_batch(m, ab, ob.lib().orc_canonical_lde_shift(log_n + ab))
        verdict = "ok"
        if got.shape != (exp.shape[0], width):
            verdict = "SHAPE %r" % (got.shape,)
        else:
            diff = got != exp[:, idx]
            high = int((got >= np.uint64(ob.P)).sum())
            if diff.any():
                r, c = np.argwhere(diff)[0]
                verdict = "MISMATCH %d first at (%d, %d)" % (int(diff.sum()), r, c)
            elif high:
                verdict = "NON-CANONICAL %d" % high
        bad += verdict != "ok"
        print("CASE %s %d %d %d %s" % (case + (verdict,)), flush=True)
    ctx.close()
    return 3 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
