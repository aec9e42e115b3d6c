"""The four EC traces from plain C (run with -m gpu for the part that runs).

examples/ec_traces_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands the lists of a small ledger (a
pass-through, two chords, a cancel; two intros, a combine, three negs) to mh_ec_traces_build, shows a refusal of the checking pass and
reads a few cells back.  What it prints must be what the generators (testing/precompile_trace.py) give on the same ledgers."""
import os, subprocess
import numpy as np
import pytest
import ec_traces_cases as EC

from miden_vm_amd import precompile_airs as PA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1 << 16


def build_example(tmp_path):
    exe = str(tmp_path / "ec_traces_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "ec_traces_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_example_compiles_as_plain_c_and_its_lists_are_the_ledgers(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror), the symbols resolve, and the lists the program spells out
    are `ec_lists` of the ledgers the GPU test compares with."""
    assert os.path.exists(build_example(tmp_path))
    g, p, a, e, t = EC.lists(EC.sub_neg_ledger())
    flat = lambda arr: [tuple(int(x) for name in arr.dtype.names for x in np.atleast_1d(r[name])) for r in arr]  # noqa: E731
    assert flat(g) == [(8, 9, 2, 3, 1)]
    assert flat(p) == [(1, 0, 0, 0, 0, 1, 1), (1, T, T + 1, T + 2, T + 3, 0, 0), (1, T + 4, T + 5, T + 6, T + 7, 0, 0), (1, T + 8, T + 9, T + 10, T + 11, 0, 0),
                       (1, T + 4, T + 16, T + 6, T + 7, 0, 0), (1, T, T + 20, 0, 0, 2, 0), (1, T + 8, T + 21, 0, 0, 2, 0)]
    assert flat(a) == [(1, 2, 1, 2, 1, 0) + (0,) * 6 + (1,), (1, 3, 2, 4, 5, 0, T + 12, T + 13, T + 14, T + 9, T + 15, T + 8, 2),
                       (1, 3, 5, 1, 3, 0) + (0,) * 6 + (1,), (1, 2, 3, 4, 5, 0, T + 18, T + 13, T + 14, T + 9, T + 19, T + 8, 1)]
    assert flat(e) == [(0, 1, 2, 0, 0, 1, 0, 0, 0, 0), (0, 1, 3, 0, 0, 1, 0, 0, 0, 0), (1, 1, 4, 1, 2, 2, 0, 0, 0, 0), (2, 1, 6, 1, 0, 1, 1, 0, 0, 1),
                       (2, 1, 5, 2, 0, 1, 0, 0, 0, 0), (2, 1, 7, 3, 0, 2, 1, 0, 0, 0)]
    assert flat(t) == [(2, T + 17), (3, T + 17)] * 2 + [(2, 3), (3, 3)] * 2


@pytest.mark.gpu
def test_c_program_builds_the_four_traces_and_prints_the_generators_cells(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    groups, points, add, msm = EC.generator(EC.sub_neg_ledger())
    assert (groups.shape, points.shape, add.shape, msm.shape) == ((2, 6), (8, 14), (16, 21), (8, 38))
    assert "plan: 2 x 8 x 16 x 8 rows; the last expression starts at row 6" in out, out
    assert "refused: mh_ec_traces_build: section 2, defect 11, index 0, operand 0" in out, out
    assert "ec traces: 2 x 6, 8 x 14, 16 x 21, 8 x 38" in out, out
    mult = PA.EP_COL_ECPOINT_MULT
    assert f"reads of the group: {int(groups[0, 5])}; of the point at infinity, G, 2 G: {int(points[0, mult])} {int(points[1, mult])} {int(points[2, mult])}" in out, out
    flags = " ".join("".join(str(int(add[4 * i, c])) for c in range(PA.EA_COL_PAI_P, PA.EA_COL_GEN + 1)) for i in range(4))
    assert "case flags of the four additions: " + flags in out, out
    assert "uses of the expressions: " + " ".join(str(int(msm[r, PA.MS_COL_MULT])) for r in (0, 1, 2, 4, 5, 6)) in out, out
    walk = lambda r: f"{int(msm[r, PA.MS_COL_I])} {int(msm[r, PA.MS_COL_J])} " + "".join(str(int(msm[r, c])) for c in (PA.MS_COL_TAKE_A, PA.MS_COL_TAKE_B, PA.MS_COL_TAKE_BOTH))  # noqa: E731
    assert (f"the combine's rows: i j takes {walk(2)} | {walk(3)}; the last neg's x, y, -y: {int(msm[7, PA.MS_COL_NEG_X])} {int(msm[7, PA.MS_COL_NEG_YA])} "
            f"{int(msm[7, PA.MS_COL_NEG_YR])}") in out, out
