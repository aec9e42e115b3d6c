"""The whole chiplets trace from plain C (run with -m gpu for the part that runs).

examples/chiplets_build_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands the five lists of a small
program to mh_miden_chiplets_build, reads the trace back, checks the frame and derives the third main trace.  What it prints must be
what the rules (tests/*_section_ref.py, tests/chiplets_frame_ref.py) give on the same lists."""
import os, subprocess
import numpy as np
import pytest
import ace_section_ref as AR
import chiplets_frame_ref as FR
from __graft_entry__ import load_package

pkg = load_package()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = AR.P


def build_example(tmp_path):
    exe = str(tmp_path / "chiplets_build_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "chiplets_build_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_c_program_builds_the_trace_and_derives_the_third(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    # the evaluation of the example, restated
    felts = [3, 0, 6, 0, P - 1, 0, 0, 0, AR.encode(7, 5, 2), AR.encode(7, 3, 1), AR.encode(2, 6, 0), AR.encode(1, 1, 1)]
    rows, ref = AR.section(np.array([(0, 1024, 9, 4, 4, 0, 0)], dtype=AR.DT), felts)
    st, pad, trace_len = FR.starts([8, 24, 9, rows.shape[0], 3])
    assert "refused: mh_miden_bitwise_section: defect 1, op 2" in out, out
    assert (f"chiplets trace: 2^6 rows, trace_len {trace_len}, starts {' '.join(str(x) for x in st)}, padding from {pad}") in out, out
    assert (f"ace: {ref['n_rows']} rows, {ref['n_wires']} wires, {ref['n_gates']} gates, {ref['n_rounds']} rounds; "
            "kernel rom: 3 rows for 3 calls") in out, out
    assert f"and result {0xDEADBEEF & 0x0F0F1234:08x}, first kernel row m 0 h0 100" in out and "poseidon2 trace: 2 requests" in out, out
