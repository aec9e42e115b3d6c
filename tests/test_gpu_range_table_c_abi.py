"""The range-check table laid on the device from plain C (run with -m gpu for the part that needs the device).

examples/range_table_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It uploads a trace of the three-column
test AIR (tests/range_airs.py) whose value and multiplicity columns are junk, calls mh_fill_range_table and prints the table it
downloads; the counts must be the lookups' and the size tests/range_table_ref.py's."""
import os, subprocess
import numpy as np
import pytest
import range_airs as RA
import range_table_ref as RR
from __graft_entry__ import ROOT


def build_example(tmp_path):
    exe = str(tmp_path / "range_table_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "range_table_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_statement(path, trace):
    blob = RA.table_lookup().blob
    log_n = int(trace.shape[0]).bit_length() - 1
    with open(path, "wb") as f:
        f.write(np.array([log_n, trace.shape[1]] + list(RA.SLOT[1:]) + [len(blob)], dtype="<u8").tobytes())
        f.write(np.asarray(blob, dtype="<u8").tobytes())
        f.write(np.ascontiguousarray(trace, dtype="<u8").tobytes())


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbol resolves."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_c_program_lays_the_table(tmp_path):
    exe = build_example(tmp_path)
    n = 1 << 7
    good, unfit, wide = (str(tmp_path / k) for k in ("good.bin", "unfit.bin", "wide.bin"))
    lookups = [7, 7, 7, 300, 2487, 65535, 0, 300]
    write_statement(good, RA.table_trace(lookups, n))
    write_statement(unfit, RA.table_trace(np.arange(0, 2 * n, 2), n))
    t = RA.table_trace(lookups, n)
    t[5, RA.C] = 1 << 16
    write_statement(wide, t)
    present = set(lookups) | {0, 65535}
    need = RR.rows_needed(present)
    r = subprocess.run([exe, good], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "balanced" in r.stdout, r.stdout + r.stderr
    assert f"{len(present)} values in {need} rows, the table starts at row {n - need}; {n} multiplicity cells written, their sum {n}" in r.stdout, r.stdout
    assert "table: 0x16 7x48 300x32 2487x16 65535x16\n" in r.stdout, r.stdout
    r = subprocess.run([exe, unfit], capture_output=True, text=True, timeout=120)
    unfit_need = RR.rows_needed(set(range(0, 2 * n, 2)) | {65535})
    assert r.returncode == 1 and f"needs {unfit_need} rows, the trace has {n}: nothing written" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe, wide], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "1 unmatched denominators" in r.stdout and f"their sum {n - 1}" in r.stdout, r.stdout + r.stderr
