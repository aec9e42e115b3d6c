"""The hasher controller's rows and the third main trace from plain C (run with -m gpu for the part that runs).

examples/hasher_section_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands a small mixed list of hash
operations to mh_miden_hasher_section, which writes the controller rows in place into a device-resident chiplets trace, derives the
Poseidon2 permutation trace with mh_miden_poseidon2_trace and compares the two request counts.  The counts and the block digest it
prints must be the ones of the rule (tests/hasher_section_ref.py) on the same list."""
import os, re, subprocess
import numpy as np
import pytest
import hasher_section_ref as HR
from __graft_entry__ import load_package

pkg = load_package()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    exe = str(tmp_path / "hasher_section_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "hasher_section_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_c_program_builds_the_section_and_derives_the_third_trace(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    # the list of the example, restated
    felts = (np.arange(1, 65, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    ops = np.array([(0, 0, 0, 0), (1, 0, 5, 12), (2, 3, 0, 20), (3, 3, 5, 44), (4, 3, 5, 44), (0, 0, 0, 0), (2, 3, 0, 20)], dtype=HR.DT)
    rows, results, ref = HR.section(ops, felts)
    assert "refused: mh_miden_hasher_section: defect 3, op 4" in out, out
    assert (f"hasher section: n_rows {rows.shape[0]}, n_permutations {ref['n_permutations']}, n_requests {ref['n_requests']}, "
            f"mrupdate_id {ref['mrupdate_id']}") in out, out
    assert f"poseidon2 trace: {ref['n_requests']} requests from {ref['n_permutations']} controller input rows" in out and "n_requests agree" in out, out
    m = re.search(r"block digest ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16}) at addr (\d+)", out)
    assert [int(g, 16) for g in m.groups()[:4]] == [int(x) for x in results["state"][2][0:4]] and int(m.group(5)) == int(results["addr"][2])
