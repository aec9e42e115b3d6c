"""The UintStoreMul and UintAdd traces from plain C (run with -m gpu for the part that runs).

examples/uint_traces_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands a store of eight values under the
modulus 97, two multiply-accumulates and two additions to mh_uint_traces_build, shows a refusal of the witness pass and reads a few cells
back.  What it prints must be what the generators (testing/precompile_trace.py) give on the same ledgers."""
import os, subprocess
import pytest
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    exe = str(tmp_path / "uint_traces_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "uint_traces_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def example_ledgers():
    store, adds, muls = PT.UintStore(), PT.UintAddRequires(), PT.UintMulRequires()
    fp = store.pin_modulus(1, 96)
    store.require_uintval(fp)
    five, seven, three, r0, r1, s0, s1 = (store.intern(v, fp) for v in (5, 7, 3, 73, 59, 12, 35))
    muls.record(2, five, seven, 1, three, r0, fp, 1)
    muls.record(1, five, seven, 1, r0, r1, fp, 2, is_sub=True)
    adds.record(five, seven, s0, fp, 1)
    adds.record_nz(r0, r1, s1, fp, 3)
    return store, adds, muls


def test_example_compiles_as_plain_c_and_its_lists_are_the_ledgers(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror), the symbols resolve, and the lists the program spells out
    are `uint_lists` of the ledgers the GPU test compares with."""
    assert os.path.exists(build_example(tmp_path))
    rows, m, a = PT.uint_lists(*example_ledgers())
    t = 1 << 16
    assert [(int(r["ptr"]), int(r["bound_ptr"]), int(r["value"][0]), int(r["val_reads"]), int(r["limb_reads"])) for r in rows] == \
        [(1, 1, 96, 1, 0)] + [(t + i, 1, v, 0, 0) for i, v in enumerate((5, 7, 3, 73, 59, 12, 35))]
    assert [tuple(int(x) for x in o) for o in m] == [(t, t + 1, t + 2, t + 3, 1, 2, 1, 0, 1), (t, t + 1, t + 3, t + 4, 1, 1, 1, 1, 2)]
    assert [tuple(int(x) for x in o) for o in a] == [(t, t + 1, t + 5, 1, 0, 0, 1), (t + 3, t + 4, t + 6, 1, 1, 0, 3)]


@pytest.mark.gpu
def test_c_program_builds_both_traces_and_prints_the_generators_cells(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    store, adds, muls = example_ledgers()
    add = PT.uint_add_trace(adds, store)
    usm = PT.uint_store_mul_trace(store, muls, PT.BytePairLutRequires())
    assert usm.shape == (32, 44) and add.shape == (4, 30)
    assert "plan: 8 values, 2 multiplications, 2 additions; 32 and 4 rows; bound index of the last value 0" in out, out
    assert "refused: mh_uint_traces_build: section 1, defect 10, index 1, operand 0" in out, out
    assert "uint traces: 32 x 44 and 4 x 30" in out, out
    val, limbs, mo = PA.US_HUB_UINTVAL_MULT, PA.US_HUB_UINTLIMBS_MULT, PA.USM_MUL_OFF
    assert (f"reads of the modulus row: {int(usm[1, val])} UintVal, {int(usm[1, limbs])} UintLimbs; of 73: {int(usm[17, val])}, {int(usm[17, limbs])}") in out, out
    assert (f"quotients {int(usm[3, mo])} {int(usm[11, mo])}, borrows {int(usm[0, mo + PA.UM_COL_BORROW])} {int(usm[8, mo + PA.UM_COL_BORROW])}, "
            f"first carries {int(usm[5, mo])} {int(usm[13, mo])}; k {int(add[1, PA.UA_CELL_K])} {int(add[3, PA.UA_CELL_K])}; "
            f"last pointer {int(usm[31, PA.US_COL_PTR])}") in out, out
