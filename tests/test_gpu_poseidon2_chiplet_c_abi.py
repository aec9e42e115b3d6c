"""The Poseidon2 chiplet trace from plain C (run with -m gpu for the part that runs).

examples/poseidon2_chiplet_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands a chain, a one-shot and an
absorption that refers to both their digests to mh_poseidon2_chiplet_trace_build, prints the digests and reads a few cells back.  What it
prints must be what the generator (testing/precompile_trace.py) gives on the same ledger with literal blocks."""
import os, subprocess
import pytest
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd import precompile_airs as PA  # noqa: E402
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    exe = str(tmp_path / "poseidon2_chiplet_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "poseidon2_chiplet_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_c_program_builds_the_trace_from_references_and_prints_the_generators_digests(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    block = lambda c: ([100 * (c + 1) + i for i in range(4)], [100 * (c + 1) + 4 + i for i in range(4)])  # noqa: E731
    req = PT.Poseidon2Requires()
    chain = req.require_absorption([1, 2, 3, 4], [block(0), block(1)])
    shot = req.require_absorption([5, 6, 7, 8], [block(2)])
    req.require_absorption([9, 10, 11, 12], [(req.digest(chain), req.digest(shot))])
    for a, (im, om) in zip(req.absorptions, [(1, 1), (2, 1), (1, 3)]):
        a[3], a[4] = im, om
    main, _ = PT.poseidon2_chiplet_trace(req)
    assert "plan: 3 absorptions, 4 cycles, 2 levels, 64 rows; starts 0 2 3, levels 0 0 1" in out, out
    assert "refused: mh_poseidon2_chiplet_trace_build: defect 4, index 7" in out, out
    assert "poseidon2 chiplet: 4 cycles in 2 levels, 2^6 rows" in out, out
    for i in range(3):
        assert f"digest {i} = " + " ".join(f"{int(x):016x}" for x in req.digest(i)) in out, out
    assert "reference form == literal form" in out, out
    st, cube = PA.P2C_STATE, PA.P2C_CUBE
    assert (f"row 48: seq 3, in_mult 1, out_mult 3, is_absorb 0, state[0] {int(main[48, st]):016x}, state[4] {int(main[48, st + 4]):016x}, "
            f"cube[0] {int(main[48, cube]):016x}; row 16: is_absorb 1; row 63: state[0] {int(main[63, st]):016x}") in out, out
