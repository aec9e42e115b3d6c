"""The Keccak round and sponge traces from plain C (run with -m gpu for the part that runs).

examples/keccak_traces_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It hands the messages "" and "abc"
to mh_keccak_traces_build, prints the two digests and reads a few cells back.  What it prints must be the known answers of Keccak-256
and what the generators (testing/precompile_trace.py) give on the same messages."""
import os, subprocess
import pytest
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
ABC = "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def build_example(tmp_path):
    exe = str(tmp_path / "keccak_traces_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "keccak_traces_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_c_program_builds_both_traces_and_prints_the_known_digests(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    sp = PT.SpongeRequires()
    got = [sp.require(m) for m in (b"", b"abc")]
    assert [g["keccak_digest"].hex() for g in got] == [EMPTY, ABC] and [g["chunk_head"] for g in got] == [0, 1]
    sponge = PT.keccak_sponge_trace(sp)
    assert "round programme: 106 operating slots, 10 levels" in out, out
    assert "refused: mh_keccak_traces_build: defect 1, message 1" in out, out
    assert f"keccak traces: 2 permutations, round 4096 rows, sponge {sponge.shape[0]} rows ({sp.next_sponge_seq} active)" in out, out
    assert f'keccak256("") = {EMPTY}' in out and f'keccak256("abc") = {ABC}' in out, out
    assert (f"round row 0: ip 25 3225, active 1 1; row 3072: active 0; sponge row 32: seq {int(sponge[32, 0])}, bytes left {int(sponge[32, 2])}, "
            f"chunk_ptr {int(sponge[32, 4])}") in out, out
    assert f"keccak-f(0)[0] = {PT.keccak_f_reference([0] * 25)[0]:016x}" in out, out
