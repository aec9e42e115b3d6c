"""The ChunkNode and TranscriptEval traces from plain C (run with -m gpu for the part that runs).

examples/transcript_traces_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It folds two Keccak claims under a
zero leaf: Keccak traces and digests, the Poseidon2 trace from a ledger of references, then both new builds, no permutation on the host.
The root it prints must be the public root of the same transcript recorded by the Python ledgers (testing/precompile_trace.py)."""
import os, subprocess
import numpy as np
import pytest
import transcript_traces_cases as TC

from miden_vm_amd.testing import precompile_trace as PT  # noqa: E402

pkg = TC.pkg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESSAGES = [b"abc", bytes(range(16, 56))]


def build_example(tmp_path):
    exe = str(tmp_path / "transcript_traces_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "transcript_traces_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def ledger():
    s = PT.Session()
    return TC.case("two claims", s, s.assert_and_fold([s.keccak(m)[1] for m in MESSAGES]))


def test_example_compiles_as_plain_c_and_its_lists_are_the_ledgers(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror), the symbols resolve, and the lists the program spells out
    are `chunk_node_lists`, `transcript_lists` and `Poseidon2Requires.lists(refs=True)` of the ledger the GPU test compares with."""
    assert os.path.exists(build_example(tmp_path))
    c = ledger()
    data, digests, rec = c.cn_lists
    assert bytes(data) == b"".join(MESSAGES)
    assert [tuple(int(x) for x in r) for r in rec] == [(0, 3, 0, 0, 0, 1, 2, 1), (3, 40, 1, 32, 3, 5, 6, 1)]
    nodes, terms, limbs, root = c.te_lists
    assert [tuple(int(x) for x in n) for n in nodes] == [(0,) * 9, (1, 0, 0, -3, 7, 0, 0, 0, 0), (1, 0, 1, -7, 8, 0, 0, 0, 0)]
    assert (terms.size, limbs.size, root) == (0, 0, 2)
    absorptions, blocks, refs = TC.p2_lists(c)
    kk = PT.KECCAK256_PRECOMPILE_ID
    assert [(tuple(int(x) for x in a["cap"]), int(a["n_blocks"]), int(a["in_mult"]), int(a["out_mult"])) for a in absorptions] == \
        [((2, 0, 0, 0), 1, 1, 1), ((2, 0, 0, 0), 1, 1, 1), ((kk, 0, 3, 0), 1, 1, 1), ((2, 0, 0, 0), 2, 1, 1), ((2, 0, 0, 0), 1, 1, 1),
         ((kk, 0, 40, 0), 1, 1, 1), ((1, 0, 0, 0), 1, 1, 1), ((1, 0, 0, 0), 1, 1, 1)]
    assert refs.tolist() == [[-1, -1], [-1, -1], [0, 1], [-1, -1], [-1, -1], [-1, -1], [3, 4], [-1, 2], [6, 5]]
    assert [int(x) for x in blocks[0]] == [0x636261] + [0] * 7 and [int(x) for x in blocks[4]] == [0x33323130, 0x37363534] + [0] * 6
    assert [int(x) for x in blocks[7][:4]] == [0] * 4


@pytest.mark.gpu
def test_c_program_prints_the_ledgers_public_root(tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    c = ledger()
    assert "refused: mh_chunk_node_trace_build: defect 9, index 0, operand 2" in out, out
    assert "chunk/node: 4 x 42 (3 chunk rows, 2 records); eval: 4 x 39 (3 active rows)" in out, out
    assert "root: " + " ".join(str(x) for x in c.public_root) in out, out
    h = " ".join(str(int(x)) for x in c.cn_exp[1, 12 + 25:12 + 29])
    assert f"h_keccak of message 1: {h}; the root row's rhs: {h}" in out, out
    assert (c.cn_exp.shape, c.te_exp.shape) == ((4, 42), (4, 39))
