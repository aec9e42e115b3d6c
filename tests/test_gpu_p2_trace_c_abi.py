"""A Miden proof from plain C with the Poseidon2 permutation trace derived on the device (run with -m gpu for the proving part).

examples/p2_trace_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It uploads the core and chiplets matrices of
a reference snapshot statement (tests/golden/ref_traces.json.gz), derives the third trace with mh_miden_poseidon2_trace, compares it with
the snapshot's own matrix, proves through mh_prove_miden_traces and verifies through mh_verify_miden.  The digest it prints must be the
one the Python binding gets from the three host matrices."""
import os, re, subprocess
import numpy as np
import pytest
from __graft_entry__ import load_package
import ref_traces as RT

pkg = load_package()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = RT.load_cases()


def build_example(tmp_path):
    exe = str(tmp_path / "p2_trace_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "p2_trace_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_statement(path, c):
    """the statement file of examples/prove_miden_c_abi.c"""
    pv, aux_in, lhs = RT.public_values(c), RT.aux_inputs(c), RT.log_heights(c)
    with open(path, "wb") as f:
        f.write(np.array(lhs + [len(aux_in)] + pv + aux_in, dtype="<u8").tobytes())
        for k in ("core", "chiplets", "poseidon2"):
            f.write(np.ascontiguousarray(c[k], dtype="<u8").tobytes())


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and both symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("case,hash_fn", [(13, "poseidon2"), (20, "blake3")])
def test_c_program_derives_proves_and_verifies(tmp_path, case, hash_fn):
    c = CASES[case - 1]
    exe, stmt = build_example(tmp_path), str(tmp_path / "statement.bin")
    write_statement(stmt, c)
    env = dict(os.environ, MH_JIT_CACHE_RO_DIR=os.path.join(ROOT, "miden-vm_amd", "jit_cache"))
    r = subprocess.run([exe, stmt, str(pkg.Ctx.LMCS[hash_fn])], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "derived trace equals the host-built one" in out and "verified" in out, out
    m = re.search(r"digest ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16})", out)
    ctx = pkg.Ctx(0)
    try:
        pv, aux_in = RT.public_values(c), RT.aux_inputs(c)
        host = pkg.Miden(ctx).prove(c["core"], c["chiplets"], c["poseidon2"], pv, aux_in, hash_fn=hash_fn)
        assert [int(g, 16) for g in m.groups()] == [int(x) for x in host.digest]
    finally:
        ctx.close()
