"""A Miden proof from plain C with the memory rows of the chiplets trace built on the device (run with -m gpu for the proving part).

examples/memory_section_c_abi.c is compiled with gcc against include/midenhip.h + libmidenhip.so.  It uploads the chiplets matrix of a
testing/core_trace.py program with its memory rows blanked, rebuilds them with mh_miden_memory_section from the access list, compares
the result with the generator's matrix, proves through mh_prove_miden_traces and verifies through mh_verify_miden.  The digest it prints
must be the one the Python binding gets from the three host matrices."""
import os, re, subprocess
import numpy as np
import pytest
import range_airs as RA
from __graft_entry__ import load_package

pkg = load_package()
from miden_vm_amd.testing import core_trace as CV  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    exe = str(tmp_path / "memory_section_c_abi")
    lib_dir = os.path.join(ROOT, "miden-vm_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "memory_section_c_abi.c"), "-L" + lib_dir, "-lmidenhip", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def write_statement(path, r, start_row, accesses):
    """the statement file of examples/prove_miden_c_abi.c, then start_row, n and the 48-byte access records"""
    lhs = [int(r[k].shape[0]).bit_length() - 1 for k in ("core", "chiplets", "poseidon2")]
    with open(path, "wb") as f:
        f.write(np.array(lhs + [len(r["aux_inputs"])] + list(r["public_values"]) + list(r["aux_inputs"]), dtype="<u8").tobytes())
        for k in ("core", "chiplets", "poseidon2"):
            f.write(np.ascontiguousarray(r[k], dtype="<u8").tobytes())
        f.write(np.array([start_row, len(accesses)], dtype="<u8").tobytes())
        f.write(np.ascontiguousarray(accesses, dtype=pkg.MEM_ACCESS_DTYPE).tobytes())


def test_example_compiles_as_plain_c(tmp_path):
    """No GPU needed: the header's new section is plain C (gcc -Wall -Werror) and the symbols resolve."""
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("iters,hash_fn", [(1, "poseidon2"), (2, "blake3")])
def test_c_program_builds_proves_and_verifies(tmp_path, iters, hash_fn):
    vm = CV.CoreVM(stack_inputs=tuple(range(16)))
    r = CV.prove_inputs(vm, RA.u32_memory_program(iters))
    t = r["chiplets"]
    rows = np.nonzero((t[:, 0] == 1) & (t[:, 1] == 1) & (t[:, 2] == 0))[0]
    acc = vm.chiplets.memory.access_array()
    assert rows.size == len(acc) > 0
    exe, stmt = build_example(tmp_path), str(tmp_path / "statement.bin")
    write_statement(stmt, r, int(rows[0]), acc)
    env = dict(os.environ, MH_JIT_CACHE_RO_DIR=os.path.join(ROOT, "miden-vm_amd", "jit_cache"))
    run = subprocess.run([exe, stmt, str(pkg.Ctx.LMCS[hash_fn])], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    assert "refused: mh_miden_memory_section: defect 1" in out and f"built: {len(acc)} rows" in out, out
    assert "rebuilt trace equals the host-built one" in out and "verified" in out, out
    m = re.search(r"digest ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16})", out)
    ctx = pkg.Ctx(0)
    try:
        host = pkg.Miden(ctx).prove(r["core"], r["chiplets"], r["poseidon2"], r["public_values"], r["aux_inputs"], hash_fn=hash_fn)
        assert [int(g, 16) for g in m.groups()] == [int(x) for x in host.digest]
    finally:
        ctx.close()
