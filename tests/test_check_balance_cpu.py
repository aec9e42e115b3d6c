"""CPU-only parts of the bus-balance checker (include/midenhip.h mh_check_balance*): the tests' Python reference against the CPU
oracle's LogUp accumulator, the statements' boundary lists (shared by eval_external and the balance check) against the Python
restatements, and the ABI across header, Rust declarations and Python layer."""
import ctypes as C
import os, re, shutil, subprocess
import numpy as np
import pytest
import airs as A
import balance_ref as BR
import oracle_binding as ob
import ref_traces as RT
from __graft_entry__ import load_package, ROOT
from miden_vm_amd import miden_statement as MS, precompile_airs as PA

P = BR.P
BALANCE_FUNCS = ["mh_check_balance", "mh_check_balance_miden", "mh_check_balance_miden_traces", "mh_check_balance_precompile",
                 "mh_check_balance_precompile_traces"]


@pytest.mark.parametrize("log_n,valid", [(4, True), (6, False), (9, False)])
def test_reference_residue_equals_the_accumulator_final(log_n, valid):
    """sum of net / denom over the reference's unmatched denominators = the oracle's LogUp accumulator final: every matched
    denominator contributes zero to the running sum."""
    _, lookup = A.logup_air()
    main = A.logup_trace(log_n, valid=valid)
    for rnd in ([(3, 5), (7, 11)], [(1 << 40, 12345), (P - 2, 99)]):
        rep = BR.balance([BR.fractions(lookup.blob, main, rnd)])
        _, fin = ob.lookup_build_aux(lookup, main, rnd)
        assert BR.residue_sum(rep) == (int(fin[0]), int(fin[1]))
        assert (rep == []) == valid
        if not valid:  # the looked-up value that is not in the table, and the table row that lost a reader
            assert len(rep) == 2 and min(len(p) for _, _, p in rep) == 1


def test_range_air_reference_with_preprocessed():
    air, lookup, trace = A.range_air(6)
    rnd = [(3, 5), (7, 11)]
    assert BR.balance([BR.fractions(lookup.blob, trace(), rnd, prep=air.preprocessed)]) == []
    rep = BR.balance([BR.fractions(lookup.blob, trace(valid=False), rnd, prep=air.preprocessed)])
    _, fin = ob.lookup_build_aux(lookup, trace(valid=False), rnd, preprocessed=air.preprocessed)
    assert rep and BR.residue_sum(rep) == (int(fin[0]), int(fin[1]))


def test_miden_eval_external_is_unchanged():
    """mh_miden_eval_external (now a sum over the shared boundary list) against the Python restatement, on the snapshots' inputs."""
    lib = load_package().load_library()
    rng = np.random.default_rng(5)
    for c in RT.load_cases()[::5]:
        aux_in = RT.aux_inputs(c)
        aux_in[4:8] = [int(x) for x in rng.integers(0, P, 4, dtype=np.uint64)]  # a non-trivial deferred root: the -1 term
        rnd = [tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)) for _ in range(2)]
        finals = [[tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64))] for _ in range(3)]
        exp = MS.eval_external(rnd, RT.public_values(c), aux_in, finals, RT.log_heights(c))[0]
        r = np.array([x for e in rnd for x in e], dtype=np.uint64)
        a = np.array(aux_in, dtype=np.uint64)
        vals = [np.array(f[0], dtype=np.uint64) for f in finals]
        vp = (C.POINTER(C.c_uint64) * 3)(*[ob.ptr(v) for v in vals])
        nv = (C.c_size_t * 3)(1, 1, 1)
        out = np.zeros(2, dtype=np.uint64)
        assert lib.mh_miden_eval_external(ob.ptr(r), ob.ptr(a), C.c_size_t(a.size), vp, nv, C.c_int(3), ob.ptr(out)) == 0
        assert (int(out[0]), int(out[1])) == exp


@pytest.mark.parametrize("name,fixed_uints", [("mh_external_precompile_session", True), ("mh_external_precompile_session_ec_only", False)])
def test_precompile_session_external_is_unchanged(name, fixed_uints):
    lib = load_package().load_library()
    rng = np.random.default_rng(6)
    rnd = [tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)) for _ in range(2)]
    finals = [[tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64))] for _ in range(12)]
    exp = PA.eval_external(rnd, finals, fixed_uints=fixed_uints)[0]
    r = np.array([x for e in rnd for x in e], dtype=np.uint64)
    vals = [np.array(f[0], dtype=np.uint64) for f in finals]
    vp = (C.POINTER(C.c_uint64) * 12)(*[ob.ptr(v) for v in vals])
    nv = (C.c_size_t * 12)(*[1] * 12)
    lh = (C.c_uint8 * 12)(*[4] * 12)
    out = np.zeros(2, dtype=np.uint64)
    assert getattr(lib, name)(None, ob.ptr(r), C.c_size_t(2), vp, nv, lh, C.c_int(12), ob.ptr(out), C.c_size_t(1)) == 1
    assert (int(out[0]), int(out[1])) == exp


def test_abi_agrees_across_header_rust_and_python():
    pkg = load_package()
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midenhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    for f in BALANCE_FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
    assert re.search(r"#define\s+MH_BALANCE_NO_PUSHES\s+UINT64_MAX", h) and "pub const MH_BALANCE_NO_PUSHES: u64 = u64::MAX;" in rs
    assert pkg.MH_BALANCE_NO_PUSHES == (1 << 64) - 1
    for name, cls in (("mh_balance_entry", pkg.BalanceEntry), ("mh_balance_push", pkg.BalancePush)):
        fields = [n for n, _ in cls._fields_]
        assert re.findall(r"pub (\w+):", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1)) == fields
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name, h, flags=re.S).group(1)
        assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == fields


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_ctypes_structures_match_the_c_structs(tmp_path):
    pkg = load_package()
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "midenhip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mh_balance_entry), offsetof(mh_balance_entry, first_push), '
                   'sizeof(mh_balance_push), offsetof(mh_balance_push, fraction), offsetof(mh_balance_push, row), '
                   'offsetof(mh_balance_push, multiplicity)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    E, Q = pkg.BalanceEntry, pkg.BalancePush
    assert got == [C.sizeof(E), E.first_push.offset, C.sizeof(Q), Q.fraction.offset, Q.row.offset, Q.multiplicity.offset] == [48, 40, 40, 8, 16, 24]


def test_library_exports_the_balance_checker():
    pkg = load_package()
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = pkg.load_library()
    for f in BALANCE_FUNCS:
        assert hasattr(lib, f), f
