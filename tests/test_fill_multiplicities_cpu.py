"""CPU-only parts of the multiplicity fill (include/midenhip.h mh_fill_multiplicities*): the tests' Python reference
(tests/multiplicity_ref.py) against the numpy ledgers it replaces, the structural slot helper of dag.Lookup, and the ABI across header,
Rust declarations, Python layer and the built library."""
import ctypes as C
import os, re
import numpy as np
import pytest
import airs as A
import multiplicity_ref as MR
from __graft_entry__ import load_package, ROOT
from miden_vm_amd import dag

P = MR.P
RNDS = ([(3, 5), (7, 11)], [(1 << 40, 12345), (P - 2, 99)])
FILL_FUNCS = ["mh_fill_multiplicities", "mh_fill_multiplicities_miden_traces", "mh_fill_multiplicities_precompile_traces"]


@pytest.mark.parametrize("log_n", [4, 10, 12])
def test_reference_reproduces_bincount_on_logup_trace(log_n):
    """M zeroed, then junk: the reference writes np.bincount's column back (the table values are distinct, so every key has one
    provider row and the unique-owner comparison is legitimate)."""
    _, lookup = A.logup_air()
    good = A.logup_trace(log_n, seed=3)
    n = 1 << log_n
    assert len(set(int(x) for x in good[:, 1])) == n
    for junk, rnd in zip((0, 0xDEADBEEF), RNDS if log_n < 12 else RNDS[:1]):
        t = good.copy()
        t[:, 2] = junk
        written, (filled,), report = MR.fill([lookup.blob], [t], rnd, [(0, 0, 1, 2)])
        assert written == n and report == []
        assert (filled == good).all()
        assert (t[:, 2] == junk).all()  # the input is not modified


@pytest.mark.parametrize("log_n", [5, 8])
def test_reference_reproduces_bincount_on_range_air(log_n):
    air, lookup, trace = A.range_air(log_n)
    good = trace()
    n = 1 << log_n
    assert len(set(int(x) for x in air.preprocessed[:, 0])) == n  # distinct by construction
    t = good.copy()
    t[:, 1] = 0
    written, (filled,), report = MR.fill([lookup.blob], [t], RNDS[0], [(0, 0, 1, 1)], preps=[air.preprocessed])
    assert written == n and report == [] and (filled == good).all()
    # a looked-up value that no table row carries stays unmatched; every other count is the ledger's
    bad = trace(valid=False)
    t = bad.copy()
    t[:, 1] = 0
    written, (filled,), report = MR.fill([lookup.blob], [t], RNDS[0], [(0, 0, 1, 1)], preps=[air.preprocessed])
    assert written == n and len(report) == 1 and report[0][1] == (1, 0)
    lost = int(np.nonzero(air.preprocessed[:, 0] == good[3, 0])[0][0])  # the table row row 3 no longer looks up
    exp = good[:, 1].copy()
    exp[lost] -= np.uint64(1)
    assert (filled[:, 1] == exp).all()


def test_reference_refusals_and_no_slots():
    _, lookup = A.logup_air()
    t = A.logup_trace(4)
    rnd = RNDS[0]
    assert MR.fill([lookup.blob], [t], rnd, [])[2] == []
    for slots, reason in (([(0, 0, 1, 8)], "range"), ([(0, 2, 0, 2)], "range"), ([(1, 0, 1, 2)], "range"), ([(0, 0, 1, 2), (0, 0, 1, 3)], "duplicate"),
                          ([(0, 0, 1, 0)], "reader"),      # V is declared: fraction 0's denominator reads it and is no slot
                          ([(0, 0, 0, 0)], "key")):        # ... and as a slot its KEY depends on the declared column
        with pytest.raises(MR.Refused) as e:
            MR.fill([lookup.blob], [t], rnd, slots)
        assert e.value.reason == reason, slots


def test_multiplicity_slots_helper():
    _, lookup = A.logup_air()
    assert lookup.multiplicity_slots([2]) == [(0, 1, 2)]
    assert lookup.multiplicity_slots([]) == [] and lookup.multiplicity_slots([0, 1]) == []  # V and T are read by denominators only
    _, lookup, _ = A.range_air(5)
    assert lookup.multiplicity_slots([1]) == [(0, 1, 1)]
    # a next-row read is not a read of the cell's own row; a column two fractions read comes back twice, in program order
    lb = dag.LookupBuilder(3, num_cols=2, num_randomness=1)
    lb.fraction(0, lb.main(2, 1), lb.randomness(0) + lb.main(0))
    lb.fraction(1, lb.main(1) * 3 - lb.main(2), lb.randomness(0) + lb.main(0))
    lb.fraction(1, -lb.main(2), lb.randomness(0) + lb.main(0))
    assert dag.Lookup(lb, "t").multiplicity_slots([1, 2]) == [(1, 0, 1), (1, 0, 2), (1, 1, 2)]


def test_shipped_slot_tables_agree_with_the_helper():
    from miden_vm_amd import core_air as CO, precompile_airs as PA
    _, lookup = PA.byte_pair_lut_air()
    assert sorted(PA.BYTE_PAIR_LUT_MULT_SLOTS) == sorted(lookup.multiplicity_slots([0, 1, 2])) and len(PA.BYTE_PAIR_LUT_MULT_SLOTS) == 3
    assert sorted(mc for _, _, mc in PA.BYTE_PAIR_LUT_MULT_SLOTS) == [0, 1, 2]
    core_lookup = CO.core_air()[1]
    assert CO.RANGE_M_MULT_SLOTS == core_lookup.multiplicity_slots([CO.RANGE_M]) and len(CO.RANGE_M_MULT_SLOTS) == 1


def test_abi_agrees_across_header_rust_python_and_library():
    """The test that fails without the feature: the three entry points and mh_mult_slot, everywhere."""
    pkg = load_package()
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midenhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = pkg.load_library()
    for f in FILL_FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
        assert hasattr(lib, f), f
    fields = ["instance", "lookup_column", "fraction", "main_column"]
    assert [n for n, _ in pkg.MultSlot._fields_] == fields
    assert [t for _, t in pkg.MultSlot._fields_] == [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32] and C.sizeof(pkg.MultSlot) == 16
    assert re.findall(r"pub (\w+): (\w+)", re.search(r"pub struct mh_mult_slot \{(.*?)\}", rs, flags=re.S).group(1)) == \
        list(zip(fields, ["i32", "u32", "u32", "u32"]))
    body = re.search(r"typedef struct mh_mult_slot \{(.*?)\} mh_mult_slot", h, flags=re.S).group(1)
    decls = [d.split() for d in body.replace(",", " ").split(";") if d.strip()]
    assert [(d[0], n) for d in decls for n in d[1:]] == list(zip(["int32_t", "uint32_t", "uint32_t", "uint32_t"], fields))
    # the statement entries take their siblings' arguments without `flags`, plus slots / n_slots / n_written before the report
    for f, sib in (("mh_fill_multiplicities_miden_traces", "mh_check_balance_miden_traces"),
                   ("mh_fill_multiplicities_precompile_traces", "mh_check_balance_precompile_traces"), ("mh_fill_multiplicities", "mh_check_balance")):
        args = lambda name: [a.split()[-1].lstrip("*").split("[")[0]  # noqa: E731
                             for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]
        want = args(sib)
        k = want.index("flags")
        assert args(f) == want[:k] + ["slots", "n_slots", "n_written"] + want[k + 1:], f
