"""CPU-only parts of the device-built Poseidon2 permutation trace (include/midenhip.h mh_poseidon2_trace_build,
mh_miden_poseidon2_trace): the ABI across header, Rust declarations, Python layer and the built library, and the scan rule the kernel
implements (tests/p2_trace_ref.py) against the request ledgers of the test generators."""
import ctypes as C
import os, re
import numpy as np
import pytest
import p2_trace_ref as PR
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd import miden_air as MA  # noqa: E402
from miden_vm_amd.testing import chiplets_trace as CT  # noqa: E402

FUNCS = ["mh_poseidon2_trace_build", "mh_miden_poseidon2_trace"]
FIELDS = [("n_requests", "uint64_t", "u64", C.c_uint64), ("n_input_rows", "uint64_t", "u64", C.c_uint64), ("log_n", "int32_t", "i32", C.c_int32),
          ("defect", "int32_t", "i32", C.c_int32), ("defect_row", "uint64_t", "u64", C.c_uint64)]


def sample(seed):
    """every section present: memory rows (column 1 = 1 under column 0 = 1), bitwise, ACE, kernel ROM, controller padding"""
    return CT.sample_chiplets(seed=seed, n_hperm=3 + seed % 3, n_bitwise=5 + seed, n_mem=12 + 4 * seed, merkle_depth=3 + seed % 2)


def test_abi_agrees_across_header_rust_python_and_library():
    """The test that fails without the feature: both entry points, the info struct and the Python wrappers, everywhere."""
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midenhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = pkg.load_library()
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
        assert hasattr(lib, f), f
    body = re.search(r"typedef struct mh_p2_trace_info \{(.*?)\} mh_p2_trace_info", h, flags=re.S).group(1)
    assert [tuple(d.split()) for d in body.split(";") if d.strip()] == [(ct, n) for n, ct, _, _ in FIELDS]
    assert re.findall(r"pub (\w+): (\w+)", re.search(r"pub struct mh_p2_trace_info \{(.*?)\}", rs, flags=re.S).group(1)) == \
        [(n, rt) for n, _, rt, _ in FIELDS]
    assert pkg.P2TraceInfo._fields_ == [(n, pt) for n, _, _, pt in FIELDS] and C.sizeof(pkg.P2TraceInfo) == 32
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    assert args("mh_poseidon2_trace_build") == ["ctx", "states", "multiplicities", "k", "log_n", "out", "info"]
    assert args("mh_miden_poseidon2_trace") == ["ctx", "chiplets", "log_n", "out", "info"]
    assert callable(pkg.poseidon2_trace) and callable(pkg.Miden.poseidon2_trace)
    # the header says what is out of scope
    doc = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    sec = doc[doc.index("the Poseidon2 permutation trace of the Miden statement"):]
    assert "Not in scope" in sec and "Poseidon2Air" in sec and "sharded" in sec


@pytest.mark.parametrize("seed", range(8))
def test_scan_rule_gives_the_hasher_ledger(seed):
    c = sample(seed)
    t, p2 = c.into_traces()
    assert (t[:, 0] == 1).any() and ((t[:, 0] == 1) & (t[:, 1] == 1)).any()        # memory-like rows the rule must ignore
    assert ((t[:, 0] == 0) & (t[:, 1] == 0) & (t[:, 2] == 1) & (t[:, 3] == 0)).any() or len(c.hasher.rows) % 8 == 0  # controller padding
    states, mult, n_in = PR.scan(t)
    ledger = c.hasher.perm_requests
    assert n_in == len(c.hasher.rows) // 2 == sum(m for _, m in ledger)
    assert [[int(x) for x in s] for s in states] == [s for s, _ in ledger]         # states, in first-occurrence order
    assert [int(m) for m in mult] == [m for _, m in ledger] and max(int(m) for m in mult) >= 2
    k = len(ledger)
    assert (MA.poseidon2_permutation_trace(PR.min_log_n(k), states, mult) == p2).all()


@pytest.mark.parametrize("log_n", [8, 11])
def test_scan_rule_on_the_bulk_generator(log_n):
    t, p2 = CT.bulk_chiplets(log_n)
    states, mult, n_in = PR.scan(t)
    k = (1 << log_n) // 16 - 1
    assert n_in == k == states.shape[0] and (mult == 1).all()
    assert (states == p2[0::16][:k, MA.COL_STATE:MA.COL_STATE + 12]).all() and (p2[0::16][k:, MA.COL_WITNESS] == 0).all()
    assert (MA.poseidon2_permutation_trace(log_n, states, mult) == p2).all()


def test_scan_rule_on_the_reference_processors_snapshots():
    """The chiplets traces the reference processor wrote (tests/golden/ref_traces.json.gz): the rule gives the Poseidon2 permutation
    trace the processor wrote next to them, all 27 cases."""
    import ref_traces as RT
    cases = RT.load_cases()
    assert len(cases) == 27
    for i, c in enumerate(cases):
        states, mult, _ = PR.scan(c["chiplets"])
        log_n = c["poseidon2"].shape[0].bit_length() - 1
        assert log_n == PR.min_log_n(states.shape[0]), i
        assert (MA.poseidon2_permutation_trace(log_n, states, mult) == c["poseidon2"]).all(), i


def test_reference_names_the_lowest_defect():
    t, _ = sample(1).into_traces()
    rows = PR.input_rows(t)
    ids = t[rows, PR.COL_PERM_ID]
    later = int([r for r in rows if (ids == t[r, PR.COL_PERM_ID]).sum() > 1][-1])   # the last row of a repeated id is not its first
    bad = t.copy()
    bad[later, PR.COL_STATE + 5] ^= np.uint64(1)
    with pytest.raises(PR.Defect) as e:
        PR.scan(bad)
    assert (e.value.kind, e.value.row) == (3, later)
    bad = t.copy()
    last = int(rows[ids == ids.max()][0])
    bad[last:last + 2, PR.COL_PERM_ID] += np.uint64(1)
    with pytest.raises(PR.Defect) as e:
        PR.scan(bad)
    assert (e.value.kind, e.value.row) == (2, int(ids.max()))
    bad[rows[2], PR.COL_PERM_ID] = 1 << 40
    with pytest.raises(PR.Defect) as e:
        PR.scan(bad)
    assert (e.value.kind, e.value.row) == (1, int(rows[2]))
    assert PR.min_log_n(0) == 6 and PR.min_log_n(3) == 6 and PR.min_log_n(4) == 7 and PR.min_log_n(63) == 10 and PR.min_log_n(64) == 11
