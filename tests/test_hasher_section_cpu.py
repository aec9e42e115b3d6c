"""CPU-only parts of the device-built hasher controller section (include/midenhip.h mh_hasher_section_build, mh_miden_hasher_section):
the ABI across header, Rust declarations, Python layer and the built library; the encoding of Hasher.op_list(); and the rule the
kernels implement (tests/hasher_section_ref.py) against testing/chiplets_trace.Hasher.section(), the in-tree executable form of the
reference's rule, and against the reference processor's own controller rows (tests/golden/ref_traces.json.gz)."""
import ctypes as C
import os, re
import numpy as np
import pytest
import hasher_section_ref as HR
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd.testing import chiplets_trace as CT  # noqa: E402

P = HR.P
FUNCS = ["mh_hasher_section_build", "mh_miden_hasher_section", "mh_hasher_section_tile"]
INFO = [("n_rows", C.c_uint64), ("n_permutations", C.c_uint64), ("n_requests", C.c_uint64), ("mrupdate_id", C.c_uint64), ("log_n", C.c_int32),
        ("defect", C.c_int32), ("defect_index", C.c_uint64)]


def test_abi_agrees_across_header_rust_python_and_library():
    doc = open(os.path.join(ROOT, "include", "midenhip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "midenhip_sys.rs")).read()
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = pkg.load_library()
    for f in FUNCS:
        assert re.search(r"\b(int|uint32_t)\s+" + f + r"\s*\(", h), f
        assert re.search(r"pub fn " + f + r"\s*\(", rs), f
        assert f in pkg.EXPORTS, f
        assert hasattr(lib, f), f
    for name in ("mh_hash_op", "mh_hash_result", "mh_hasher_section_info"):
        assert re.search(r"typedef struct " + name + r" \{", h) and re.search(r"pub struct " + name + r" \{", rs), name
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    assert rust("mh_hash_op") == [("kind", "u32"), ("count", "u32"), ("index", "u64"), ("payload", "u64")]
    assert rust("mh_hash_result") == [("addr", "u64"), ("state", "[u64; 12]"), ("old_root", "[u64; 4]")]
    assert rust("mh_hasher_section_info") == [("n_rows", "u64"), ("n_permutations", "u64"), ("n_requests", "u64"), ("mrupdate_id", "u64"),
                                              ("log_n", "i32"), ("defect", "i32"), ("defect_index", "u64")]
    dt = pkg.HASH_OP_DTYPE
    assert dt.itemsize == 24 and list(dt.names) == ["kind", "count", "index", "payload"] and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 16]
    assert pkg.HASH_RESULT_DTYPE.itemsize == 136
    assert pkg.HasherSectionInfo._fields_ == INFO and C.sizeof(pkg.HasherSectionInfo) == 48
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    assert args("mh_hasher_section_build") == rargs("mh_hasher_section_build") == ["ctx", "ops", "n_ops", "felts", "n_felts", "log_n", "out", "results", "info"]
    assert args("mh_miden_hasher_section") == rargs("mh_miden_hasher_section") == ["ctx", "chiplets", "ops", "n_ops", "felts", "n_felts", "results", "info"]
    assert callable(pkg.hasher_section) and callable(pkg.Miden.hasher_section)
    tile = pkg.hasher_section_tile(lib)
    assert tile >= 64 and tile & (tile - 1) == 0
    sec = doc[doc.index("the hasher controller's trace section, built on the device"):]
    assert "memoised replay" in sec.lower() and "Not in scope" in sec
    scope = sec[sec.index("Not in scope"):]
    for word in ("sharded", "device-resident op lists", "bitwise", "ACE", "kernel-ROM", "decoder", "Poseidon2Air"):
        assert word in scope, word


def check_against_generator(ops, felts):
    """The rule against Hasher: rows (perm_id and padding included), the ledger, what every call returned, and op_list() back."""
    rows, results, info = HR.section(ops, felts)
    h, returned = HR.replay(ops, felts)
    exp = h.section()
    assert rows.shape == exp.shape and (rows == exp).all(), np.argwhere(rows != exp)[:8]
    assert (rows < np.uint64(P)).all()
    assert info["n_requests"] == len(h.perm_requests) and info["multiplicities"] == [m for _, m in h.perm_requests]
    assert [[int(x) for x in s] for s in info["request_states"]] == [s for s, _ in h.perm_requests]
    assert info["mrupdate_id"] == h.mrupdate_id and info["n_permutations"] == len(h.rows) // 2
    for i, (ret, (kind, _, _, _)) in enumerate(zip(returned, HR.records(ops))):
        assert int(results["addr"][i]) == ret[0]
        got = [int(x) for x in results["state"][i]]
        assert got == ret[1] if kind == HR.PERMUTE else got[0:4] == list(ret[-1])
        assert [int(x) for x in results["old_root"][i]] == (list(ret[1]) if kind == HR.UPDATE else [0] * 4)
    ops2, felts2 = h.op_list()
    assert ops2.dtype == pkg.HASH_OP_DTYPE and felts2.dtype == np.uint64
    assert [(k, c, i) for k, c, i, _ in HR.records(ops2)] == [(k, c, i) for k, c, i, _ in HR.records(ops)]
    assert (HR.section(ops2, felts2)[0] == exp).all()
    return rows


@pytest.mark.parametrize("block", range(4))
def test_op_list_replayed_through_the_rule_gives_the_generators_section(block):
    """80 seeded mixed lists: every kind, 64-bit operands, ops listed again (memoised replays), updates in the middle of the list."""
    seen = dict(mod=set(), kinds=set(), repeats=0, mru_mid=0)
    for seed in range(20 * block, 20 * block + 20):
        ops, felts = HR.random_list(seed, n_ops=10 + seed % 7)
        rows = check_against_generator(ops, felts)
        live = rows[rows[:, 0] == 1]
        seen["mod"].add(rows.shape[0] - 2 * live.shape[0])
        seen["kinds"] |= {k for k, _, _, _ in HR.records(ops)}
        seen["repeats"] += len(set(int(x) for x in live[:, 19])) < live.shape[0]
        seen["mru_mid"] += len(set(int(x) for x in live[:, 16])) > 2
    assert seen["kinds"] == {0, 1, 2, 3, 4} and seen["mod"] == {0, 2, 4, 6} and seen["repeats"] and seen["mru_mid"], seen


def test_sample_chiplets_log_their_hasher_calls():
    for seed in range(3):
        c = CT.sample_chiplets(seed=seed, merkle_depth=3 + seed)
        ops, felts = c.hasher.op_list()
        rows, _, info = HR.section(ops, felts)
        assert (rows == c.hasher.section()).all() and info["n_requests"] == len(c.hasher.perm_requests)


def test_hand_written_lists():
    """What a reader can check by eye: depth 64, index corners, x and x + p as one state, an update with old == new."""
    w = lambda a: [a, a + 1, a + 2, a + 3]  # noqa: E731
    path = [w(10 * j) for j in range(64)]
    flat = [x for s in path for x in s]
    felts = w(7) + flat
    rows = check_against_generator(np.array([(3, 64, P - 1, 0), (3, 64, 0, 0), (3, 1, 1, 0), (3, 2, 3, 0)], dtype=HR.DT), felts)
    assert int(rows[0, 15]) == P - 1 and int(rows[127, 15]) == 0 and int(rows[126, 15]) == (P - 1) >> 63 and int(rows[127, 18]) == 0
    small = [5, 2 ** 32 - 2, 0, 1] * 3
    felts = small + [x + P for x in small]
    rows = check_against_generator(np.array([(0, 0, 0, 0), (0, 0, 0, 12), (0, 0, 0, 0)], dtype=HR.DT), felts)
    assert [int(x) for x in rows[:6, 19]] == [0] * 6 and (rows[0] == rows[2]).all()
    felts = w(1) + w(1) + w(20) + w(30)
    rows = check_against_generator(np.array([(3, 2, 2, 4), (4, 2, 2, 0), (2, 1, 0, 0)], dtype=HR.DT), felts)
    assert [int(x) for x in rows[0:12:2, 19]] == [0, 1, 0, 1, 0, 1] and [int(x) for x in rows[:, 16]] == [0] * 4 + [1] * 12
    assert [int(x) for x in rows[12, 0:3]] == [1, 0, 0] and [int(x) for x in rows[14, 0:3]] == [0, 1, 0]


# ---- the reference processor's own controller rows ----
def ops_of_rows(rows):
    """The op list a controller section came from: permutations are segmented by the boundary flags, the kind is read from the
    selectors.  A RETURN_HASH permutation with boundary 1 / 1 is a control block (capacity 0, d, 0, 0) -- a one-batch basic block is the
    same rows with d = 0."""
    ops, felts, p, n = [], [], 0, rows.shape[0] // 2
    cell = lambda r, c: int(rows[r, c])  # noqa: E731
    state = lambda r: [int(x) for x in rows[r, 3:15]]  # noqa: E731
    while p < n and cell(2 * p, 0) == 1:
        sel = tuple(cell(2 * p, c) for c in range(3))
        assert cell(2 * p, 17) == 1, "an op starts on a boundary row"
        q = p
        while cell(2 * q + 1, 17) == 0:
            q += 1
        count = q - p + 1
        if sel == CT.LINEAR_HASH:
            s = state(2 * p)
            if count == 1 and cell(2 * p + 1, 2) == 1:
                ops.append((0, 0, 0, len(felts)))
                felts += s
            elif count == 1:
                assert s[8] == 0 and s[10:12] == [0, 0]
                ops.append((1, 0, s[9], len(felts)))
                felts += s[0:8]
            else:
                assert s[8:12] == [0] * 4
                ops.append((2, count, 0, len(felts)))
                felts += [x for j in range(p, q + 1) for x in state(2 * j)[0:8]]
            p = q + 1
            continue
        halves = lambda j: (state(2 * j)[4:8], state(2 * j)[0:4]) if cell(2 * j, 18) else (state(2 * j)[0:4], state(2 * j)[4:8])  # noqa: E731
        index, value = cell(2 * p, 15), halves(p)[0]
        siblings = [x for j in range(p, q + 1) for x in halves(j)[1]]
        if sel == CT.MP_VERIFY:
            ops.append((3, count, index, len(felts)))
            felts += value + siblings
            p = q + 1
            continue
        assert sel == CT.MR_UPDATE_OLD and tuple(cell(2 * (q + 1), c) for c in range(3)) == CT.MR_UPDATE_NEW
        new_value = halves(q + 1)[0]
        assert [x for j in range(q + 1, q + 1 + count) for x in halves(j)[1]] == siblings and cell(2 * (q + 1), 15) == index
        ops.append((4, count, index, len(felts)))
        felts += value + new_value + siblings
        p = q + 1 + count
    return np.array(ops, dtype=HR.DT), np.array(felts, dtype=np.uint64)


def test_rule_rebuilds_the_reference_processors_controller_rows():
    """The 27 snapshots: the controller rows (column 0 = 0, selector s0 or the (0, 1, 0) padding) recovered into op lists, rebuilt cell
    for cell, perm_id and padding included."""
    import ref_traces as RT
    cases = RT.load_cases()
    assert len(cases) == 27
    kinds, total = set(), 0
    for c in cases:
        chip = c["chiplets"]
        rows = chip[chip[:, 0] == 0][:, 1:21]
        assert rows.shape[0] and rows.shape[0] % 8 == 0
        ops, felts = ops_of_rows(rows)
        got = check_against_generator(ops, felts)
        assert got.shape == rows.shape and (got == rows).all(), np.argwhere(got != rows)[:8]
        kinds |= {k for k, _, _, _ in HR.records(ops)}
        total += rows.shape[0]
    assert {1, 2} <= kinds and total >= 27 * 8, (kinds, total)


# ---- defects ----
GOOD_FELTS = list(range(100, 160))
GOOD = [(0, 0, 0, 0), (3, 2, 3, 12), (2, 2, 0, 4), (4, 3, 5, 20), (1, 0, 9, 40)]


@pytest.mark.parametrize("bad,kind", [
    ((5, 1, 0, 0), 1), ((0xFFFFFFFF, 0, 0, 0), 1),
    ((2, 0, 0, 0), 2), ((3, 0, 0, 0), 2), ((4, 65, 0, 0), 2),
    ((3, 2, 4, 0), 3), ((4, 63, 1 << 63, 0), 3), ((3, 64, P, 0), 3), ((4, 64, (1 << 64) - 1, 0), 3),
    ((0, 0, 0, 49), 4), ((1, 0, 0, 53), 4), ((2, 8, 0, 0), 4), ((3, 15, 0, 0), 4), ((4, 13, 0, 1), 4), ((0, 0, 0, 1 << 63), 4),
    ((2, 0xFFFFFFFF, 0, (1 << 64) - 1), 4)])
def test_rule_refuses_the_lowest_defective_op(bad, kind):
    """The lists go on after the offending op, with another defect later, so that the LOWEST index is what is asked for; where the
    generator can express the op it stops there too."""
    for at in (0, 3, len(GOOD)):
        ops = GOOD[:at] + [bad] + GOOD[at:] + [(7, 0, 0, 0), bad]
        if bad == (2, 0xFFFFFFFF, 0, (1 << 64) - 1):
            with pytest.raises(HR.TooMany):
                HR.section(np.array(ops, dtype=HR.DT), GOOD_FELTS)
            continue
        with pytest.raises(HR.Defect) as e:
            HR.section(np.array(ops, dtype=HR.DT), GOOD_FELTS)
        assert (e.value.kind, e.value.index) == (kind, at)
        if kind in (2, 3) and bad[1] <= 12 and bad[2] < P:
            with pytest.raises((AssertionError, IndexError)):
                HR.replay(np.array(ops[:at + 1], dtype=HR.DT), GOOD_FELTS)


def test_rule_edges_that_are_no_defects_and_the_fit():
    ops = np.array(GOOD, dtype=HR.DT)
    rows, _, info = HR.section(ops, GOOD_FELTS)
    assert info["n_permutations"] == 1 + 2 + 2 + 6 + 1 and rows.shape == (24, 20) and info["mrupdate_id"] == 1
    HR.section(np.array([(0, 0, 0, 48), (3, 14, (1 << 14) - 1, 0), (2, 7, 0, 4)], dtype=HR.DT), GOOD_FELTS)   # operands end at the last felt
    HR.section(np.array([(3, 64, P - 1, 0)], dtype=HR.DT), list(range(260)))
    for cap, index in ((0, 0), (2, 1), (5, 1), (6, 2), (21, 3), (22, 4), (23, 4)):
        with pytest.raises(HR.Defect) as e:
            HR.section(ops, GOOD_FELTS, cap_rows=cap)
        assert (e.value.kind, e.value.index) == (5, index)
    assert HR.section(ops, GOOD_FELTS, cap_rows=24)[0].shape == (24, 20)
    with pytest.raises(HR.Defect) as e:                                  # the rows fit, the padding does not
        HR.section(ops[:2], GOOD_FELTS, cap_rows=6)
    assert (e.value.kind, e.value.index) == (5, 2)
    with pytest.raises(HR.Defect) as e:                                  # defects 1..4 come before the fit
        HR.section(np.array(GOOD + [(9, 0, 0, 0)], dtype=HR.DT), GOOD_FELTS, cap_rows=2)
    assert (e.value.kind, e.value.index) == (1, len(GOOD))
    empty = HR.section(np.zeros(0, dtype=HR.DT), [])
    assert empty[0].shape == (0, 20) and empty[2]["n_requests"] == 0
    assert [HR.min_log_n(n) for n in (0, 8, 64, 72, 128, 136)] == [6, 6, 6, 7, 7, 8]
