"""CPU-only parts of the device-built memory section (include/midenhip.h mh_memory_section_build, mh_miden_memory_section): the ABI across
header, Rust declarations, Python layer and the built library, and the rule the kernels implement (tests/memory_section_ref.py) against
testing/chiplets_trace.Memory.section(), the in-tree restatement of Memory::fill_trace."""
import ctypes as C
import os, re
import numpy as np
import pytest
import memory_section_ref as MR
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd.testing import chiplets_trace as CT  # noqa: E402

P = MR.P
FUNCS = ["mh_memory_section_build", "mh_miden_memory_section", "mh_memory_section_tile"]
INFO = [("n_rows", "uint64_t", "u64", C.c_uint64), ("n_words", "uint64_t", "u64", C.c_uint64), ("n_contexts", "uint64_t", "u64", C.c_uint64),
        ("log_n", "int32_t", "i32", C.c_int32), ("defect", "int32_t", "i32", C.c_int32), ("defect_index", "uint64_t", "u64", C.c_uint64)]
ACCESS = ["ctx", "addr", "clk", "kind", "value"]


def test_abi_agrees_across_header_rust_python_and_library():
    """The test that fails without the feature: the entry points, both structs and the Python wrappers, everywhere."""
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
    # mh_mem_section_info: 40 bytes
    body = re.search(r"typedef struct mh_mem_section_info \{(.*?)\} mh_mem_section_info", h, flags=re.S).group(1)
    assert [tuple(d.split()) for d in body.split(";") if d.strip()] == [(ct, n) for n, ct, _, _ in INFO]
    assert re.findall(r"pub (\w+): (\w+)", re.search(r"pub struct mh_mem_section_info \{(.*?)\}", rs, flags=re.S).group(1)) == \
        [(n, rt) for n, _, rt, _ in INFO]
    assert pkg.MemSectionInfo._fields_ == [(n, pt) for n, _, _, pt in INFO] and C.sizeof(pkg.MemSectionInfo) == 40
    # mh_mem_access: 48 bytes, four uint32_t then four uint64_t
    body = re.search(r"typedef struct mh_mem_access \{(.*?)\} mh_mem_access", h, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t ctx, addr, clk, kind", "uint64_t value[4]"]
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", re.search(r"pub struct mh_mem_access \{(.*?)\}", rs, flags=re.S).group(1)) == \
        [("ctx", "u32"), ("addr", "u32"), ("clk", "u32"), ("kind", "u32"), ("value", "[u64; 4]")]
    dt = pkg.MEM_ACCESS_DTYPE
    assert dt.itemsize == 48 and list(dt.names) == ACCESS
    assert [dt.fields[n][1] for n in ACCESS] == [0, 4, 8, 12, 16] and dt["value"].shape == (4,) and dt["value"].base == np.dtype("<u8")
    assert all(dt[n] == np.dtype("<u4") for n in ACCESS[:4])
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    assert args("mh_memory_section_build") == rargs("mh_memory_section_build") == ["ctx", "accesses", "n", "log_n", "out", "row_of", "info"]
    assert args("mh_miden_memory_section") == rargs("mh_miden_memory_section") == ["ctx", "chiplets", "start_row", "accesses", "n", "row_of", "info"]
    assert callable(pkg.memory_section) and callable(pkg.Miden.memory_section)
    tile = pkg.memory_section_tile(lib)
    assert tile >= 64 and tile & (tile - 1) == 0
    # the header states the precondition and what is out of scope
    sec = doc[doc.index("the memory chiplet's trace section, built on the device"):]
    assert "PRECONDITION" in sec and "Not in scope" in sec
    scope = sec[sec.index("Not in scope"):]
    for word in ("sharded", "device-resident access lists", "four chiplet sections", "arrival order", "2^24"):
        assert word in scope, word


def check_against_generator(acc):
    m = MR.replay(acc)
    rows, row_of, n_words, n_contexts = MR.section(acc)
    exp = m.section()
    assert rows.shape == exp.shape == (len(acc), 17)
    assert (rows == exp).all(), np.argwhere(rows != exp)[:8]
    assert sorted(int(r) for r in row_of) == list(range(len(acc)))
    assert n_words == sum(len(w) for w in m.trace.values()) and n_contexts == len(m.trace)
    # the additive log of the generator is the list it was played (the value slots an access ignores are zero in the log)
    used = {0: 1, 1: 0, 2: 4, 3: 0}
    assert m.accesses == [(c, a, k, kd, tuple(v[:used[kd]]) + (0,) * (4 - used[kd])) for c, a, k, kd, v in MR.records(acc)]
    back = m.access_array()
    assert back.dtype == pkg.MEM_ACCESS_DTYPE and (MR.section(back)[0] == exp).all()
    return rows, row_of


@pytest.mark.parametrize("block", range(8))
def test_rule_gives_the_generators_section_on_random_lists(block):
    """240 seeded lists of up to 60 accesses: contexts up to 2^32 - 1, words up to 2^32 - 4, a first clock of 0, several reads in one
    cycle, element and word accesses mixed on one word."""
    seen = dict(clk0=0, same_cycle=0, mixed=0, big_ctx=0, big_word=0)
    for seed in range(30 * block, 30 * block + 30):
        acc = MR.random_list(seed)
        rows, _ = check_against_generator(acc)
        seen["clk0"] += int(rows[0, 6]) == 0
        seen["same_cycle"] += bool((rows[:, 13] == 0).any())
        seen["big_ctx"] += bool((rows[:, 2] == (1 << 32) - 1).any())
        seen["big_word"] += bool((rows[:, 3] == (1 << 32) - 4).any())
        per_word = {}
        for r in rows:
            per_word.setdefault((int(r[2]), int(r[3])), set()).add(int(r[1]))
        seen["mixed"] += any(len(s) == 2 for s in per_word.values())
    assert all(v > 0 for v in seen.values()), seen


def snapshot_memory_rows(chiplets):
    return chiplets[(chiplets[:, 0] == 1) & (chiplets[:, 1] == 1) & (chiplets[:, 2] == 0)][:, 3:20]


def accesses_of_rows(rows):
    """The program-order list a section came from: by clock, the section's order within a cycle."""
    acc = []
    for r in sorted(range(rows.shape[0]), key=lambda r: (int(rows[r, 6]), r)):
        rw, ew, ctx, waddr, i0, i1, clk = (int(x) for x in rows[r, 0:7])
        idx = i0 + 2 * i1
        v = [int(x) for x in rows[r, 7:11]]
        value = (0, 0, 0, 0) if rw else (tuple(v) if ew else (v[idx], 0, 0, 0))
        acc.append((ctx, waddr + idx, clk, rw | (ew << 1), value))
    return acc


def test_rule_on_the_reference_processors_snapshots():
    """tests/golden/ref_traces.json.gz: 7 of the 27 cases hold memory rows, 14 in all; the rule and the generator rebuild them."""
    import ref_traces as RT
    cases = [c for c in RT.load_cases() if snapshot_memory_rows(c["chiplets"]).shape[0]]
    assert len(cases) == 7 and sum(snapshot_memory_rows(c["chiplets"]).shape[0] for c in cases) == 14
    for c in cases:
        rows = snapshot_memory_rows(c["chiplets"])
        acc = accesses_of_rows(rows)
        got, _ = check_against_generator(acc)
        assert (got == rows).all(), np.argwhere(got != rows)[:8]


W = (11, 12, 13, 14)


def test_scenarios_of_the_reference_memory_tests():
    """The situations the reference's own memory tests set up, as access lists written out here; the expected rows come from the
    generator and, for the cells a reader can check by eye, from the literals below."""
    # the first access at clock 0: delta 1 all the same
    rows, _ = check_against_generator([(0, 0, 0, 1, (0, 0, 0, 0))])
    assert [int(x) for x in rows[0]] == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0]
    # element and word reads of untouched memory: zeros, the element index in idx0 / idx1
    acc = [(0, 0, 1, 1, (0,) * 4), (0, 3, 2, 1, (0,) * 4), (0, 8, 3, 3, (0,) * 4), (0, 3, 4, 1, (0,) * 4), (0, 4, 5, 3, (0,) * 4)]
    rows, row_of = check_against_generator(acc)
    assert (rows[:, 7:11] == 0).all() and [int(x) for x in row_of] == [0, 1, 4, 2, 3]
    assert [int(x) for x in rows[1, 0:7]] == [1, 0, 0, 0, 1, 1, 2] and [int(x) for x in rows[4, 0:7]] == [1, 1, 0, 8, 0, 0, 3]
    assert [int(x) for x in rows[:, 14]] == [1, 1, 1, 0, 0]                      # f_scw
    assert [int(rows[r, 11]) + (int(rows[r, 12]) << 16) for r in range(5)] == [1, 1, 2, 4, 4]
    # write then read: the word after the access, element writes over a word write, another word in between
    acc = [(0, 4, 1, 2, W), (0, 6, 2, 0, (99, 0, 0, 0)), (0, 0, 3, 0, (5, 0, 0, 0)), (0, 4, 4, 3, (0,) * 4), (0, 6, 5, 1, (0,) * 4),
           (0, 1, 6, 1, (0,) * 4), (0, 4, 7, 2, (P, P + 1, (1 << 64) - 1, 0))]
    rows, row_of = check_against_generator(acc)
    assert [int(x) for x in row_of] == [2, 3, 0, 4, 5, 1, 6]
    assert [int(x) for x in rows[3, 7:11]] == [11, 12, 99, 14] == [int(x) for x in rows[5, 7:11]]
    assert [int(x) for x in rows[1, 7:11]] == [5, 0, 0, 0]
    assert [int(x) for x in rows[6, 7:11]] == [0, 1, ((1 << 64) - 1) % P, 0]
    # two contexts: the context difference is the delta, a word starts from zeros in each context
    acc = [(0, 0, 1, 2, W), (3, 0, 2, 0, (7, 0, 0, 0)), (0, 0, 3, 3, (0,) * 4), (3, 0, 4, 3, (0,) * 4), ((1 << 32) - 1, (1 << 32) - 1, 5, 1, (0,) * 4)]
    rows, row_of = check_against_generator(acc)
    assert [int(x) for x in row_of] == [0, 2, 1, 3, 4]
    assert [int(x) for x in rows[2, 7:11]] == [7, 0, 0, 0] and [int(x) for x in rows[1, 7:11]] == list(W)
    assert int(rows[2, 11]) + (int(rows[2, 12]) << 16) == 3 and int(rows[4, 11]) + (int(rows[4, 12]) << 16) == (1 << 32) - 4
    assert [int(x) for x in rows[4, 2:6]] == [(1 << 32) - 1, (1 << 32) - 4, 1, 1] and [int(x) for x in rows[4, 15:17]] == [0xFFFF, 0x3FFF]
    assert int(rows[4, 13]) == pow((1 << 32) - 4, P - 2, P)


GOOD = [(0, 0, 1, 2, W), (0, 1, 2, 1, (0,) * 4), (0, 2, 2, 1, (0,) * 4), (1, 8, 2, 0, (4, 0, 0, 0)), (0, 0, 5, 3, (0,) * 4)]


@pytest.mark.parametrize("bad,kind", [
    ((0, 6, 9, 3, (0,) * 4), 2), ((0, 5, 9, 2, W), 2),                      # unaligned word read / write
    ((0, 3, 5, 0, (1, 0, 0, 0)), 3), ((0, 0, 5, 2, W), 3),                  # a write in the cycle of a read
    ((1, 9, 2, 1, (0,) * 4), 3), ((1, 8, 2, 3, (0,) * 4), 3), ((1, 11, 2, 0, (1, 0, 0, 0)), 3)])   # anything in the cycle of a write
def test_rule_names_what_the_generator_stops_at(bad, kind):
    """Defects 2 and 3 are assertions of the generator: it stops at the access the rule names.  The lists go on after the offending
    access, with a second defect later, so that the LOWEST index is what is asked for."""
    for at in (len(GOOD), len(GOOD) + 2):
        acc = GOOD + [(2, 0, 6, 1, (0,) * 4)] * (at - len(GOOD)) + [bad, (5, 0, 9, 1, (0,) * 4), bad]
        with pytest.raises(AssertionError):
            MR.replay(acc)
        m = CT.Memory()
        stopped = None
        for i, (ctx, addr, clk, k, v) in enumerate(acc):
            try:
                [m.write, m.read, m.write_word, m.read_word][k](*([ctx, addr, clk] + ([v[0]] if k == 0 else [v] if k == 2 else [])))
            except AssertionError:
                stopped = i
                break
        assert stopped == at and len(m.accesses) == at + 1                   # the log holds the refused call as its last entry
        with pytest.raises(MR.Defect) as e:
            MR.section(acc)
        assert (e.value.kind, e.value.index) == (kind, at)
        with pytest.raises(MR.Defect) as e:
            MR.section(m.access_array())
        assert (e.value.kind, e.value.index) == (kind, at)


def test_rule_defects_the_generator_cannot_express():
    with pytest.raises(MR.Defect) as e:
        MR.section(GOOD + [(0, 0, 9, 4, (0,) * 4), (0, 1, 9, 3, (0,) * 4)])
    assert (e.value.kind, e.value.index) == (1, len(GOOD))
    with pytest.raises(MR.Defect) as e:                                      # kinds 1 and 2 come before kind 3, whatever the indices
        MR.section([(0, 0, 1, 0, (1, 0, 0, 0)), (0, 0, 1, 1, (0,) * 4), (0, 1, 9, 3, (0,) * 4)])
    assert (e.value.kind, e.value.index) == (2, 2)
    with pytest.raises(MR.Defect) as e:
        MR.section(GOOD, capacity=4)
    assert (e.value.kind, e.value.index) == (4, 4)
    assert MR.section(GOOD, capacity=5)[0].shape == (5, 17) and MR.section([])[0].shape == (0, 17)
    assert [MR.min_log_n(n) for n in (0, 1, 64, 65, 128, 129)] == [6, 6, 6, 7, 7, 8]
