"""CPU-only parts of the device-built bitwise, ACE and kernel-ROM sections and of the whole chiplets trace (include/midenhip.h
mh_bitwise_section_build .. mh_miden_chiplets_build): the ABI across header, Rust declarations, Python layer and the built library; the
generator's lists (Ace.eval_list, KernelRom's call log, Chiplets.lists); and the rules the kernels implement (tests/
bitwise_section_ref.py, ace_section_ref.py, kernel_rom_section_ref.py, chiplets_frame_ref.py) against testing/chiplets_trace, the
in-tree executable form of the reference's rules, against the reference processor's snapshots (tests/golden/ref_traces.json.gz) and
against the situations of the reference's own chiplet tests (tests/golden/chiplet_section_scenarios.json)."""
import ctypes as C
import json, os, re
import numpy as np
import pytest
import ace_section_ref as AR
import bitwise_section_ref as BR
import chiplets_frame_ref as FR
import hasher_section_ref as HR
import kernel_rom_section_ref as KR
import memory_section_ref as MR
from __graft_entry__ import load_package, ROOT

pkg = load_package()
from miden_vm_amd.testing import chiplets_trace as CT  # noqa: E402

P = AR.P
FUNCS = ["mh_bitwise_section_build", "mh_miden_bitwise_section", "mh_ace_section_build", "mh_miden_ace_section", "mh_ace_section_tile",
         "mh_kernel_rom_section_build", "mh_miden_kernel_rom_section", "mh_miden_chiplets_build", "mh_miden_chiplets_frame"]


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
    structs = ("mh_bitwise_op", "mh_bitwise_section_info", "mh_ace_eval", "mh_ace_section_info", "mh_kernel_rom_section_info",
               "mh_chiplets_lists", "mh_chiplets_info")
    for name in structs:
        assert re.search(r"typedef struct " + name + r" \{", h) and re.search(r"pub struct " + name + r" \{", rs), name
    rust = lambda name: re.findall(r"pub (\w+): ([\w\[\]; *]+),", re.search(r"pub struct " + name + r" \{(.*?)\}", rs, flags=re.S).group(1))  # noqa: E731
    assert rust("mh_bitwise_op") == [("op", "u32"), ("a", "u32"), ("b", "u32")]
    assert rust("mh_ace_eval") == [("ctx", "u32"), ("ptr", "u32"), ("clk", "u32"), ("num_vars", "u32"), ("num_eval", "u32"), ("reserved", "u32"),
                                   ("payload", "u64")]
    kinds = {"u32": C.c_uint32, "u64": C.c_uint64, "i32": C.c_int32, "[u64; 5]": C.c_uint64 * 5}
    infos = {"mh_bitwise_section_info": pkg.BitwiseSectionInfo, "mh_ace_section_info": pkg.AceSectionInfo,
             "mh_kernel_rom_section_info": pkg.KernelRomSectionInfo, "mh_hasher_section_info": pkg.HasherSectionInfo,
             "mh_mem_section_info": pkg.MemSectionInfo}
    for name, cls in infos.items():
        assert [(f, kinds[t]) for f, t in rust(name)] == list(cls._fields_), name
    ci = [(f, kinds[t] if t in kinds else infos[t]) for f, t in rust("mh_chiplets_info")]
    assert ci == list(pkg.ChipletsInfo._fields_)
    assert [f for f, _ in rust("mh_chiplets_lists")] == [f for f, _ in pkg.ChipletsLists._fields_]
    dt = pkg.BITWISE_OP_DTYPE
    assert dt.itemsize == 12 and list(dt.names) == ["op", "a", "b"] and dt == BR.DT
    dt = pkg.ACE_EVAL_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24] and dt == AR.DT
    assert C.sizeof(pkg.BitwiseSectionInfo) == 24 and C.sizeof(pkg.AceSectionInfo) == 56 and C.sizeof(pkg.KernelRomSectionInfo) == 32
    assert C.sizeof(pkg.ChipletsLists) == 16 * 8
    assert C.sizeof(pkg.ChipletsInfo) == 7 * 8 + 16 + 8 + 48 + 24 + 40 + 56 + 32
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", h, flags=re.S).group(1).split(",")]  # noqa: E731
    rargs = lambda name: re.findall(r"(\w+): ", re.search(r"pub fn " + name + r"\s*\((.*?)\)", rs, flags=re.S).group(1))  # noqa: E731
    want = {
        "mh_bitwise_section_build": ["ctx", "ops", "n_ops", "log_n", "out", "results", "info"],
        "mh_miden_bitwise_section": ["ctx", "chiplets", "start_row", "ops", "n_ops", "results", "info"],
        "mh_ace_section_build": ["ctx", "evals", "n_evals", "felts", "n_felts", "log_n", "out", "info"],
        "mh_miden_ace_section": ["ctx", "chiplets", "start_row", "evals", "n_evals", "felts", "n_felts", "info"],
        "mh_kernel_rom_section_build": ["ctx", "procs", "n_procs", "calls", "n_calls", "log_n", "out", "digests", "info"],
        "mh_miden_kernel_rom_section": ["ctx", "chiplets", "start_row", "procs", "n_procs", "calls", "n_calls", "digests", "info"],
        "mh_miden_chiplets_build": ["ctx", "lists", "log_n", "out", "info"],
        "mh_miden_chiplets_frame": ["ctx", "chiplets", "padding_start"],
    }
    for name, a in want.items():
        assert args(name) == rargs(name) == a, name
    for name in ("bitwise_section", "ace_section", "kernel_rom_section"):
        assert callable(getattr(pkg, name)) and callable(getattr(pkg.Miden, name)), name
    assert callable(pkg.Miden.chiplets_frame) and callable(pkg.Miden.chiplets_build)
    tile = pkg.ace_section_tile(lib)
    assert tile >= 64 and tile & (tile - 1) == 0
    sec = doc[doc.index("the bitwise, ACE and kernel-ROM sections, and the whole chiplets trace, built on the device"):]
    assert "waits up to 8 times" in sec and "SyscallTargetNotInKernel" in sec and "n_rounds" in sec
    scope = sec[sec.index("Not in scope"):]
    for word in ("sharded contexts", "device-resident lists", "deriving the lists from a program", "memory accesses an evaluation", "precompile prover"):
        assert word in scope, word
    # the two earlier sections keep their words
    for title in ("the memory chiplet's trace section, built on the device", "the hasher controller's trace section, built on the device"):
        old = doc[doc.index(title):]
        old = old[old.index("Not in scope"):old.index("*/")]
        for word in ("bitwise", "ACE"):
            assert word in old, (title, word)


def test_no_product_source_computes_the_sections_on_the_host():
    """The library never evaluates a circuit or sorts digests on the host: the new stages hold kernels, and their host code has no
    sort and no field product."""
    for name in ("bitwise_section.hip", "ace_section.hip", "kernel_rom_section.hip", "chiplets_build.hip"):
        src = open(os.path.join(ROOT, "miden-vm_amd", "csrc", name)).read()
        assert "__global__" in src, name
        host = src[src.index("// ---- host ----"):] if "// ---- host ----" in src else ""
        assert "std::sort" not in src and "qsort" not in src and "e2_mul" not in host and "gl_mul" not in host, name


# ---- the rules against the generator ----
def sample(seed, **kw):
    rng = np.random.default_rng(1000 + seed)
    kw.setdefault("n_bitwise", int(rng.integers(0, 12)))
    kw.setdefault("kernel_procs", int(rng.integers(0, 6)))
    procs = kw["kernel_procs"]
    kw.setdefault("syscalls", tuple(int(x) for x in rng.integers(0, 4, procs)))
    kw.setdefault("ace", bool(seed % 3))
    return CT.sample_chiplets(seed=seed, **kw)


def ref_sections(lists, log_n=None):
    """The five rules on one set of lists -> what chiplets_frame_ref.stack gives."""
    h_rows = HR.section(lists["hash_ops"], lists["hash_felts"])[0] if len(lists["hash_ops"]) else np.zeros((0, 20), dtype=np.uint64)
    m_rows = MR.section(lists["mem_accesses"])[0] if len(lists["mem_accesses"]) else np.zeros((0, 17), dtype=np.uint64)
    secs = [h_rows, BR.section(lists["bitwise_ops"])[0], m_rows, AR.section(lists["ace_evals"], lists["ace_felts"])[0],
            KR.section(lists["kernel_procs"], lists["kernel_calls"])[0]]
    return FR.stack(secs, log_n)


@pytest.mark.parametrize("seed", range(30))
def test_rules_equal_the_generator_on_seeded_programs(seed):
    c = sample(seed)
    lists = c.lists()
    rows, results = BR.section(lists["bitwise_ops"])
    assert (rows == c.bitwise.section()).all() and rows.shape == c.bitwise.section().shape
    assert [int(x) for x in results] == [(a & b) if op == 0 else (a ^ b) for op, a, b in c.bitwise.ops]
    rows, info = AR.section(lists["ace_evals"], lists["ace_felts"])
    assert rows.shape == c.ace.section().shape and (rows == c.ace.section()).all()
    rows, digests = KR.section(lists["kernel_procs"], lists["kernel_calls"])
    assert rows.shape == c.kernel_rom.section().shape and (rows == c.kernel_rom.section()).all()
    assert [[int(x) for x in d] for d in digests] == c.kernel_rom.digests()
    t, st, pad, trace_len = ref_sections(lists)
    exp = c.into_traces()[0]
    assert t.shape == exp.shape and (t == exp).all(), np.argwhere(t != exp)[:8]
    assert trace_len == c.trace_len() and pad == trace_len - 1
    assert (t < np.uint64(P)).all()


def test_rules_on_hand_written_lists():
    # bitwise: the corners of the operands, both ops
    vals = [0, 1, 0xFFFFFFFF, 0x80000000, 0x12345678]
    b = CT.Bitwise()
    for x in vals:
        for y in vals:
            b.u32and(x, y)
            b.u32xor(x, y)
    rows, _ = BR.section(np.array(b.ops, dtype=BR.DT))
    assert (rows == b.section()).all()
    assert [int(x) for x in rows[7]] == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    # kernel ROM: byte order against numeric order, equal prefixes, duplicates, x + p
    procs = [[0x0001, 0, 0, 0], [0x0100, 0, 0, 0], [5, 5, 5, 9], [5, 5, 5, 8], [0x0100, 0, 0, 0], [P + 5, 5, 5, 9]]
    k = CT.KernelRom([[x % P for x in d] for d in procs])   # the generator keys a digest by the bytes it is handed
    calls = [procs[1], procs[0], procs[1], [5, 5, 5, P + 8]]
    for d in calls:
        k.access_proc([x % P for x in d])
    rows, digests = KR.section(procs, calls)
    assert (rows == k.section()).all() and rows.shape[0] == 4
    assert [int(x) for x in rows[:, 1]] == [0x0100, 0x0001, 5, 5] and [int(x) for x in rows[:, 0]] == [2, 1, 1, 0]
    assert [int(x) for x in rows[2:, 4]] == [8, 9]
    # ACE: several evaluations through the generator's memory, clock order
    rng = np.random.default_rng(7)
    circuits = [AR.sized_circuit(rng, 2, 4), AR.chain_circuit(rng, 8), AR.flat_circuit(rng, 12), AR.random_circuit(rng, 5, 30)]
    evals, felts = AR.make_list(circuits, ctx=3, ptr=64, clk0=100)
    ace = CT.Ace()
    for e in evals[::-1]:   # executed out of clock order: the section sorts by clock
        at, nv, ne = int(e["payload"]), int(e["num_vars"]), int(e["num_eval"])
        mem, tick = CT.Memory(), 1   # a memory per evaluation: they all sit at one address
        for i in range(nv // 2):
            mem.write_word(3, 64 + 4 * i, tick, [int(x) for x in felts[at + 4 * i:at + 4 * i + 4]])
            tick += 1
        for k_ in range(ne):
            mem.write(3, 64 + 2 * nv + k_, tick, int(felts[at + 2 * nv + k_]))
            tick += 1
        ace.eval_circuit(mem, 3, 64, int(e["clk"]), nv, ne)
    rows, info = AR.section(evals, felts)
    assert (rows == ace.section()).all() and rows.shape == ace.section().shape
    ev2, f2 = ace.eval_list()
    assert (ev2["clk"] == evals["clk"]).all() and (AR.section(ev2, f2)[0] == rows).all()
    assert info["n_gates"] == sum(int(e["num_eval"]) for e in evals) and info["n_rows"] == rows.shape[0]


def test_round_counts_of_the_two_extreme_circuits():
    rng = np.random.default_rng(3)
    for n in (4, 64, 68, 128, 132):
        assert AR.section(*AR.make_list([AR.chain_circuit(rng, n)]))[1]["n_rounds"] == n
        assert AR.section(*AR.make_list([AR.flat_circuit(rng, n)]))[1]["n_rounds"] == -(-n // 64)


# ---- the reference processor's snapshots ----
def snapshot_sections(chiplets):
    t = chiplets
    bw = t[(t[:, 0] == 1) & (t[:, 1] == 0)][:, 2:15]
    ace = t[(t[:, 0] == 1) & (t[:, 1] == 1) & (t[:, 2] == 1) & (t[:, 3] == 0)][:, 4:20]
    kr = t[(t[:, 0] == 1) & (t[:, 1] == 1) & (t[:, 2] == 1) & (t[:, 3] == 1) & (t[:, 4] == 0)][:, 5:10]
    return bw, ace, kr


def lists_of_rows(bw, ace, kr):
    ops = np.array([(int(bw[8 * k, 0]), int(bw[8 * k + 7, 1]), int(bw[8 * k + 7, 2])) for k in range(bw.shape[0] // 8)], dtype=BR.DT)
    evals, felts, r = [], [], 0
    while r < ace.shape[0]:
        assert ace[r, 0] == 1
        n = r + 1
        while n < ace.shape[0] and ace[n, 0] == 0:
            n += 1
        block = ace[r:n]
        reads, gates = block[block[:, 1] == 0], block[block[:, 1] == 1]
        evals.append((int(block[0, 2]), int(block[0, 3]), int(block[0, 4]), 2 * len(reads), len(gates), 0, len(felts)))
        for x in reads:
            felts += [int(x[7]), int(x[8]), int(x[10]), int(x[11])]
        for x in gates:
            felts.append(AR.encode(int(x[9]), int(x[12]), {P - 1: 0, 0: 1, 1: 2}[int(x[5])]))
        r = n
    procs = kr[:, 1:5]
    calls = np.repeat(procs, [int(m) for m in kr[:, 0]], axis=0)
    return ops, np.array(evals, dtype=AR.DT), np.array(felts, dtype=np.uint64), procs[::-1], calls


def test_rules_on_the_reference_processors_snapshots():
    """tests/golden/ref_traces.json.gz: 2 of the 27 cases hold kernel-ROM rows, none holds bitwise or ACE rows (SNAPSHOT_CASES); the
    rules rebuild every such row from the lists read off the rows (procedures handed over in reverse trace order, so the sort has work
    to do).  The bitwise and ACE rules therefore rest on the generator and on the scenarios below."""
    import ref_traces as RT
    held = {"bitwise": 0, "ace": 0, "kernel_rom": 0}
    for c in RT.load_cases():
        bw, ace, kr = snapshot_sections(c["chiplets"])
        ops, evals, felts, procs, calls = lists_of_rows(bw, ace, kr)
        held["bitwise"] += bool(bw.shape[0])
        held["ace"] += bool(ace.shape[0])
        held["kernel_rom"] += bool(kr.shape[0])
        assert bw.shape[0] % 8 == 0 and (BR.section(ops)[0] == bw).all()
        assert (AR.section(evals, felts)[0] == ace).all()
        assert (KR.section(procs, calls)[0] == kr).all()
    print("snapshot cases with rows:", held)
    assert held == SNAPSHOT_CASES, held


# counted on the fixture: none of the 27 programs uses the bitwise or the ACE chiplet; cases 13 and 14 (SYSCALL) declare a kernel
SNAPSHOT_CASES = {"bitwise": 0, "ace": 0, "kernel_rom": 2}


# ---- the reference's own chiplet tests, as data ----
def test_scenarios_of_the_reference_chiplet_tests():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "chiplet_section_scenarios.json")))
    for s in doc["bitwise"]:
        rows, results = BR.section(np.array([tuple(o) for o in s["ops"]], dtype=BR.DT))
        assert rows.shape[0] == 8 * len(s["ops"])
        for k, (op, a, b) in enumerate(s["ops"]):
            assert int(results[k]) == ((a & b) if op == 0 else (a ^ b)) == int(rows[8 * k + 7, 12])
            for i in range(8):                      # check_decomposition: the bits of a row rebuild its a and b
                r = rows[8 * k + i]
                assert sum(int(r[3 + j]) << j for j in range(4)) == int(r[1]) & 0xF and sum(int(r[7 + j]) << j for j in range(4)) == int(r[2]) & 0xF
                assert int(r[1]) == a >> (28 - 4 * i) and int(r[2]) == b >> (28 - 4 * i) and int(r[11]) == (int(rows[8 * k + i - 1, 12]) if i else 0)
    for s in doc["kernel_rom"]:
        if "defect" in s:
            with pytest.raises(KR.Defect) as e:
                KR.section(s["procs"], s["calls"])
            assert [e.value.kind, e.value.index] == s["defect"]
        else:
            assert KR.section(s["procs"], s["calls"])[0].tolist() == s["rows"]
    for s in doc["ace"]:
        felts = [x for w in s["words"] for x in w] + [AR.encode(*i) for i in s["instructions"]]
        evals = np.array([(0, 0, 1, s["num_vars"], s["num_eval"], 0, 0)], dtype=AR.DT)
        rows, info = AR.section(evals, felts)
        assert rows.shape[0] == s["num_vars"] // 2 + s["num_eval"] and not rows[-1, 7:9].any(), s["name"]
        # verify_trace: the multiplicities of an evaluation sum to twice its gates
        assert int(rows[:s["num_vars"] // 2, 14:16].sum()) + int(rows[s["num_vars"] // 2:, 15].sum()) == 2 * s["num_eval"]


# ---- defects ----
def expect(mod, kind, index, fn, gate=None):
    with pytest.raises(mod.Defect) as e:
        fn()
    assert (e.value.kind, e.value.index) == (kind, index), (e.value.kind, e.value.index)
    if gate is not None:
        assert e.value.gate == gate


def test_every_defect_kind_is_named_with_its_index():
    ops = np.zeros(5, dtype=BR.DT)
    ops["op"] = [0, 2, 1, 3, 0]
    expect(BR, 1, 1, lambda: BR.section(ops))
    ops["op"] = [0, 1, 1, 0, 7]
    expect(BR, 1, 4, lambda: BR.section(ops))
    expect(BR, 2, 3, lambda: BR.section(np.zeros(5, dtype=BR.DT), cap_rows=31))
    procs = [[1, 2, 3, 4], [5, 6, 7, 8]]
    expect(KR, 1, 0, lambda: KR.section(procs, [[9, 9, 9, 9], procs[0]]))
    expect(KR, 1, 2, lambda: KR.section(procs, [procs[0], procs[1], [1, 2, 3, 5]]))
    expect(KR, 2, 1, lambda: KR.section(procs, [], cap_rows=1))
    rng = np.random.default_rng(11)
    good = lambda: AR.make_list([AR.sized_circuit(rng, 4, 8) for _ in range(3)])  # noqa: E731
    for at in (0, 2):
        for field, value in (("num_vars", 0), ("num_vars", 3), ("num_eval", 0), ("num_eval", 6), ("num_vars", 1 << 30)):
            ev, f = good()
            ev[field][at] = value
            expect(AR, 1, at, lambda: AR.section(ev, f))
    ev, f = good()
    ev["clk"][2] = ev["clk"][1]
    expect(AR, 2, 2, lambda: AR.section(ev, f))
    ev, f = good()
    ev["payload"][2] += 1
    expect(AR, 3, 2, lambda: AR.section(ev, f))
    ev, f = good()
    ev["ptr"][0] = (1 << 32) - 15          # 2 * 4 + 8 = 16 addresses
    expect(AR, 3, 0, lambda: AR.section(ev, f))
    ev["ptr"][0] = (1 << 32) - 16
    AR.section(ev, f)
    for at in (0, 2):
        nw, base = 12, None
        for gate, ins in ((0, AR.encode(11, 10, 3)), (3, AR.encode(4, 11, 1)), (2, AR.encode(12, 11, 2)), (7, AR.encode(0, 11, 0))):
            ev, f = good()
            f[int(ev["payload"][at]) + 8 + gate] = ins   # opcode 3; the gate itself (id 7 - 3 = 4); an id of nw; the last gate itself
            expect(AR, 4, at, lambda: AR.section(ev, f), gate=gate)
    ev, f = good()
    expect(AR, 5, 1, lambda: AR.section(ev, f, cap_rows=19))   # 10 rows an evaluation
    for at in (0, 2):
        cs = [AR.sized_circuit(rng, 4, 8, zero=(i != at)) for i in range(3)]
        ev, f = AR.make_list(cs)
        expect(AR, 6, at, lambda: AR.section(ev, f))
    # an earlier evaluation's kind 4 goes before a later one's kind 1; within an evaluation the header kinds go first
    ev, f = good()
    ev["num_vars"][2] = 3
    f[int(ev["payload"][1]) + 8] = AR.encode(0, 0, 3)
    expect(AR, 4, 1, lambda: AR.section(ev, f), gate=0)
    # the frame: one row too many
    secs = [np.zeros((8, 20), dtype=np.uint64), np.zeros((56, 13), dtype=np.uint64)] + [np.zeros((0, w), dtype=np.uint64) for w in (17, 16, 5)]
    with pytest.raises(FR.Defect) as e:
        FR.stack(secs, log_n=6)
    assert (e.value.section, e.value.kind, e.value.index) == (5, 1, 65)
    secs[1], secs[2] = secs[1][:48], np.zeros((7, 17), dtype=np.uint64)
    t, st, pad, trace_len = FR.stack(secs, log_n=6)     # trace_len == 2^log_n: one padding row
    assert (st, pad, trace_len) == ([0, 8, 56, 63, 63], 63, 64) and (t[63:, 0:5] == 1).all() and not t[63:, 5:21].any()

